// K27 of libwb2hip.so: the structure functions of forecast and truth and the
// variogram score (Scheuerer & Hamill 2015), the verification of the
// DIFFERENCES between grid points that the pointwise tables and the energy
// score (Pinson & Tastu 2013) are nearly blind to.  The reference has no
// counterpart.
//
//   wb2_variogram_sums  sums[o][i][c][l][0..2] = the sums of gy, gf and sc over
//                       the valid pairs of lag l whose anchor lies in row i of
//                       outer index o, in a column of class c (float64);
//                       cnt[o][i][c][l][0..1] = the number of valid and of
//                       invalid pairs
//
// A lag is (a, b), a >= 0 rows and b columns, in GRID POINTS; the partner of
// the anchor (i, j) is (i + a, (j + b) mod n_col) and exists iff i + a < n_row.
// One existing pair, truth y, y' and members x_m, x'_m in STORAGE order, all in
// float64 after an exact widening, no fused multiply-add:
//   g(d) = |d| (order 1), d d (order 2), sqrt_rn(|d|) (order 0.5)
//   gy = g(y - y');  G = g(x_0 - x'_0);  G = G + g(x_m - x'_m);  gf = G / M
//   s = gy - gf;  sc = s s
// The pair is invalid iff any of y, y', x_m, x'_m is NaN (K18's rule, at both
// ends).  A pair that does not exist is neither valid nor invalid.
//
// One WAVE (a workgroup of its own) owns one anchor row of one outer index and
// walks it in tiles of 64 columns, as the class-sums layer does.  The truth
// ("member -1") and the members go through wave-private LDS strips, four items
// at a time: per item and per DISTINCT row offset among the lags (0 always)
// the wave requests the tile's 64 columns of that row and a halo of the
// columns that the lags of that row offset reach to the left and to the right,
// the index wrapped at the seam; the four items of up to five row offsets are
// requested before any is stored.  A strip holds columns col0 - 32 .. col0 +
// 95.  Column-shifted partners are read from the strips, never from memory
// again: a lane issues 1 + (distinct non-zero row offsets the row can reach)
// requests per member, plus the halos' share.  Each lane keeps gy, G and one
// invalid bit per lag in registers, every index a compile-time constant (the
// kernel is instantiated for 4, 8 and 16 lag slots).  After the last member
// the lane stores gy, gf, sc of every lag -- +0.0 where the pair is invalid or
// absent -- and the pairs' states in an LDS tile [point][slot] that takes the
// strips' place.  Then the roles turn (K24's walk): lane s < 3 n_lag owns slot
// s = 3 l + term and adds the 64 points in column order, eight LDS reads in
// flight; lanes 3 l and 3 l + 1 also count the valid and the invalid pairs.
// Where the class of the column changes the lane stores its running sum and
// takes up the new class's.  A sum is ONE sequential chain from +0.0 over the
// columns in increasing order, whatever the tiles are.  Plain stores, no
// atomics of any kind.

#include <cstdint>

#include "class_sums.hpp"
#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kVgMaxLag = 16;
constexpr int kVgMaxRowOffset = 16;
constexpr int kVgHalo = 32;                      // max_col_offset
constexpr int kVgStrip = kWave + 2 * kVgHalo;    // columns of one strip
constexpr int kVgAhead = kExceedAhead;           // members in flight
constexpr int kVgRows = 5;                       // row offsets in flight
constexpr int kVgTerm = 3;                       // gy, gf, sc
constexpr long long kVgLds = 64 * 1024;          // budget of one wave
constexpr char kVgTakes[] = "the variogram sums take";

struct VgParams {
  const void* ens;
  const void* truth;
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const int* col_class;         // [n_col]
  double* sums;                 // [n_outer][n_row][n_class][n_lag][3]
  int* cnt;                     // [n_outer][n_row][n_class][n_lag][2]
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class, n_lag, n_off, state_at;
  // distinct row offsets, increasing, off[0] is row offset 0:
  // a | left halo << 8 | right halo << 16
  int off[kVgMaxLag + 1];
  // strip index | a << 8 | (b + kVgHalo) << 16
  int lag[kVgMaxLag];
};

template <int ORDER>
__device__ __forceinline__ double vg_g(double d) {
  if constexpr (ORDER == 1) return __builtin_fabs(d);
  else if constexpr (ORDER == 2) return d * d;
  else return sqrt_rn(__builtin_fabs(d));
}

// column c of a row of n_col, for c in (-n_col, 2 n_col); beyond (columns
// that only a lane past the row end would pair with): the last column
__device__ __forceinline__ int vg_wrap(int c, int n_col) {
  c = c < 0 ? c + n_col : c;
  c = c >= n_col ? c - n_col : c;
  return c >= n_col ? n_col - 1 : c;
}

// One item (the truth or a member) of a tile: the lane's own value and its NL
// partners from the item's strips `s0`, every LDS read requested before any is
// used and no branch among them; at[l] is the partner's place in the strips
// (the lane's own for a lag that is not there: its bit of `bad` is dropped
// later and its g adds +0.0 or a NaN that nobody reads).  TRUTH: acc[l] = g,
// else acc[l] = acc[l] + g.
template <typename T, int ORDER, int NL, bool TRUTH>
__device__ __forceinline__ void vg_item(const T* s0, int lane,
                                        const int (&at)[NL],
                                        double (&acc)[NL], unsigned& bad) {
  const T x0 = s0[kVgHalo + lane];
  T xp[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) xp[l] = s0[at[l] + lane];
  const bool nan0 = is_nan(x0);
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    bad |= nan0 || is_nan(xp[l]) ? 1u << l : 0u;
    const double g = vg_g<ORDER>((double)x0 - (double)xp[l]);
    // (g is no -0.0: +0.0 + g is g, bit for bit)
    if constexpr (TRUTH) acc[l] = g;
    else acc[l] = acc[l] + g;
  }
}

template <typename T, int ORDER, int NL>
__global__ void __launch_bounds__(kWave)
    variogram_sums_kernel(const VgParams p) {
  extern __shared__ double vg_lds[];
  // T strip[kVgAhead][n_off][kVgStrip], then double tile[64][ns] in its place
  T* strip = reinterpret_cast<T*>(vg_lds);
  double* tile = vg_lds;
  int* state = reinterpret_cast<int*>(vg_lds) + p.state_at;  // [64]
  constexpr int G = 8;  // points whose LDS reads are in flight together
  const int lane = threadIdx.x;
  const long long o = outer_index();
  const int row = (int)blockIdx.x;
  if (o >= p.n_outer) return;
  const int M = p.n_member;
  const int n_lag = p.n_lag;
  const int n_off = p.n_off;
  const int n_col = p.n_col;
  const int n_slot = kVgTerm * n_lag;
  const int ns = n_slot | 1;  // (an odd stride of 8 bytes: no bank conflict)

  const long long slab = (long long)p.n_row * n_col;
  const long long first = (long long)row * n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);

  // the slot of this lane
  const bool mine = lane < n_slot;
  const int my_lag = mine ? lane / kVgTerm : 0;
  const int my_term = mine ? lane - my_lag * kVgTerm : 0;
  const bool counts = mine && my_term < 2;
  const long long cell = (o * p.n_row + row) * (long long)p.n_class;
  double* dsum = p.sums + cell * n_slot + (mine ? lane : 0);
  int* dcnt = p.cnt + cell * 2 * n_lag + 2 * my_lag + (counts ? my_term : 0);
  const int my_bit = my_lag + (my_term == 1 ? kVgMaxLag : 0);
  double sum = 0.0;
  int n_in = 0;
  int cur = -1;                 // the class of the running sums
  unsigned long long seen = 0;  // classes this row has met

  auto store_class = [&](int c, double s, int n) {
    if (mine) dsum[(long long)c * n_slot] = s;
    if (counts) dcnt[(long long)c * 2 * n_lag] = n;
  };

  // the row offsets this row reaches (they increase; 0 is always one)
  int n_reach = 0;
  for (int k = 0; k < n_off; ++k) n_reach += row + (p.off[k] & 0xff) < p.n_row;

  // the lags that are there for this row, and where their partners lie
  int at[NL];
  unsigned there = 0;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int w = p.lag[l];
    const int k = w & 0xff, a = (w >> 8) & 0xff, bpos = w >> 16;
    const bool on = l < n_lag && row + a < p.n_row;  // wave-uniform
    at[l] = on ? k * kVgStrip + bpos : kVgHalo;
    there |= on ? 1u << l : 0u;
  }

  const int n_tile = (n_col + kWave - 1) / kWave;
  for (int tcol = 0; tcol < n_tile; ++tcol) {
    const int col0 = tcol * kWave;
    const bool active = col0 + lane < n_col;
    const int cls_v = p.col_class[active ? col0 + lane : n_col - 1];
    // a lane past the end of the row holds the column its neighbours wrap to
    const int main_bytes = vg_wrap(col0 + lane, n_col) * (int)sizeof(T);

    double gy[NL], Gm[NL];
    unsigned bad = 0;  // bit l: the pair of lag l holds a NaN
#pragma unroll
    for (int l = 0; l < NL; ++l) gy[l] = Gm[l] = 0.0;

    // item -1 is the truth, item m >= 0 member m: kVgAhead items at a time
    for (int m0 = -1; m0 < M; m0 += kVgAhead) {
      const int nu = M - m0 < kVgAhead ? M - m0 : kVgAhead;
      long long stride = p.member_stride;
      asm volatile("" : "+s"(stride));
      // (the strips' or the tile's reads of the round before are done)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // kVgRows row offsets of the kVgAhead items are requested before any is
      // stored
      for (int k0 = 0; k0 < n_reach; k0 += kVgRows) {
        T v[kVgRows][kVgAhead], h[kVgRows][kVgAhead];
        int hpos[kVgRows];
        bool halo[kVgRows];
#pragma unroll
        for (int kk = 0; kk < kVgRows; ++kk) {
          const bool live = k0 + kk < n_reach;  // wave-uniform
          const int w = p.off[live ? k0 + kk : 0];
          const int a = w & 0xff, hl = (w >> 8) & 0xff, hr = (w >> 16) & 0xff;
          // the halo: lanes [0, hl) the columns to the left, nearest first,
          // lanes [hl, hl + hr) the columns to the right
          halo[kk] = live && lane < hl + hr;
          hpos[kk] = lane < hl ? kVgHalo - 1 - lane
                               : kVgHalo + kWave + (lane - hl);
          const int hcol = halo[kk] ? col0 + hpos[kk] - kVgHalo : col0;
          const int halo_bytes = vg_wrap(hcol, n_col) * (int)sizeof(T);
          const long long down = (long long)a * n_col;
#pragma unroll
          for (int u = 0; u < kVgAhead; ++u) {
            const T* rb = (m0 + u < 0 ? tb : xb + (m0 + u) * stride) + down;
            // a dead slot reads nothing
            const int rec = live && u < nu ? 0x7fffffff : 0;
            v[kk][u] = member_load<T>(rb, main_bytes, rec);
            h[kk][u] = (T)0;
            if (halo[kk]) h[kk][u] = member_load<T>(rb, halo_bytes, rec);
          }
        }
#pragma unroll
        for (int kk = 0; kk < kVgRows; ++kk) {
          if (k0 + kk >= n_reach) break;
#pragma unroll
          for (int u = 0; u < kVgAhead; ++u) {
            T* s = strip + (u * n_off + k0 + kk) * kVgStrip;
            s[kVgHalo + lane] = v[kk][u];
            if (halo[kk]) s[hpos[kk]] = h[kk][u];
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const int item = n_off * kVgStrip;  // the strips of one item
      if (m0 >= 0 && nu == kVgAhead) {
        // a whole group of members: no branch, the LDS reads of all in flight
#pragma unroll
        for (int u = 0; u < kVgAhead; ++u)
          vg_item<T, ORDER, NL, false>(strip + u * item, lane, at, Gm, bad);
      } else {
        int u = 0;
        if (m0 < 0) {
          vg_item<T, ORDER, NL, true>(strip, lane, at, gy, bad);
          u = 1;
        }
        for (; u < nu; ++u)
          vg_item<T, ORDER, NL, false>(strip + u * item, lane, at, Gm, bad);
      }
    }
    bad &= there;

    const unsigned long long change = class_change(cls_v, cur, lane);

    // the strips are done with: the tile takes their place
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    unsigned st = 0;  // bit l: valid, bit 16 + l: invalid
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (l >= n_lag) break;
      const bool pair = active && ((there >> l) & 1u);
      const bool isbad = (bad >> l) & 1u;
      const bool ok = pair && !isbad;
      st |= ok ? 1u << l : 0u;
      st |= pair && isbad ? 1u << (kVgMaxLag + l) : 0u;
      const double gf = Gm[l] / (double)M;
      const double s = gy[l] - gf;
      const double sc = s * s;
      double* d = tile + lane * ns + kVgTerm * l;
      d[0] = ok ? gy[l] : 0.0;
      d[1] = ok ? gf : 0.0;
      d[2] = ok ? sc : 0.0;
    }
    state[lane] = (int)st;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const double* mytile = tile + (mine ? lane : 0);
    const int n_here = n_col - col0 < kWave ? n_col - col0 : kWave;
    for (int j0 = 0; j0 < n_here; j0 += G) {
      const unsigned all = (1u << G) - 1;
      if (j0 + G <= n_here && ((unsigned)(change >> j0) & all) == 0) {
        // G points of the running class: the same additions in the same order
        // as below, their LDS reads requested together
        double w[G];
        int b[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          b[u] = state[j0 + u];
          w[u] = mytile[(j0 + u) * ns];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          sum = sum + w[u];
          n_in += (b[u] >> my_bit) & 1;
        }
        continue;
      }
      const int j1 = j0 + G < n_here ? j0 + G : n_here;
      for (int j = j0; j < j1; ++j) {
        const int c = __builtin_amdgcn_readlane(cls_v, j);
        if (c != cur) {
          if (cur >= 0) store_class(cur, sum, n_in);
          cur = c;
          sum = 0.0;
          n_in = 0;
          if ((seen >> c) & 1) {  // (a lane reads back its own stores)
            if (mine) sum = dsum[(long long)c * n_slot];
            if (counts) n_in = dcnt[(long long)c * 2 * n_lag];
          }
          seen |= 1ull << c;
        }
        sum = sum + mytile[j * ns];
        n_in += (state[j] >> my_bit) & 1;
      }
    }
  }
  if (cur >= 0) store_class(cur, sum, n_in);
  for (int c = 0; c < p.n_class; ++c)
    if (!((seen >> c) & 1)) store_class(c, 0.0, 0);
}

struct VgPlan {
  int n_off;
  int off[kVgMaxLag + 1];
  int lag[kVgMaxLag];
  long long strip_bytes, tile_bytes, lds_bytes;
  int state_at;  // in ints
};

// Every check that needs no operand, and the strips of the lags.  0 or
// negative.
inline int vg_shape(int dtype, int n_member, int n_class, int order_code,
                    const int32_t* lags, int n_lag, int n_col, bool sized,
                    VgPlan* q) {
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_member >= 1 && n_member <= kExceedMaxMember,
              "n_member=%d: %s 1 to %d members", n_member, kVgTakes,
              kExceedMaxMember);
  WB2_REQUIRE(n_class >= 1 && n_class <= kExceedMaxClass,
              "n_class=%d: %s 1 to %d column classes", n_class, kVgTakes,
              kExceedMaxClass);
  WB2_REQUIRE(n_lag >= 1 && n_lag <= kVgMaxLag, "n_lag=%d: %s 1 to %d lags",
              n_lag, kVgTakes, kVgMaxLag);
  WB2_REQUIRE(order_code >= 0 && order_code <= 2,
              "order_code=%d: %s 0 (order 0.5), 1 (order 1) or 2 (order 2)",
              order_code, kVgTakes);
  WB2_REQUIRE(lags, "null pointer argument");
  bool has[kVgMaxRowOffset + 1] = {true};
  for (int l = 0; l < n_lag; ++l) {
    const int a = lags[2 * l], b = lags[2 * l + 1];
    WB2_REQUIRE(a >= 0 && a <= kVgMaxRowOffset,
                "lag %d: row offset a=%d: %s 0 to %d", l, a, kVgTakes,
                kVgMaxRowOffset);
    WB2_REQUIRE(b >= -kVgHalo && b <= kVgHalo,
                "lag %d: column offset b=%d: %s -%d to %d", l, b, kVgTakes,
                kVgHalo, kVgHalo);
    WB2_REQUIRE(!sized || n_col <= 0 || (b > -n_col && b < n_col),
                "lag %d: column offset b=%d: |b| must be below n_col=%d", l, b,
                n_col);
    WB2_REQUIRE(a != 0 || b != 0, "lag %d is (0, 0): a point is no pair", l);
    has[a] = true;
  }
  int index[kVgMaxRowOffset + 1];
  q->n_off = 0;
  for (int a = 0; a <= kVgMaxRowOffset; ++a)
    if (has[a]) {
      index[a] = q->n_off;
      q->off[q->n_off++] = a;
    }
  for (int l = 0; l < n_lag; ++l) {
    const int a = lags[2 * l], b = lags[2 * l + 1];
    const int k = index[a];
    int hl = (q->off[k] >> 8) & 0xff, hr = (q->off[k] >> 16) & 0xff;
    if (-b > hl) hl = -b;
    if (b > hr) hr = b;
    q->off[k] = a | hl << 8 | hr << 16;
    q->lag[l] = k | a << 8 | (b + kVgHalo) << 16;
  }
  const long long elem = dtype == WB2_F32 ? 4 : 8;
  q->strip_bytes = (long long)kVgAhead * q->n_off * kVgStrip * elem;
  q->tile_bytes = (long long)kWave * ((kVgTerm * n_lag) | 1) * 8;
  const long long body =
      q->strip_bytes > q->tile_bytes ? q->strip_bytes : q->tile_bytes;
  q->state_at = (int)(body / 4);
  q->lds_bytes = body + kWave * 4;
  WB2_REQUIRE(q->lds_bytes <= kVgLds,
              "the strips of %d row offsets and the tile of %d lags take %lld "
              "bytes: over the LDS budget of %lld bytes", q->n_off, n_lag,
              q->lds_bytes, kVgLds);
  return 0;
}

// f(T{}, integral_constant<ORDER>{}, integral_constant<NL>{}): the dtype, the
// order code and the least instantiated lag slots that hold n_lag
template <class F>
void for_variogram(int dtype, int order_code, int n_lag, F&& f) {
  auto slots = [&](auto T0, auto O) {
    if (n_lag <= 4) f(T0, O, std::integral_constant<int, 4>{});
    else if (n_lag <= 8) f(T0, O, std::integral_constant<int, 8>{});
    else f(T0, O, std::integral_constant<int, 16>{});
  };
  auto order = [&](auto T0) {
    if (order_code == 0) slots(T0, std::integral_constant<int, 0>{});
    else if (order_code == 1) slots(T0, std::integral_constant<int, 1>{});
    else slots(T0, std::integral_constant<int, 2>{});
  };
  if (dtype == WB2_F32) order(float{});
  else order(double{});
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_variogram_geometry(int dtype, int32_t n_member, int32_t n_class,
                           int order_code, const int32_t* lags, int32_t n_lag,
                           int32_t* min_member, int32_t* max_member,
                           int32_t* max_lags, int32_t* max_row_offset,
                           int32_t* max_col_offset, int32_t* tile_cols,
                           int32_t* rows_per_group, int64_t* lds_bytes,
                           int32_t* max_grid_outer) {
  using namespace wb2;
  VgPlan plan{};
  if (const int rc = vg_shape(dtype, n_member, n_class, order_code, lags, n_lag,
                              0, false, &plan))
    return rc;
  WB2_REQUIRE(max_lags && max_row_offset && max_col_offset && lds_bytes,
              "null pointer argument");
  *max_lags = kVgMaxLag;
  *max_row_offset = kVgMaxRowOffset;
  *max_col_offset = kVgHalo;
  *lds_bytes = plan.lds_bytes;
  if (const int rc = class_geometry(min_member, max_member, tile_cols,
                                    rows_per_group, max_grid_outer))
    return rc;
  *max_member = kExceedMaxMember;
  return 0;
}

int wb2_variogram_sums(int dtype, const void* ens, const int64_t* ens_slab,
                       const void* truth, const int64_t* truth_slab,
                       int32_t n_member, int64_t member_stride,
                       int64_t n_outer, int32_t n_row, int32_t n_col,
                       const int32_t* col_class, int32_t n_class,
                       int order_code, const int32_t* lags, int32_t n_lag,
                       double* sums, int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  VgPlan plan{};
  if (const int rc = vg_shape(dtype, n_member, n_class, order_code, lags, n_lag,
                              n_col, true, &plan))
    return rc;
  VgParams p{};
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, &p);
  if (go <= 0) return go;
  if (const int rc = class_operands(col_class, sums, cnt, n_row, n_col,
                                    n_class, &p))
    return rc;
  p.n_lag = n_lag;
  p.n_off = plan.n_off;
  p.state_at = plan.state_at;
  for (int k = 0; k < plan.n_off; ++k) p.off[k] = plan.off[k];
  for (int l = 0; l < n_lag; ++l) p.lag[l] = plan.lag[l];
  dim3 grid, block;
  if (const int rc = class_grid(n_outer, n_row, &grid, &block)) return rc;
  for_variogram(dtype, order_code, n_lag, [&](auto T0, auto O, auto NL) {
    hipLaunchKernelGGL(
        (variogram_sums_kernel<decltype(T0), decltype(O)::value,
                               decltype(NL)::value>),
        grid, block, (size_t)plan.lds_bytes, static_cast<hipStream_t>(stream),
        p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
