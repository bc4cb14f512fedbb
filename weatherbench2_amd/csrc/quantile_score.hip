// K28 of libwb2hip.so: the per-level sums of quantile verification -- the
// pinball (quantile) loss, the forecast quantile itself and the counts of the
// truth below / at the quantile, from which the host forms the quantile score,
// quantile reliability and the coverage, width and interval score (Winkler
// 1972) of central prediction intervals.  The reference has no counterpart.
//
//   wb2_quantile_score_sums  sums[o][i][c][l][0..1] = the sums of pinball and
//                            q over the valid points of the columns of class c
//                            in row i of outer index o, level l (float64);
//                            cnt[o][i][c][l][0..1] = the points with y < q and
//                            with y == q; valid[o][i][c][0..1] = the valid and
//                            the invalid points
//
// One point, truth y, level l with the host's tables lo, hi, t, tau, 1 - tau,
// all in float64 after an exact widening, no fused multiply-add:
//   ensemble mode (0): members sorted x_0 <= ... <= x_{M-1};
//     d = x_hi - x_lo in the DATA's dtype;
//     q = x_lo + d t (t < 1/2), q = x_hi - d (1 - t) otherwise (K12's lerp)
//   direct mode (1): the M "members" are the quantile values in storage order;
//     q = x_lo, nothing is sorted or interpolated
//   u = y - q;  pinball = tau u (u >= 0), (1 - tau) (-u) otherwise
//   below = y < q, tie = y == q (IEEE compares)
// The point is invalid iff the truth or any member is NaN (K18's rule).
//
// One WAVE (a workgroup of its own) owns one row of one outer index and walks
// it in tiles of 64 columns, in column order.  Per tile a lane requests its
// point's class, truth and members, all before any is looked at (each row is
// read once: (M + 1) elements per point), sorts the members in registers with
// the padded networks of ensemble_kernels.hpp (K20's front) and stores them
// in a wave-private LDS tile [M][64] (the truth is needed by its own lane
// alone and stays in a register).  The lane stays with its point: per level
// it reads x_lo and x_hi back from the tile at the wave-uniform rows lo[l],
// hi[l] -- no register is ever indexed by a run-time value -- and keeps q,
// pinball and the two flags under compile-time slot indices.  Those go, +0.0
// where the point is invalid, into an LDS tile [point][2 n_level | 1] that
// takes the members' place, the flags as one word per point beside it.  Then
// lane s < 2 n_level takes slot s = 2 l + term and
// adds the points of the tile in column order, eight LDS reads in flight
// (K24's walk); lane 2 l counts `below`, lane 2 l + 1 `tie` of level l, and
// every lane counts the valid and the invalid points from two ballots (lane 0
// stores them).  Where the class of the column changes (wave-uniform) the lane
// stores its sum and takes up the new class's -- read back if the row met the
// class before, 0 otherwise: the sum of a (row, class, level, term) is ONE
// sequential chain over its columns in increasing order, whatever the tiles
// are.  Plain stores, no atomics of any kind.
//
// The requests of a tile, the mask of class changes and the host side are
// class_sums.hpp's.

#include <cstdint>
#include <limits>

#include "class_sums.hpp"
#include "common.hpp"
#include "ensemble_kernels.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kQsMaxLevel = 16;           // levels of one launch
constexpr int kQsTerm = 2;                // pinball, q
constexpr long long kQsLds = 64 * 1024;   // budget of one wave
constexpr char kQsTakes[] = "the quantile score sums take";

struct QsParams {
  const void* ens;
  const void* truth;
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const int* col_class;         // [n_col]
  double* sums;                 // [n_outer][n_row][n_class][n_level][2]
  int* cnt;                     // [n_outer][n_row][n_class][n_level][2]
  int* valid;                   // [n_outer][n_row][n_class][2]
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class, n_level, direct, state_at;
  int lo[kQsMaxLevel], hi[kQsMaxLevel];
  double t[kQsMaxLevel], tau[kQsMaxLevel], one_minus_tau[kQsMaxLevel];
};

template <typename T, int NPAD, int NL>
__global__ void __launch_bounds__(kWave)
    quantile_score_sums_kernel(const QsParams p) {
  extern __shared__ double qs_lds[];
  // T member[M][64] (the truth stays in its lane's register), then double
  // tile[64][ns] in its place
  T* member = reinterpret_cast<T*>(qs_lds);
  double* tile = qs_lds;
  unsigned* state = reinterpret_cast<unsigned*>(qs_lds) + p.state_at;  // [64]
  constexpr int G = 8;  // points whose LDS reads are in flight together
  const int lane = threadIdx.x;
  const long long o = outer_index();
  const int row = (int)blockIdx.x;
  if (o >= p.n_outer) return;
  const int M = p.n_member;
  const int n_level = p.n_level;
  const bool direct = p.direct != 0;
  const int n_slot = kQsTerm * n_level;
  const int ns = n_slot | 1;  // (an odd stride of 8 bytes: no bank conflict)
  const T inf = std::numeric_limits<T>::infinity();

  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);

  // the slot of this lane: bit my_bit of a point's word is what it counts
  const bool mine = lane < n_slot;
  const int my_level = mine ? lane / kQsTerm : 0;
  const int my_term = mine ? lane - my_level * kQsTerm : 0;
  const int my_bit = my_level + (my_term == 1 ? kQsMaxLevel : 0);
  const long long cell = (o * p.n_row + row) * (long long)p.n_class;
  double* dsum = p.sums + cell * n_slot + (mine ? lane : 0);
  int* dcnt = p.cnt + cell * n_slot + (mine ? lane : 0);
  int* dvalid = p.valid + cell * 2;
  double sum = 0.0;
  int n_in = 0, n_valid = 0, n_invalid = 0;
  int cur = -1;                 // the class of the running sums
  unsigned long long seen = 0;  // classes this row has met

  auto store_class = [&](int c, double s, int n, int nv, int ni) {
    if (mine) {
      dsum[(long long)c * n_slot] = s;
      dcnt[(long long)c * n_slot] = n;
    }
    if (lane == 0) {
      dvalid[2 * c] = nv;
      dvalid[2 * c + 1] = ni;
    }
  };

  const int n_tile = (p.n_col + kWave - 1) / kWave;
  for (int tcol = 0; tcol < n_tile; ++tcol) {
    const int col0 = tcol * kWave;
    const bool active = col0 + lane < p.n_col;
    // a lane past the end of the row reads its last column again
    const int colc = active ? col0 + lane : p.n_col - 1;
    int cls_v, Mt;
    T y, x[NPAD];
    class_tile<T, NPAD>(xb, tb, p.col_class, p.member_stride, M, colc, cls_v, y,
                        Mt, x, [] {});
    bool bad = is_nan(y);
#pragma unroll
    for (int m = 0; m < NPAD; ++m) {
      const bool live = m < Mt;  // wave-uniform
      bad = bad || (live && is_nan(x[m]));
      // NaN -> +inf (v_min returns the other operand; the point is invalid
      // and never summed), dead slots +inf: they sort behind every member
      x[m] = live ? vmin(x[m], inf) : inf;
    }
    if (!direct && M > 1) sort_network<NPAD, NPAD>(x);
    const bool ok = active && !bad;
    const unsigned long long ok_mask = __ballot(ok);
    const unsigned long long bad_mask = __ballot(active && bad);
    const unsigned long long change = class_change(cls_v, cur, lane);

    // the DS operations of one wave execute in order; the fences restrain the
    // compiler.  (The walk's reads of the tile before are done.)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int m = 0; m < NPAD; ++m)
      if (m < Mt) member[m * kWave + lane] = x[m];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    // lane = point: the NL levels, every read requested before any is used
    const double yd = (double)y;
    T xlo[NL], xhi[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const bool on = l < n_level;  // wave-uniform
      xlo[l] = member[(on ? p.lo[l] : 0) * kWave + lane];
      xhi[l] = member[(on ? p.hi[l] : 0) * kWave + lane];
    }
    double q[NL], pin[NL];
    unsigned st = 0;  // bit l: below, bit 16 + l: tie
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (l >= n_level) break;
      const double t = p.t[l];
      const double d = (double)(T)(xhi[l] - xlo[l]);
      const double low = (double)xlo[l] + d * t;
      const double high = (double)xhi[l] - d * (1.0 - t);
      const double ql = direct ? (double)xlo[l] : (t < 0.5 ? low : high);
      const double u = yd - ql;
      const double up = p.tau[l] * u;
      const double down = p.one_minus_tau[l] * (-u);
      q[l] = ok ? ql : 0.0;
      pin[l] = ok ? (u >= 0.0 ? up : down) : 0.0;
      st |= ok && yd < ql ? 1u << l : 0u;
      st |= ok && yd == ql ? 1u << (kQsMaxLevel + l) : 0u;
    }

    // the members are done with: the tile takes their place
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (l >= n_level) break;
      double* d = tile + lane * ns + kQsTerm * l;
      d[0] = pin[l];
      d[1] = q[l];
    }
    state[lane] = st;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const double* mytile = tile + (mine ? lane : 0);
    const int n_here = p.n_col - col0 < kWave ? p.n_col - col0 : kWave;
    for (int j0 = 0; j0 < n_here; j0 += G) {
      const unsigned all = (1u << G) - 1;
      if (j0 + G <= n_here && ((unsigned)(change >> j0) & all) == 0) {
        // G points of the running class: the same additions in the same order
        // as below, their LDS reads requested together
        double w[G];
        unsigned b[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          b[u] = state[j0 + u];
          w[u] = mytile[(j0 + u) * ns];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          sum = sum + w[u];
          n_in += (int)((b[u] >> my_bit) & 1u);
        }
        n_valid += __builtin_popcount((unsigned)(ok_mask >> j0) & all);
        n_invalid += __builtin_popcount((unsigned)(bad_mask >> j0) & all);
        continue;
      }
      const int j1 = j0 + G < n_here ? j0 + G : n_here;
      for (int j = j0; j < j1; ++j) {
        const int c = __builtin_amdgcn_readlane(cls_v, j);
        if (c != cur) {
          if (cur >= 0) store_class(cur, sum, n_in, n_valid, n_invalid);
          cur = c;
          sum = 0.0;
          n_in = n_valid = n_invalid = 0;
          if ((seen >> c) & 1) {  // (a lane reads back its own stores)
            if (mine) {
              sum = dsum[(long long)c * n_slot];
              n_in = dcnt[(long long)c * n_slot];
            }
            if (lane == 0) {
              n_valid = dvalid[2 * c];
              n_invalid = dvalid[2 * c + 1];
            }
          }
          seen |= 1ull << c;
        }
        sum = sum + mytile[j * ns];
        n_in += (int)((state[j] >> my_bit) & 1u);
        n_valid += (int)((ok_mask >> j) & 1ull);
        n_invalid += (int)((bad_mask >> j) & 1ull);
      }
    }
  }
  if (cur >= 0) store_class(cur, sum, n_in, n_valid, n_invalid);
  for (int c = 0; c < p.n_class; ++c)
    if (!((seen >> c) & 1)) store_class(c, 0.0, 0, 0, 0);
}

struct QsPlan {
  long long member_bytes, tile_bytes, lds_bytes;
  int state_at;  // in ints
};

// Every check that needs no operand, and the LDS plan.  0 or negative.
inline int qs_shape(int dtype, int n_member, int n_class, int mode,
                    int n_level, QsPlan* q) {
  if (const int rc = class_shape(kQsTakes, dtype, n_member, n_class)) return rc;
  WB2_REQUIRE(mode == 0 || mode == 1,
              "mode=%d: %s 0 (sorted ensemble) or 1 (direct quantiles)", mode,
              kQsTakes);
  WB2_REQUIRE(n_level >= 1 && n_level <= kQsMaxLevel,
              "n_level=%d: %s 1 to %d levels", n_level, kQsTakes, kQsMaxLevel);
  const long long elem = dtype == WB2_F32 ? 4 : 8;
  q->member_bytes = (long long)n_member * kWave * elem;
  q->tile_bytes = (long long)kWave * ((kQsTerm * n_level) | 1) * 8;
  const long long body =
      q->member_bytes > q->tile_bytes ? q->member_bytes : q->tile_bytes;
  q->state_at = (int)(body / 4);
  q->lds_bytes = body + kWave * 4;
  WB2_REQUIRE(q->lds_bytes <= kQsLds,
              "the tile of %d members and %d levels takes %lld bytes: over the "
              "LDS budget of %lld bytes", n_member, n_level, q->lds_bytes,
              kQsLds);
  return 0;
}

// f(T{}, integral_constant<NPAD>{}, integral_constant<NL>{}): for_npad() and
// the least instantiated level slots that hold n_level
template <class F>
void for_quantile_score(int dtype, int n_member, int n_level, F&& f) {
  for_npad(dtype, n_member, [&](auto T0, auto N) {
    if (n_level <= 4) f(T0, N, std::integral_constant<int, 4>{});
    else if (n_level <= 8) f(T0, N, std::integral_constant<int, 8>{});
    else f(T0, N, std::integral_constant<int, 16>{});
  });
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_quantile_score_geometry(int dtype, int32_t n_member, int32_t n_class,
                                int mode, int32_t n_level,
                                int32_t* min_member, int32_t* max_member,
                                int32_t* max_levels, int32_t* tile_cols,
                                int32_t* rows_per_group, int64_t* lds_bytes,
                                int32_t* max_grid_outer) {
  using namespace wb2;
  QsPlan plan{};
  if (const int rc = qs_shape(dtype, n_member, n_class, mode, n_level, &plan))
    return rc;
  WB2_REQUIRE(max_levels && lds_bytes, "null pointer argument");
  *max_levels = kQsMaxLevel;
  *lds_bytes = plan.lds_bytes;
  return class_geometry(min_member, max_member, tile_cols, rows_per_group,
                        max_grid_outer);
}

int wb2_quantile_score_sums(int dtype, const void* ens, const int64_t* ens_slab,
                            const void* truth, const int64_t* truth_slab,
                            int32_t n_member, int64_t member_stride,
                            int64_t n_outer, int32_t n_row, int32_t n_col,
                            const int32_t* col_class, int32_t n_class, int mode,
                            int32_t n_level, const int32_t* lo,
                            const int32_t* hi, const double* t,
                            const double* tau, const double* one_minus_tau,
                            double* sums, int32_t* cnt, int32_t* valid,
                            void* stream) {
  WB2_TRACE();
  using namespace wb2;
  QsPlan plan{};
  if (const int rc = qs_shape(dtype, n_member, n_class, mode, n_level, &plan))
    return rc;
  WB2_REQUIRE(lo && hi && t && tau && one_minus_tau, "null pointer argument");
  QsParams p{};
  for (int l = 0; l < n_level; ++l) {
    // (the kernel reads the members' tile at these rows)
    WB2_REQUIRE(lo[l] >= 0 && lo[l] <= hi[l] && hi[l] < n_member,
                "level %d: positions lo=%d, hi=%d: %s 0 <= lo <= hi < "
                "n_member=%d", l, (int)lo[l], (int)hi[l], kQsTakes, n_member);
    WB2_REQUIRE(mode == 0 || lo[l] == hi[l],
                "level %d: positions lo=%d, hi=%d: direct quantiles take lo == "
                "hi", l, (int)lo[l], (int)hi[l]);
    p.lo[l] = lo[l];
    p.hi[l] = hi[l];
    p.t[l] = t[l];
    p.tau[l] = tau[l];
    p.one_minus_tau[l] = one_minus_tau[l];
  }
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, &p);
  if (go <= 0) return go;
  WB2_REQUIRE(valid, "null pointer argument");
  if (const int rc = class_operands(col_class, sums, cnt, n_row, n_col,
                                    n_class, &p))
    return rc;
  p.valid = valid;
  p.n_level = n_level;
  p.direct = mode;
  p.state_at = plan.state_at;
  dim3 grid, block;
  if (const int rc = class_grid(n_outer, n_row, &grid, &block)) return rc;
  for_quantile_score(dtype, n_member, n_level, [&](auto T0, auto N, auto NL) {
    hipLaunchKernelGGL(
        (quantile_score_sums_kernel<decltype(T0), decltype(N)::value,
                                    decltype(NL)::value>),
        grid, block, (size_t)plan.lds_bytes, static_cast<hipStream_t>(stream),
        p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
