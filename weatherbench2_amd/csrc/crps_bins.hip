// K20 of libwb2hip.so: the per-rank-bin sums of Hersbach's CRPS decomposition
// (Wea. Forecasting 2000).  The reference has the CRPS itself (metrics.py:
// 760-830) and no counterpart of the decomposition.
//
//   wb2_crps_bin_sums  sums[o][i][c][0][b] = the sum of alpha_b, sums[..][1][b]
//                      = the sum of beta_b over the valid points of the columns
//                      of class c in row i of outer index o (float64);
//                      cnt[o][i][c][0..2] = the below-, above- and valid counts
//   wb2_crps_bin_fold  table[cell][r][s] = sum_i wrow[r][i] *
//                      (sum_c mult[r][c] * sums[cell][i][c][s])
//
// One point, members sorted x_1 <= ... <= x_M, truth y, all in float64 after an
// exact widening: bin 0: beta = max(x_1 - y, 0); bin M: alpha = max(y - x_M,
// 0); bins 0 < b < M: c = min(max(y, x_b), x_{b+1}), alpha = c - x_b, beta =
// x_{b+1} - c; alpha_0 = beta_M = 0.  below = y < x_1, above = y > x_M (strict).
// Invalid iff the truth or any member is NaN (K18's rule).
//
// One WAVE (a workgroup of its own) owns one row of one outer index and walks
// it in tiles of 64 columns, in column order.  Per tile a lane requests its
// point's members, all before any is looked at (each row is read once: (M + 1)
// elements per point), sorts them in registers with the networks of
// ensemble_kernels.hpp (+inf padding up to the next power of two) and stores
// the M sorted values and the truth in a wave-private LDS tile [M + 1][64 + 1]
// (the odd pitch: the transposed reads below hit 64 banks).  Then the roles
// turn: lane b (1 <= b < M) owns bin b, lane 0 owns beta_0 and alpha_M, and
// the wave walks the 64 points of the tile in column order, eight at a time;
// every lane reads x_b, x_{b+1} and y of a point (three LDS reads, two
// conflict-free, one a broadcast), forms its alpha and beta and adds them to
// its two running float64 sums.  The 2 (M + 1) values of a point thus never
// exist in one lane: they are made where they are added.  The running sums
// belong to the class of the current column; where the class changes (a
// wave-uniform test; classes are mostly runs of columns) the lane stores them
// to the output and loads the sums of the new class (0 where the row has not
// met it): the sum of a (row, class) is ONE sequential chain over its columns
// in increasing order, whatever the tiles are.  The outlier counts are the
// signs of lane 0's two terms.  Plain stores, no atomics of any kind.
//
// The host side is class_sums.hpp's, shared with K21 and K24.  The kernel keeps
// its own copy of that layer's class_tile() and class_change(): with either
// inlined the float32 64-slot form is 1.6 % slower (profiles/NOTES.md).

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

constexpr int kCrpsPitch = kWave + 1;
constexpr int kCrpsFoldThreads = 256;  // (the sums kernel: one wave)
constexpr char kCrpsTakes[] = "the CRPS bin sums take";

struct CrpsParams {
  const void* ens;
  const void* truth;
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const int* col_class;         // [n_col]
  double* sums;                 // [n_outer][n_row][n_class][2][M + 1]
  int* cnt;                     // [n_outer][n_row][n_class][3]
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class;
};

__device__ __forceinline__ void crps_terms(int lane, double yj, double lo,
                                           double hi, double& a, double& b) {
  double cl = yj < lo ? lo : yj;
  cl = cl > hi ? hi : cl;
  const double over = yj - lo, under = hi - yj;  // lane 0: lo = x_M, hi = x_1
  a = lane == 0 ? (over > 0.0 ? over : 0.0) : cl - lo;
  b = lane == 0 ? (under > 0.0 ? under : 0.0) : hi - cl;
}

template <typename T, int NPAD>
__global__ void __launch_bounds__(kWave)
    crps_bin_sums_kernel(const CrpsParams p) {
  extern __shared__ double crps_tiles[];  // [M + 1][kCrpsPitch] of T
  constexpr int G = 8;  // points whose LDS reads are in flight together
  const int lane = threadIdx.x;
  const long long o = outer_index();
  const int row = (int)blockIdx.x;
  if (o >= p.n_outer) return;
  const int M = p.n_member;
  const int nb = M + 1;
  T* tile = reinterpret_cast<T*>(crps_tiles);
  const T inf = std::numeric_limits<T>::infinity();

  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);
  const long long cell = (o * p.n_row + row) * p.n_class;
  double* srow = p.sums + cell * 2 * nb;
  int* crow = p.cnt + cell * 3;

  // the bins of this lane: alpha_ia from (x_lo, y), beta_lane from (y, x_hi)
  const bool mine = lane < M;
  const int ia = lane == 0 ? M : lane;
  const T* t_lo = tile + (lane == 0 ? M - 1 : (mine ? lane - 1 : 0)) *
                             kCrpsPitch;
  const T* t_hi = tile + (mine ? lane : 0) * kCrpsPitch;
  const T* t_y = tile + M * kCrpsPitch;
  double sum_a = 0.0, sum_b = 0.0;
  // (lane 0's are stored: its alpha and beta are the two outlier distances)
  int n_below = 0, n_above = 0, n_valid = 0;
  int cur = -1;                 // the class of the running sums
  unsigned long long seen = 0;  // classes this row has met

  auto store_class = [&](int c, double a, double b, int n0, int n1, int n2) {
    double* d = srow + (long long)c * 2 * nb;
    if (mine) {
      d[ia] = a;
      d[nb + lane] = b;
    }
    if (lane == 0) {
      d[0] = 0.0;        // alpha_0
      d[nb + M] = 0.0;   // beta_M
      int* n = crow + c * 3;
      n[0] = n0;
      n[1] = n1;
      n[2] = n2;
    }
  };

  const int n_tile = (p.n_col + kWave - 1) / kWave;
  for (int tcol = 0; tcol < n_tile; ++tcol) {
    const int col0 = tcol * kWave;
    const bool active = col0 + lane < p.n_col;
    // a lane past the end of the row reads its last column again
    const int colc = active ? col0 + lane : p.n_col - 1;
    const int cls_v = p.col_class[colc];
    const T y = tb[colc];
    // every member is requested before any is looked at: the bases are
    // wave-uniform (K3's buffer loads), a slot >= M is switched off through
    // its descriptor and costs no memory access.  (The stride is made opaque
    // per tile, or hipcc keeps all NPAD bases in SGPRs across the tile loop.)
    // (So is the member count: the NPAD tests `m < M` are scalar compares
    // made where they are used, not lane masks and descriptors kept in SGPRs.)
    long long stride = p.member_stride;
    int Mt = M;
    asm volatile("" : "+s"(stride), "+s"(Mt));
    const int lane_bytes = colc * (int)sizeof(T);
    T x[NPAD];
#pragma unroll
    for (int m = 0; m < NPAD; ++m)
      x[m] = member_load<T, true>(xb + m * stride, lane_bytes,
                                  m < Mt ? 0x7fffffff : 0);
    bool bad = is_nan(y);
#pragma unroll
    for (int m = 0; m < NPAD; ++m) {
      const bool live = m < Mt;  // wave-uniform
      bad = bad || (live && is_nan(x[m]));
      // NaN -> +inf (v_min returns the other operand; the point is invalid
      // and never summed), dead slots +inf: they sort behind every member
      x[m] = live ? vmin(x[m], inf) : inf;
    }
    if (M > 1) sort_network<NPAD, NPAD>(x);
    const unsigned long long ok_mask = __ballot(active && !bad);
    // bit j: column j opens another class than column j - 1 (bit 0: than the
    // running sums)
    const int c_first = __builtin_amdgcn_readlane(cls_v, 0);
    const int cls_left = __shfl_up(cls_v, 1);
    const unsigned long long change =
        __ballot(lane > 0 && cls_v != cls_left) | (c_first != cur ? 1ull : 0ull);
    // the DS operations of one wave execute in order; the fences restrain the
    // compiler
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int m = 0; m < NPAD; ++m)
      if (m < Mt) tile[m * kCrpsPitch + lane] = x[m];
    tile[M * kCrpsPitch + lane] = y;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int n_here = p.n_col - col0 < kWave ? p.n_col - col0 : kWave;
    for (int j0 = 0; j0 < n_here; j0 += G) {
      const unsigned all = (1u << G) - 1;
      if (j0 + G <= n_here && ((unsigned)(change >> j0) & all) == 0 &&
          ((unsigned)(ok_mask >> j0) & all) == all) {
        // G valid points of the running class: the same additions in the same
        // order as below, their 3 G LDS reads requested together
        T ty[G], tl[G], th[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          ty[u] = t_y[j0 + u];
          tl[u] = t_lo[j0 + u];
          th[u] = t_hi[j0 + u];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          double a, b;
          crps_terms(lane, (double)ty[u], (double)tl[u], (double)th[u], a,
                        b);
          sum_a = sum_a + a;
          sum_b = sum_b + b;
          n_above += a > 0.0 ? 1 : 0;
          n_below += b > 0.0 ? 1 : 0;
        }
        n_valid += G;
        continue;
      }
      const int j1 = j0 + G < n_here ? j0 + G : n_here;
      for (int j = j0; j < j1; ++j) {
        const int c = __builtin_amdgcn_readlane(cls_v, j);
        if (c != cur) {
          if (cur >= 0)
            store_class(cur, sum_a, sum_b, n_below, n_above, n_valid);
          cur = c;
          sum_a = sum_b = 0.0;
          n_below = n_above = n_valid = 0;
          if ((seen >> c) & 1) {  // (each lane reads back what it stored)
            const double* d = srow + (long long)c * 2 * nb;
            if (mine) {
              sum_a = d[ia];
              sum_b = d[nb + lane];
            }
            if (lane == 0) {
              const int* n = crow + c * 3;
              n_below = n[0];
              n_above = n[1];
              n_valid = n[2];
            }
          }
          seen |= 1ull << c;
        }
        if ((ok_mask >> j) & 1) {
          double a, b;
          crps_terms(lane, (double)t_y[j], (double)t_lo[j], (double)t_hi[j],
                        a, b);
          sum_a = sum_a + a;
          sum_b = sum_b + b;
          n_above += a > 0.0 ? 1 : 0;
          n_below += b > 0.0 ? 1 : 0;
          n_valid += 1;
        }
      }
    }
  }
  if (cur >= 0) store_class(cur, sum_a, sum_b, n_below, n_above, n_valid);
  for (int c = 0; c < p.n_class; ++c)
    if (!((seen >> c) & 1)) store_class(c, 0.0, 0.0, 0, 0, 0);
}

struct CrpsFoldParams {
  const double* sums;  // [n_cell][n_row][n_class][n_slot]
  const double* wrow;  // [n_region][n_row]
  const int* mult;     // [n_region][n_class]
  double* table;       // [n_cell][n_region][n_slot]
  long long n_out;     // n_cell * n_region * n_slot
  int n_row, n_class, n_slot, n_region;
};

// One thread per output element, classes and rows in increasing order: the
// simple path (wb2_event_fold's shape with float64 inputs).
__global__ void __launch_bounds__(kCrpsFoldThreads)
    crps_bin_fold_kernel(const CrpsFoldParams p) {
  const long long idx = (long long)blockIdx.x * kCrpsFoldThreads + threadIdx.x;
  if (idx >= p.n_out) return;
  const int slot = (int)(idx % p.n_slot);
  const long long rest = idx / p.n_slot;
  const int r = (int)(rest % p.n_region);
  const long long cell = rest / p.n_region;
  const double* __restrict__ sums =
      p.sums + cell * p.n_row * p.n_class * p.n_slot + slot;
  const int* __restrict__ mult = p.mult + (long long)r * p.n_class;
  const double* __restrict__ wrow = p.wrow + (long long)r * p.n_row;
  double acc = 0.0;
  for (int i = 0; i < p.n_row; ++i) {
    double s = 0.0;
#pragma unroll 4
    for (int c = 0; c < p.n_class; ++c)
      s = s + (double)mult[c] *
                  sums[((long long)i * p.n_class + c) * p.n_slot];
    acc = acc + wrow[i] * s;
  }
  p.table[idx] = acc;
}

// bytes of the tile of one wave = one workgroup (the rows share nothing, and
// single-wave workgroups spread a few thousand rows evenly over the CUs)
inline long long crps_lds_bytes(int dtype, int n_member) {
  return (long long)(n_member + 1) * kCrpsPitch * (dtype == WB2_F32 ? 4 : 8);
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_crps_bins_geometry(int dtype, int32_t n_member, int32_t n_class,
                           int32_t* min_member, int32_t* max_member,
                           int32_t* tile_cols, int32_t* rows_per_group,
                           int64_t* lds_bytes, int32_t* max_grid_outer) {
  using namespace wb2;
  if (const int rc = class_shape(kCrpsTakes, dtype, n_member, n_class))
    return rc;
  WB2_REQUIRE(lds_bytes, "null pointer argument");
  *lds_bytes = crps_lds_bytes(dtype, n_member);
  return class_geometry(min_member, max_member, tile_cols, rows_per_group,
                        max_grid_outer);
}

int wb2_crps_bin_sums(int dtype, const void* ens, const int64_t* ens_slab,
                      const void* truth, const int64_t* truth_slab,
                      int32_t n_member, int64_t member_stride, int64_t n_outer,
                      int32_t n_row, int32_t n_col, const int32_t* col_class,
                      int32_t n_class, double* sums, int32_t* cnt,
                      void* stream) {
  WB2_TRACE();
  using namespace wb2;
  if (const int rc = class_shape(kCrpsTakes, dtype, n_member, n_class))
    return rc;
  CrpsParams p{};
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, &p);
  if (go <= 0) return go;
  if (const int rc = class_operands(col_class, sums, cnt, n_row, n_col,
                                    n_class, &p))
    return rc;
  dim3 grid, block;
  if (const int rc = class_grid(n_outer, n_row, &grid, &block)) return rc;
  const size_t lds = (size_t)crps_lds_bytes(dtype, n_member);
  for_npad(dtype, n_member, [&](auto T0, auto N) {
    hipLaunchKernelGGL((crps_bin_sums_kernel<decltype(T0), decltype(N)::value>),
                       grid, block, lds, static_cast<hipStream_t>(stream), p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_crps_bin_fold(const double* sums, int64_t n_cell, int32_t n_row,
                      int32_t n_class, int32_t n_slot, const double* wrow,
                      const int32_t* mult, int32_t n_region, double* table,
                      void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(n_row >= 0 && n_class >= 1 && n_slot >= 1,
              "bad sizes: %d rows, %d classes, %d slots", (int)n_row,
              (int)n_class, (int)n_slot);
  WB2_EMPTY_OK(n_cell);
  WB2_EMPTY_OK(n_region);
  WB2_REQUIRE(table && (n_row == 0 || (sums && wrow && mult)),
              "null pointer argument");
  CrpsFoldParams p{};
  p.sums = sums;
  p.wrow = wrow;
  p.mult = mult;
  p.table = table;
  p.n_out = (long long)n_cell * n_region * n_slot;
  p.n_row = n_row;
  p.n_class = n_class;
  p.n_slot = n_slot;
  p.n_region = n_region;
  const long long blocks = (p.n_out + kCrpsFoldThreads - 1) / kCrpsFoldThreads;
  WB2_REQUIRE(blocks < (1ll << 31), "the grid does not fit: %lld elements",
              p.n_out);
  hipLaunchKernelGGL(crps_bin_fold_kernel, dim3((unsigned)blocks),
                     dim3(kCrpsFoldThreads), 0, static_cast<hipStream_t>(stream),
                     p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
