// K21 of libwb2hip.so: the sums of the threshold-weighted CRPS (twCRPS;
// Gneiting & Ranjan 2011, the chaining-function form of Allen, Ginsbourger &
// Ziegel 2023) with the tail weights 1[z >= t] (upper) and 1[z <= t] (lower).
// The reference has the CRPS itself (metrics.py:760-830) and no counterpart.
//
//   wb2_twcrps_sums  sums[t][o][i][c][0] = the sum of A, sums[..][1] = the sum
//                    of B over the points of the columns of class c in row i
//                    of outer index o that are valid for threshold t
//                    (float64); cnt[t][o][i][c] = the number of those points
//
// One point, members sorted x_1 <= ... <= x_M, truth y, threshold t, all in
// float64 after an exact widening, v(z) = z < t ? t : z (upper) or z > t ? t :
// z (lower):
//   A = sum_{i=1..M} |v(x_i) - v(y)|                      in sorted order
//   B = sum_{k=1..M-1} (double)(k (M - k)) * (v(x_{k+1}) - v(x_k))   in k
// both sequential from +0.0, the product rounded before it is added.  v is
// monotone, so ONE sort serves every threshold.  The point is invalid for
// threshold t iff the truth, any member or that threshold's value is NaN.
//
// One WAVE (a workgroup of its own) owns one row of one outer index and walks
// it in tiles of 64 columns, in column order.  Per tile a lane requests its
// point's truth, thresholds and members, all before any is looked at (each row
// is read once: (M + 1 + T) elements per point), and sorts the members in
// registers with the networks of ensemble_kernels.hpp (+inf padding up to the
// next power of two).  Every threshold of the launch is then one pass over the
// sorted registers, and the lane stores its A and B -- +0.0 where the point is
// invalid for the threshold or lies past the row end -- in a wave-private LDS
// tile [2 T][64 + 1] of float64 (the odd pitch: the transposed reads below hit
// distinct banks).  Then the roles turn: lane s (s < 2 T) owns slot s =
// (threshold s / 2, term s % 2) and walks the 64 points of the tile in column
// order, eight LDS reads at a time, adding each to its running float64 sum.
// Every summand is >= +0.0 and the chain starts from +0.0, so adding the +0.0
// of an invalid point leaves every bit of the sum as it was: the sum is the
// chain over the valid points.  The running sum belongs to the class of the
// current column; where the class changes (a wave-uniform test) the lane
// stores it and takes up the sum of the new class (0 where the row has not
// met it): the sum of a (threshold, row, class, term) is ONE sequential chain
// over its columns in increasing order, whatever the tiles are.  The valid
// counts come from the ballots of the per-threshold validity.  Plain stores,
// no atomics of any kind.
//
// The requests of a tile, the mask of class changes and the host side are
// class_sums.hpp's, shared with K24 (the host side with K20 too); the threshold
// batches are event_common.hpp's, shared with K18 and K19.

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

constexpr int kTwPitch = kWave + 1;
constexpr char kTwTakes[] = "the twCRPS sums take";

struct TwParams : ExceedOperands {
  const int* col_class;  // [n_col]
  double* sums;          // the first threshold of this launch
  int* cnt;              // likewise
  long long thr_cells;   // n_outer * n_row * n_class: cells of one threshold
  int n_row, n_col, n_class;
  int nt;                // thresholds of this launch, 1 .. kExceedThr
  int lower;             // the tail: v = min(z, t) instead of max(z, t)
};

template <typename T, int NPAD>
__global__ void __launch_bounds__(kWave)
    twcrps_sums_kernel(const TwParams p) {
  extern __shared__ double tw_tile[];  // [2 nt][kTwPitch]
  constexpr int G = 8;  // points whose LDS reads are in flight together
  const int lane = threadIdx.x;
  const long long o = outer_index();
  const int row = (int)blockIdx.x;
  if (o >= p.n_outer) return;
  const int M = p.n_member;
  const int nt = p.nt;
  const bool lower = p.lower != 0;
  const T inf = std::numeric_limits<T>::infinity();

  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);
  const T* hb[kExceedThr];
#pragma unroll
  for (int q = 0; q < kExceedThr; ++q)
    hb[q] = q < nt ? exceed_slab<T>(p.thr[q], p.thr_slab[q], o, slab, first)
                   : tb;  // (never read)

  // the slot of this lane: threshold lane / 2, term lane % 2
  const bool mine = lane < 2 * nt;
  const int my_q = mine ? lane >> 1 : 0;  // (a lane without a slot stores none)
  const bool counts = mine && (lane & 1) == 0;  // the A lane keeps the count
  const long long cell = (o * p.n_row + row) * (long long)p.n_class;
  double* dsum = p.sums + (my_q * p.thr_cells + cell) * 2 + (lane & 1);
  int* dcnt = p.cnt + my_q * p.thr_cells + cell;
  const double* t_mine = tw_tile + (mine ? lane : 0) * kTwPitch;
  double sum = 0.0;
  int n_valid = 0;
  int cur = -1;                 // the class of the running sum
  unsigned long long seen = 0;  // classes this row has met

  auto store_class = [&](int c, double s, int n) {
    if (mine) dsum[(long long)c * 2] = s;
    if (counts) dcnt[c] = n;
  };

  const int n_tile = (p.n_col + kWave - 1) / kWave;
  for (int tcol = 0; tcol < n_tile; ++tcol) {
    const int col0 = tcol * kWave;
    const bool active = col0 + lane < p.n_col;
    // a lane past the end of the row reads its last column again
    const int colc = active ? col0 + lane : p.n_col - 1;
    int cls_v, Mt;
    T y, x[NPAD], hv[kExceedThr];
    class_tile<T, NPAD>(xb, tb, p.col_class, p.member_stride, M, colc, cls_v, y,
                        Mt, x, [&] {
#pragma unroll
      for (int q = 0; q < kExceedThr; ++q) hv[q] = q < nt ? hb[q][colc] : T(0);
    });
    bool bad = is_nan(y);
#pragma unroll
    for (int m = 0; m < NPAD; ++m) {
      const bool live = m < Mt;  // wave-uniform
      bad = bad || (live && is_nan(x[m]));
      // NaN -> +inf (v_min returns the other operand; the point is invalid
      // and adds +0.0), dead slots +inf: they sort behind every member
      x[m] = live ? vmin(x[m], inf) : inf;
    }
    if (M > 1) sort_network<NPAD, NPAD>(x);
    const unsigned long long change = class_change(cls_v, cur, lane);

    // the DS operations of one wave execute in order; the fences restrain the
    // compiler
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    unsigned long long my_ok = 0;  // the validity ballot of this lane's slot
#pragma unroll
    for (int q = 0; q < kExceedThr; ++q) {
      if (q < nt) {  // wave-uniform
        const double t = (double)hv[q];
        auto clampv = [&](double z) {
          return lower ? (z > t ? t : z) : (z < t ? t : z);
        };
        const double vy = clampv((double)y);
        double a = 0.0, b = 0.0, prev = 0.0;
#pragma unroll
        for (int m = 0; m < NPAD; ++m) {
          if (m < Mt) {  // wave-uniform
            const double v = clampv((double)x[m]);
            a = a + __builtin_fabs(v - vy);
            if (m > 0) b = b + (double)(m * (Mt - m)) * (v - prev);
            prev = v;
          }
        }
        const bool ok = active && !bad && !is_nan(hv[q]);
        tw_tile[(2 * q) * kTwPitch + lane] = ok ? a : 0.0;
        tw_tile[(2 * q + 1) * kTwPitch + lane] = ok ? b : 0.0;
        const unsigned long long okm = __ballot(ok);
        if (my_q == q) my_ok = okm;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int n_here = p.n_col - col0 < kWave ? p.n_col - col0 : kWave;
    for (int j0 = 0; j0 < n_here; j0 += G) {
      const unsigned all = (1u << G) - 1;
      if (j0 + G <= n_here && ((unsigned)(change >> j0) & all) == 0) {
        // G points of the running class: the same additions in the same order
        // as below, their LDS reads requested together
        double v[G];
#pragma unroll
        for (int u = 0; u < G; ++u) v[u] = t_mine[j0 + u];
#pragma unroll
        for (int u = 0; u < G; ++u) sum = sum + v[u];
        n_valid += __popc((unsigned)(my_ok >> j0) & all);
        continue;
      }
      const int j1 = j0 + G < n_here ? j0 + G : n_here;
      for (int j = j0; j < j1; ++j) {
        const int c = __builtin_amdgcn_readlane(cls_v, j);
        if (c != cur) {
          if (cur >= 0) store_class(cur, sum, n_valid);
          cur = c;
          sum = 0.0;
          n_valid = 0;
          if ((seen >> c) & 1) {  // (each lane reads back what it stored)
            if (mine) sum = dsum[(long long)c * 2];
            if (counts) n_valid = dcnt[c];
          }
          seen |= 1ull << c;
        }
        sum = sum + t_mine[j];
        n_valid += (int)((my_ok >> j) & 1);
      }
    }
    // (the next tile overwrites the LDS tile: its reads above are done)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  if (cur >= 0) store_class(cur, sum, n_valid);
  for (int c = 0; c < p.n_class; ++c)
    if (!((seen >> c) & 1)) store_class(c, 0.0, 0);
}

inline long long tw_lds_bytes(int nt) {
  return (long long)2 * nt * kTwPitch * (long long)sizeof(double);
}

inline int tw_shape(int dtype, int n_member, int n_class, int n_threshold) {
  if (const int rc = class_shape(kTwTakes, dtype, n_member, n_class)) return rc;
  WB2_REQUIRE(n_threshold >= 1, "n_threshold=%d", n_threshold);
  return 0;
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_twcrps_geometry(int dtype, int32_t n_member, int32_t n_class,
                        int32_t n_threshold, int32_t* min_member,
                        int32_t* max_member, int32_t* thresholds_per_launch,
                        int32_t* tile_cols, int32_t* rows_per_group,
                        int64_t* lds_bytes, int32_t* max_grid_outer) {
  using namespace wb2;
  if (const int rc = tw_shape(dtype, n_member, n_class, n_threshold)) return rc;
  WB2_REQUIRE(thresholds_per_launch && lds_bytes, "null pointer argument");
  *thresholds_per_launch = n_threshold < kExceedThr ? n_threshold : kExceedThr;
  *lds_bytes = tw_lds_bytes(*thresholds_per_launch);
  return class_geometry(min_member, max_member, tile_cols, rows_per_group,
                        max_grid_outer);
}

int wb2_twcrps_sums(int dtype, const void* ens, const int64_t* ens_slab,
                    const void* truth, const int64_t* truth_slab,
                    const void* const* threshold, const int64_t* thr_slab,
                    int32_t n_threshold, int32_t n_member,
                    int64_t member_stride, int64_t n_outer, int32_t n_row,
                    int32_t n_col, const int32_t* col_class, int32_t n_class,
                    int lower, double* sums, int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  if (const int rc = tw_shape(dtype, n_member, n_class, n_threshold)) return rc;
  TwParams p{};
  const int go = exceed_operands(ens, ens_slab, truth, truth_slab, threshold,
                                 n_threshold, n_member, member_stride, n_outer,
                                 n_row, n_col, &p);
  if (go <= 0) return go;
  if (const int rc = class_operands(col_class, sums, cnt, n_row, n_col,
                                    n_class, &p))
    return rc;
  p.thr_cells = (long long)n_outer * n_row * n_class;
  p.lower = lower != 0;
  dim3 grid, block;
  if (const int rc = class_grid(n_outer, n_row, &grid, &block)) return rc;
  return exceed_batches(
      &p, threshold, thr_slab, n_threshold, kExceedThr, [&](int t0, int nt) {
        p.sums = sums + t0 * p.thr_cells * 2;
        p.cnt = cnt + t0 * p.thr_cells;
        p.nt = nt;
        for_npad(dtype, n_member, [&](auto T0, auto N) {
          hipLaunchKernelGGL(
              (twcrps_sums_kernel<decltype(T0), decltype(N)::value>), grid,
              block, (size_t)tw_lds_bytes(nt),
              static_cast<hipStream_t>(stream), p);
        });
      });
}

}  // extern "C"
