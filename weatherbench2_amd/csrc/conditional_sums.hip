// K24 of libwb2hip.so: the per-bin sums of conditional verification -- the
// spread-error diagnostic (Leutbecher & Palmer 2008) and the conditional bias
// (Murphy & Winkler 1987): ensemble mean, truth, ensemble variance and squared
// error of the mean, binned by the variance, the mean or the truth.  The
// reference has the region means (EnsembleVariance, EnsembleMeanMSE, Bias) and
// no stratified counterpart.
//
//   wb2_conditional_sums  sums[o][i][c][b][0..3] = the sums of mu, y, s2, se
//                         over the valid points of bin b among the columns of
//                         class c in row i of outer index o (float64);
//                         cnt[o][i][c][b] = the number of those points
//
// One point, members x_0 .. x_{M-1} in STORAGE order, truth y, all in float64
// after an exact widening, no fused multiply-add:
//   S = x_0; S = S + x_m;  mu = S / (double)M
//   d_m = x_m - mu;  Q = d_0 d_0;  Q = Q + d_m d_m;  s2 = Q / (double)(M - 1)
//   (M = 1: s2 = +0.0);  e = mu - y;  se = e e
//   v = s2 (mode 0), mu (mode 1), y (mode 2);  bin = #{k : edge_k <= v}
// The point is invalid iff the truth or any member is NaN (K18's rule).
//
// One WAVE (a workgroup of its own) owns one row of one outer index and walks
// it in tiles of 64 columns, in column order.  Per tile a lane requests its
// point's truth and members, all before any is looked at (each row is read
// once: (M + 1) elements per point), forms the four values and the bin in its
// own registers -- the edges live one per lane in a register and are handed
// round by v_readlane -- and stores them in a wave-private LDS tile: [4][64]
// float64 and [64] int32 (the bin; -1 where the point is invalid or lies past
// the row end).  Then the roles turn: lane b (b < B) owns bin b and walks the
// 64 points of the tile in column order, eight at a time; every lane reads the
// bin and the four values of a point (five LDS reads, all broadcasts) and adds
// to each of its four running float64 sums the value if the bin is its own and
// +0.0 otherwise.  A chain started at +0.0 never holds -0.0, so that +0.0
// leaves every bit of the sum as it was: the sum is the chain over the bin's
// own points.  The running sums belong to the class of the current column;
// where the class changes (a wave-uniform test) the lane stores them and takes
// up the sums of the new class (0 where the row has not met it): the sum of a
// (row, class, bin, term) is ONE sequential chain over its columns in
// increasing order, whatever the tiles are.  Plain stores, no atomics of any
// kind.
//
// The requests of a tile, the mask of class changes and the host side are
// class_sums.hpp's, shared with K21 (the host side with K20 too).

#include <cstdint>

#include "class_sums.hpp"
#include "common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kCondMaxEdge = kWave - 1;  // lane b owns bin b: one wave of bins
constexpr int kCondTerm = 4;        // mu, y, s2, se
constexpr char kCondTakes[] = "the conditional sums take";

struct CondParams {
  const void* ens;
  const void* truth;
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const int* col_class;         // [n_col]
  const double* edges;          // [n_edge], increasing (mode 0: squared)
  double* sums;                 // [n_outer][n_row][n_class][B][4]
  int* cnt;                     // [n_outer][n_row][n_class][B]
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class, n_edge, mode;
};

// the double of lane `k` (wave-uniform k)
__device__ __forceinline__ double lane_f64(double v, int k) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, k);
  const unsigned hi =
      (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

template <typename T, int NPAD>
__global__ void __launch_bounds__(kWave)
    conditional_sums_kernel(const CondParams p) {
  __shared__ double cond_val[kCondTerm][kWave];
  __shared__ int cond_bin[kWave];
  constexpr int G = 8;  // points whose LDS reads are in flight together
  const int lane = threadIdx.x;
  const long long o = outer_index();
  const int row = (int)blockIdx.x;
  if (o >= p.n_outer) return;
  const int M = p.n_member;
  const int n_edge = p.n_edge;
  const int nb = n_edge + 1;
  const int mode = p.mode;

  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);

  // lane k holds edge k (a lane without one is never asked)
  const double my_edge = lane < n_edge ? p.edges[lane] : 0.0;

  // the bin of this lane
  const bool mine = lane < nb;
  const long long cell = (o * p.n_row + row) * (long long)p.n_class;
  double* dsum = p.sums + (cell * nb + (mine ? lane : 0)) * kCondTerm;
  int* dcnt = p.cnt + cell * nb + (mine ? lane : 0);
  double sum[kCondTerm] = {0.0, 0.0, 0.0, 0.0};
  int n_in = 0;
  int cur = -1;                 // the class of the running sums
  unsigned long long seen = 0;  // classes this row has met

  auto store_class = [&](int c, const double (&s)[kCondTerm], int n) {
    if (mine) {
      double* d = dsum + (long long)c * nb * kCondTerm;
#pragma unroll
      for (int k = 0; k < kCondTerm; ++k) d[k] = s[k];
      dcnt[(long long)c * nb] = n;
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
    // (a NaN member makes S, and with it every value, NaN: the point is then
    // stored with bin -1 and no lane adds it)
    bool bad = is_nan(y);
    double S = (double)x[0];
    bad = bad || is_nan(x[0]);
#pragma unroll
    for (int m = 1; m < NPAD; ++m)
      if (m < Mt) {  // wave-uniform
        bad = bad || is_nan(x[m]);
        S = S + (double)x[m];
      }
    const double mu = S / (double)Mt;
    const double d0 = (double)x[0] - mu;
    double Q = d0 * d0;
#pragma unroll
    for (int m = 1; m < NPAD; ++m)
      if (m < Mt) {
        const double d = (double)x[m] - mu;
        Q = Q + d * d;
      }
    const double s2 = Mt > 1 ? Q / (double)(Mt - 1) : 0.0;
    const double yd = (double)y;
    const double e = mu - yd;
    const double se = e * e;
    const double v = mode == 0 ? s2 : (mode == 1 ? mu : yd);
    int bin = 0;
    for (int k = 0; k < n_edge; ++k) bin += lane_f64(my_edge, k) <= v ? 1 : 0;
    if (!active || bad) bin = -1;

    const unsigned long long change = class_change(cls_v, cur, lane);

    // the DS operations of one wave execute in order; the fences restrain the
    // compiler
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    cond_val[0][lane] = mu;
    cond_val[1][lane] = yd;
    cond_val[2][lane] = s2;
    cond_val[3][lane] = se;
    cond_bin[lane] = bin;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int n_here = p.n_col - col0 < kWave ? p.n_col - col0 : kWave;
    for (int j0 = 0; j0 < n_here; j0 += G) {
      const unsigned all = (1u << G) - 1;
      if (j0 + G <= n_here && ((unsigned)(change >> j0) & all) == 0) {
        // G points of the running class: the same additions in the same order
        // as below, their LDS reads requested together
        double w[G][kCondTerm];
        int b[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          b[u] = cond_bin[j0 + u];
#pragma unroll
          for (int k = 0; k < kCondTerm; ++k) w[u][k] = cond_val[k][j0 + u];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const bool in = b[u] == lane;
#pragma unroll
          for (int k = 0; k < kCondTerm; ++k)
            sum[k] = sum[k] + (in ? w[u][k] : 0.0);
          n_in += in ? 1 : 0;
        }
        continue;
      }
      const int j1 = j0 + G < n_here ? j0 + G : n_here;
      for (int j = j0; j < j1; ++j) {
        const int c = __builtin_amdgcn_readlane(cls_v, j);
        if (c != cur) {
          if (cur >= 0) store_class(cur, sum, n_in);
          cur = c;
#pragma unroll
          for (int k = 0; k < kCondTerm; ++k) sum[k] = 0.0;
          n_in = 0;
          if (((seen >> c) & 1) && mine) {  // (a lane reads back its own stores)
            const double* d = dsum + (long long)c * nb * kCondTerm;
#pragma unroll
            for (int k = 0; k < kCondTerm; ++k) sum[k] = d[k];
            n_in = dcnt[(long long)c * nb];
          }
          seen |= 1ull << c;
        }
        const bool in = cond_bin[j] == lane;
#pragma unroll
        for (int k = 0; k < kCondTerm; ++k)
          sum[k] = sum[k] + (in ? cond_val[k][j] : 0.0);
        n_in += in ? 1 : 0;
      }
    }
    // (the next tile overwrites the LDS tile: its reads above are done)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  if (cur >= 0) store_class(cur, sum, n_in);
  const double zero[kCondTerm] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < p.n_class; ++c)
    if (!((seen >> c) & 1)) store_class(c, zero, 0);
}

inline long long cond_lds_bytes() {
  return (long long)kCondTerm * kWave * (long long)sizeof(double) +
         (long long)kWave * (long long)sizeof(int);
}

inline int cond_shape(int dtype, int n_member, int n_class, int n_edge) {
  if (const int rc = class_shape(kCondTakes, dtype, n_member, n_class))
    return rc;
  WB2_REQUIRE(n_edge >= 0 && n_edge <= kCondMaxEdge,
              "n_edge=%d: %s 0 to %d bin edges", n_edge, kCondTakes,
              kCondMaxEdge);
  return 0;
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_conditional_geometry(int dtype, int32_t n_member, int32_t n_class,
                             int32_t n_edge, int32_t* min_member,
                             int32_t* max_member, int32_t* max_edges,
                             int32_t* tile_cols, int32_t* rows_per_group,
                             int64_t* lds_bytes, int32_t* max_grid_outer) {
  using namespace wb2;
  if (const int rc = cond_shape(dtype, n_member, n_class, n_edge)) return rc;
  WB2_REQUIRE(max_edges && lds_bytes, "null pointer argument");
  *max_edges = kCondMaxEdge;
  *lds_bytes = cond_lds_bytes();
  return class_geometry(min_member, max_member, tile_cols, rows_per_group,
                        max_grid_outer);
}

int wb2_conditional_sums(int dtype, const void* ens, const int64_t* ens_slab,
                         const void* truth, const int64_t* truth_slab,
                         int32_t n_member, int64_t member_stride,
                         int64_t n_outer, int32_t n_row, int32_t n_col,
                         const int32_t* col_class, int32_t n_class, int mode,
                         const double* edges, int32_t n_edge, double* sums,
                         int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  if (const int rc = cond_shape(dtype, n_member, n_class, n_edge)) return rc;
  WB2_REQUIRE(mode >= 0 && mode <= 2, "mode=%d: %s 0 (spread), 1 (forecast) "
              "or 2 (truth)", mode, kCondTakes);
  CondParams p{};
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, &p);
  if (go <= 0) return go;
  WB2_REQUIRE(edges || n_edge == 0, "null pointer argument");
  if (const int rc = class_operands(col_class, sums, cnt, n_row, n_col,
                                    n_class, &p))
    return rc;
  p.edges = edges;
  p.n_edge = n_edge;
  p.mode = mode;
  dim3 grid, block;
  if (const int rc = class_grid(n_outer, n_row, &grid, &block)) return rc;
  for_npad(dtype, n_member, [&](auto T0, auto N) {
    hipLaunchKernelGGL(
        (conditional_sums_kernel<decltype(T0), decltype(N)::value>), grid,
        block, 0, static_cast<hipStream_t>(stream), p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
