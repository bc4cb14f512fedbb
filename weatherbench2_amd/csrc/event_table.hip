// K18 of libwb2hip.so: joint exceedance tables for threshold-event
// verification (reliability diagram, ROC, Brier decomposition, contingency
// table).  The reference reduces the event `x > threshold` to one score per
// threshold (metrics.py:1524-1891); it has no counterpart of the table.
//
//   wb2_event_counts  cnt[t][o][i][c][code] = number of columns j of class c
//                     in row i of outer index o whose point has `code` under
//                     threshold t
//   wb2_event_fold    table[t][o][r][code] = sum_i wrow[r][i] *
//                     (double)(sum_c mult[r][c] * cnt[t][o][i][c][code])
//
// For one point (k, obs, invalid: event_common.hpp): code = obs * (M + 1) + k,
// the invalid code is 2 (M + 1), n_code = 2 (M + 1) + 1.  The region weights
// factor into a row
// weight and an integer column multiplicity that is constant on a column
// class, so the counting kernel adds integers only (LDS atomics: integer adds
// commute, two runs are bit-equal) and the float work is the ordered fold.
// No global atomics, no float atomics.
//
// Counting: a workgroup of 256 threads owns rows_per_group adjacent rows of one
// outer index -- one contiguous run of every slab -- and walks it with 16-byte
// lanes (or one element per access).  A thread takes its points through
// exceed_points(), forms the codes and adds 1 to the LDS histogram
// [threshold][row][class][code]; after a barrier the histogram goes
// to memory with plain stores.  Members and truth are read ONCE for the
// thresholds of a launch: (M + 1 + T) elements per point.

#include <cstdint>

#include "common.hpp"
#include "event_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kEventThreads = 256;
constexpr int kEventRows = 4;    // rows of one workgroup, at most
constexpr long long kEventLds = 64 * 1024;  // bytes of histogram per workgroup
constexpr char kEventTakes[] = "the event table takes";

struct EventParams : ExceedOperands {
  const int* col_class;         // [n_col]
  int* cnt;                     // the first threshold of this launch
  long long cnt_thr_stride;     // counts of one threshold
  int n_row, n_col, n_class, rows_per_group;
};

template <typename T, int VEC, int NT>
__global__ void __launch_bounds__(kEventThreads)
    event_counts_kernel(const EventParams p) {
  extern __shared__ int hist[];  // [NT][rows_per_group][n_class][n_code]
  const long long o = outer_index();
  if (o >= p.n_outer) return;  // (the whole workgroup)
  const int M = p.n_member;
  const int n_code = 2 * (M + 1) + 1;
  const int row0 = (int)blockIdx.x * p.rows_per_group;
  const int nrow = p.n_row - row0 < p.rows_per_group ? p.n_row - row0
                                                     : p.rows_per_group;
  const int row_bins = p.n_class * n_code;
  const int thr_bins = p.rows_per_group * row_bins;
  for (int i = threadIdx.x; i < NT * thr_bins; i += kEventThreads) hist[i] = 0;
  __syncthreads();

  // (once per workgroup: the element loop below loads no table)
  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row0 * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);
  const T* hb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    hb[t] = exceed_slab<T>(p.thr[t], p.thr_slab[t], o, slab, first);
  const int n_elem = nrow * p.n_col;  // (the host checked that it fits)
  for (int e = (int)threadIdx.x * VEC; e < n_elem; e += kEventThreads * VEC) {
    T tv[VEC], hv[NT][VEC];
    load_v<T, VEC>(tb + e, tv);
#pragma unroll
    for (int t = 0; t < NT; ++t) load_v<T, VEC>(hb[t] + e, hv[t]);
    int k[NT][VEC];
    bool obs[NT][VEC], bad[VEC];
    exceed_points<T, VEC, NT>(xb + e, p.member_stride, M, tv, hv, k, obs, bad);
    // (VEC divides n_col on the wide path: a lane never spans two rows)
    const int r = e / p.n_col;
    const int c = e - r * p.n_col;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int bin = r * row_bins + p.col_class[c + v] * n_code;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int code = bad[v] ? 2 * (M + 1)
                                : (obs[t][v] ? M + 1 : 0) + k[t][v];
        __hip_atomic_fetch_add(&hist[t * thr_bins + bin + code], 1,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  __syncthreads();
  const int n_out = nrow * row_bins;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int* dst = p.cnt + t * p.cnt_thr_stride +
               (o * p.n_row + row0) * (long long)row_bins;
    for (int i = threadIdx.x; i < n_out; i += kEventThreads)
      dst[i] = hist[t * thr_bins + i];
  }
}

struct EventFoldParams {
  const int* cnt;      // [n_cell][n_row][n_class][n_code]
  const double* wrow;  // [n_region][n_row]
  const int* mult;     // [n_region][n_class]
  double* table;       // [n_cell][n_region][n_code]
  long long n_out;     // n_cell * n_region * n_code
  int n_row, n_class, n_code, n_region;
};

// One thread per output element, rows in increasing order: the simple path.
__global__ void __launch_bounds__(kEventThreads)
    event_fold_kernel(const EventFoldParams p) {
  const long long idx = (long long)blockIdx.x * kEventThreads + threadIdx.x;
  if (idx >= p.n_out) return;
  const int code = (int)(idx % p.n_code);
  const long long rest = idx / p.n_code;
  const int r = (int)(rest % p.n_region);
  const long long cell = rest / p.n_region;
  const int* __restrict__ cnt =
      p.cnt + cell * p.n_row * p.n_class * p.n_code + code;
  const int* __restrict__ mult = p.mult + (long long)r * p.n_class;
  const double* __restrict__ wrow = p.wrow + (long long)r * p.n_row;
  double acc = 0.0;
  // eight rows (and four classes of each) at a time, so that their loads are
  // in flight together; the float sum keeps its order
  constexpr int kRows = 8;
  int i = 0;
  for (; i + kRows <= p.n_row; i += kRows) {
    long long s[kRows] = {};
#pragma unroll 4
    for (int c = 0; c < p.n_class; ++c) {
      const long long m = mult[c];
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        s[u] += m * cnt[((long long)(i + u) * p.n_class + c) * p.n_code];
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) acc += wrow[i + u] * (double)s[u];
  }
  for (; i < p.n_row; ++i) {
    long long s = 0;
    for (int c = 0; c < p.n_class; ++c)
      s += (long long)mult[c] *
           cnt[((long long)i * p.n_class + c) * p.n_code];
    acc += wrow[i] * (double)s;
  }
  p.table[idx] = acc;
}

struct EventGeometry {
  int rows_per_group, thresholds_per_launch;
  long long lds_bytes;
};

// The most thresholds per launch that fit the budget first (they share the
// read of the members), then the most rows.  False: not even one row of one
// threshold fits.
inline bool event_geometry(int n_member, int n_class, int n_threshold,
                           EventGeometry* g) {
  const long long row_bytes = 4ll * n_class * (2 * (n_member + 1) + 1);
  const int nt_max = n_threshold < kExceedThr ? n_threshold : kExceedThr;
  for (int nt = nt_max; nt >= 1; --nt)
    for (int rows = kEventRows; rows >= 1; rows /= 2)
      if (nt * rows * row_bytes <= kEventLds) {
        *g = {rows, nt, nt * rows * row_bytes};
        return true;
      }
  return false;
}

// exceed_shape() and the column classes: the checks of the geometry query.
inline int event_shape(int dtype, int n_member, int n_class, int n_threshold) {
  if (const int rc = exceed_shape(kEventTakes, dtype, n_member, n_threshold))
    return rc;
  WB2_REQUIRE(n_class >= 1 && n_class <= kExceedMaxClass,
              "n_class=%d: %s 1 to %d column classes", n_class, kEventTakes,
              kExceedMaxClass);
  return 0;
}

#define WB2_REQUIRE_EVENT_LDS(n_member, n_class, n_threshold, g)               \
  WB2_REQUIRE(event_geometry(n_member, n_class, n_threshold, &g),              \
              "the histogram of %d classes x %d codes does not fit the LDS "   \
              "budget of %lld bytes", (int)n_class, 2 * ((int)n_member + 1) + 1, \
              kEventLds)

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_event_counts_geometry(int dtype, int32_t n_member, int32_t n_class,
                              int32_t n_threshold, int wide,
                              int32_t* rows_per_group,
                              int32_t* thresholds_per_launch,
                              int64_t* lds_bytes, int32_t* max_grid_outer) {
  using namespace wb2;
  (void)wide;  // the lane width changes neither the rows nor the histogram
  if (const int rc = event_shape(dtype, n_member, n_class, n_threshold))
    return rc;
  WB2_REQUIRE(rows_per_group && thresholds_per_launch && lds_bytes &&
              max_grid_outer, "null pointer argument");
  EventGeometry g;
  WB2_REQUIRE_EVENT_LDS(n_member, n_class, n_threshold, g);
  *rows_per_group = g.rows_per_group;
  *thresholds_per_launch = g.thresholds_per_launch;
  *lds_bytes = g.lds_bytes;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_event_counts(int dtype, const void* ens, const int64_t* ens_slab,
                     const void* truth, const int64_t* truth_slab,
                     const void* const* threshold, const int64_t* thr_slab,
                     int32_t n_threshold, int32_t n_member,
                     int64_t member_stride, int64_t n_outer, int32_t n_row,
                     int32_t n_col, const int32_t* col_class, int32_t n_class,
                     int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  if (const int rc = event_shape(dtype, n_member, n_class, n_threshold))
    return rc;
  EventGeometry g;
  WB2_REQUIRE_EVENT_LDS(n_member, n_class, n_threshold, g);
  EventParams p{};
  const int go = exceed_operands(ens, ens_slab, truth, truth_slab, threshold,
                                 n_threshold, n_member, member_stride, n_outer,
                                 n_row, n_col, &p);
  if (go <= 0) return go;
  WB2_REQUIRE(col_class && cnt, "null pointer argument");
  // (the walk over a row group counts in int, one stride past its end)
  WB2_REQUIRE((long long)g.rows_per_group * n_col < (1ll << 30),
              "n_col=%d: a group of %d rows is too long", (int)n_col,
              g.rows_per_group);
  const bool wide = exceed_wide(dtype, ens, truth, threshold, n_threshold,
                                n_col, member_stride);
  const int n_code = 2 * (n_member + 1) + 1;
  p.col_class = col_class;
  p.cnt_thr_stride = (long long)n_outer * n_row * n_class * n_code;
  p.n_row = n_row;
  p.n_col = n_col;
  p.n_class = n_class;
  p.rows_per_group = g.rows_per_group;
  const long long groups = (n_row + g.rows_per_group - 1) / g.rows_per_group;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_outer, groups, &grid),
              "the grid does not fit: %lld outer indices of %lld row groups",
              (long long)n_outer, groups);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return exceed_batches(
      &p, threshold, thr_slab, n_threshold, g.thresholds_per_launch,
      [&](int t0, int nt) {
        p.cnt = cnt + t0 * p.cnt_thr_stride;
        const size_t lds = (size_t)nt * g.rows_per_group * n_class * n_code * 4;
        for_exceed(dtype, wide, nt, [&](auto T0, auto V, auto NT) {
          hipLaunchKernelGGL(
              (event_counts_kernel<decltype(T0), decltype(V)::value,
                                   decltype(NT)::value>),
              grid, dim3(kEventThreads), lds, s, p);
        });
      });
}

int wb2_event_fold(const int32_t* cnt, int64_t n_cell, int32_t n_row,
                   int32_t n_class, int32_t n_code, const double* wrow,
                   const int32_t* mult, int32_t n_region, double* table,
                   void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(n_row >= 0 && n_class >= 1 && n_code >= 1,
              "bad sizes: %d rows, %d classes, %d codes", (int)n_row,
              (int)n_class, (int)n_code);
  WB2_EMPTY_OK(n_cell);
  WB2_EMPTY_OK(n_region);
  WB2_REQUIRE(table && (n_row == 0 || (cnt && wrow && mult)),
              "null pointer argument");
  EventFoldParams p{};
  p.cnt = cnt;
  p.wrow = wrow;
  p.mult = mult;
  p.table = table;
  p.n_out = (long long)n_cell * n_region * n_code;
  p.n_row = n_row;
  p.n_class = n_class;
  p.n_code = n_code;
  p.n_region = n_region;
  const long long blocks = (p.n_out + kEventThreads - 1) / kEventThreads;
  WB2_REQUIRE(blocks < (1ll << 31), "the grid does not fit: %lld elements",
              p.n_out);
  hipLaunchKernelGGL(event_fold_kernel, dim3((unsigned)blocks),
                     dim3(kEventThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
