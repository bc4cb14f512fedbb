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
// For one point: k = members with x > thr (IEEE: a NaN threshold exceeds
// nothing, equality is not exceedance), obs = truth > thr, invalid iff truth
// or any member is NaN.  code = obs * (M + 1) + k, the invalid code is
// 2 (M + 1), n_code = 2 (M + 1) + 1.  The region weights factor into a row
// weight and an integer column multiplicity that is constant on a column
// class, so the counting kernel adds integers only (LDS atomics: integer adds
// commute, two runs are bit-equal) and the float work is the ordered fold.
// No global atomics, no float atomics.
//
// Counting: a workgroup of 256 threads owns rows_per_group adjacent rows of one
// outer index -- one contiguous run of every slab -- and walks it with 16-byte
// lanes (or one element per access).  A thread loads the truth and up to 4
// thresholds of its points, then the M members kEventAhead at a time (all
// requested before any is compared), forms the codes and adds 1 to the LDS
// histogram [threshold][row][class][code]; after a barrier the histogram goes
// to memory with plain stores.  Members and truth are read ONCE for the
// thresholds of a launch: (M + 1 + T) elements per point.

#include <cstdint>

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kEventThreads = 256;
constexpr int kEventThr = 4;     // thresholds that share one read
constexpr int kEventRows = 4;    // rows of one workgroup, at most
constexpr int kEventAhead = 4;   // members requested before any is compared
constexpr long long kEventLds = 64 * 1024;  // bytes of histogram per workgroup
constexpr int kEventMaxMember = 128;
constexpr int kEventMaxClass = 64;

struct EventParams {
  const void* ens;
  const void* truth;
  const void* thr[kEventThr];
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const long long* thr_slab[kEventThr];  // each [n_outer] or null
  const int* col_class;         // [n_col]
  int* cnt;                     // the first threshold of this launch
  long long cnt_thr_stride;     // counts of one threshold
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class, rows_per_group;
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

  const long long slab_elems = (long long)p.n_row * p.n_col;
  const long long first = (long long)row0 * p.n_col;
  const T* xb = static_cast<const T*>(p.ens) +
                (p.ens_slab ? p.ens_slab[o] : o) * slab_elems + first;
  const T* tb = static_cast<const T*>(p.truth) +
                (p.truth_slab ? p.truth_slab[o] : o) * slab_elems + first;
  const T* hb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    hb[t] = static_cast<const T*>(p.thr[t]) +
            (p.thr_slab[t] ? p.thr_slab[t][o] : o) * slab_elems + first;

  const int n_elem = nrow * p.n_col;  // (the host checked that it fits)
  for (int e = (int)threadIdx.x * VEC; e < n_elem; e += kEventThreads * VEC) {
    T tv[VEC], hv[NT][VEC];
    load_v<T, VEC>(tb + e, tv);
#pragma unroll
    for (int t = 0; t < NT; ++t) load_v<T, VEC>(hb[t] + e, hv[t]);
    int k[NT][VEC];
    bool bad[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      bad[v] = is_nan(tv[v]);
#pragma unroll
      for (int t = 0; t < NT; ++t) k[t][v] = 0;
    }
    const T* xe = xb + e;
    int m = 0;
    for (; m + kEventAhead <= M; m += kEventAhead) {
      T x[kEventAhead][VEC];
#pragma unroll
      for (int u = 0; u < kEventAhead; ++u)
        load_v<T, VEC>(xe + (m + u) * p.member_stride, x[u]);
#pragma unroll
      for (int u = 0; u < kEventAhead; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          bad[v] = bad[v] || is_nan(x[u][v]);
#pragma unroll
          for (int t = 0; t < NT; ++t) k[t][v] += x[u][v] > hv[t][v] ? 1 : 0;
        }
    }
    for (; m < M; ++m) {
      T x[VEC];
      load_v<T, VEC>(xe + m * p.member_stride, x);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        bad[v] = bad[v] || is_nan(x[v]);
#pragma unroll
        for (int t = 0; t < NT; ++t) k[t][v] += x[v] > hv[t][v] ? 1 : 0;
      }
    }
    // (VEC divides n_col on the wide path: a lane never spans two rows)
    const int r = e / p.n_col;
    const int c = e - r * p.n_col;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int bin = r * row_bins + p.col_class[c + v] * n_code;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int code = bad[v] ? 2 * (M + 1)
                                : (tv[v] > hv[t][v] ? M + 1 : 0) + k[t][v];
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
  const int nt_max = n_threshold < kEventThr ? n_threshold : kEventThr;
  for (int nt = nt_max; nt >= 1; --nt)
    for (int rows = kEventRows; rows >= 1; rows /= 2)
      if (nt * rows * row_bytes <= kEventLds) {
        *g = {rows, nt, nt * rows * row_bytes};
        return true;
      }
  return false;
}

#define WB2_REQUIRE_EVENT_SHAPE(dtype, n_member, n_class, n_threshold)        \
  do {                                                                         \
    WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d",      \
                (int)dtype);                                                   \
    WB2_REQUIRE(n_member >= 1 && n_member <= kEventMaxMember,                  \
                "n_member=%d: the event table takes 1 to %d members",          \
                (int)n_member, kEventMaxMember);                               \
    WB2_REQUIRE(n_class >= 1 && n_class <= kEventMaxClass,                     \
                "n_class=%d: the event table takes 1 to %d column classes",    \
                (int)n_class, kEventMaxClass);                                 \
    WB2_REQUIRE(n_threshold >= 1, "n_threshold=%d", (int)n_threshold);         \
  } while (0)

#define WB2_REQUIRE_EVENT_LDS(n_member, n_class, n_threshold, g)               \
  WB2_REQUIRE(event_geometry(n_member, n_class, n_threshold, &g),              \
              "the histogram of %d classes x %d codes does not fit the LDS "   \
              "budget of %lld bytes", (int)n_class, 2 * ((int)n_member + 1) + 1, \
              kEventLds)

template <typename T, int VEC>
void launch_counts(int nt, dim3 grid, size_t lds, hipStream_t s,
                   const EventParams& p) {
#define WB2_L(NT)                                                        \
  hipLaunchKernelGGL((event_counts_kernel<T, VEC, NT>), grid,            \
                     dim3(kEventThreads), lds, s, p)
  switch (nt) {
    case 1: WB2_L(1); break;
    case 2: WB2_L(2); break;
    case 3: WB2_L(3); break;
    default: WB2_L(4); break;
  }
#undef WB2_L
}

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
  WB2_REQUIRE_EVENT_SHAPE(dtype, n_member, n_class, n_threshold);
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
  WB2_REQUIRE_EVENT_SHAPE(dtype, n_member, n_class, n_threshold);
  EventGeometry g;
  WB2_REQUIRE_EVENT_LDS(n_member, n_class, n_threshold, g);
  WB2_REQUIRE(member_stride >= 0, "member_stride=%lld is negative",
              (long long)member_stride);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_row);
  WB2_EMPTY_OK(n_col);
  WB2_REQUIRE(ens && truth && threshold && col_class && cnt,
              "null pointer argument");
  for (int t = 0; t < n_threshold; ++t)
    WB2_REQUIRE(threshold[t], "null pointer argument (threshold %d)", t);
  // (the walk over a row group counts in int, one stride past its end)
  WB2_REQUIRE((long long)g.rows_per_group * n_col < (1ll << 30),
              "n_col=%d: a group of %d rows is too long", (int)n_col,
              g.rows_per_group);
  const int w = wide_lanes(dtype);
  bool wide = all_aligned16(ens, truth) && n_col % w == 0 &&
              member_stride % w == 0;
  for (int t = 0; t < n_threshold; ++t) wide = wide && aligned16(threshold[t]);
  const int n_code = 2 * (n_member + 1) + 1;
  EventParams p{};
  p.ens = ens;
  p.truth = truth;
  p.ens_slab = reinterpret_cast<const long long*>(ens_slab);
  p.truth_slab = reinterpret_cast<const long long*>(truth_slab);
  p.col_class = col_class;
  p.cnt_thr_stride = (long long)n_outer * n_row * n_class * n_code;
  p.member_stride = member_stride;
  p.n_outer = n_outer;
  p.n_member = n_member;
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
  // more thresholds than one launch takes: further launches, each with its
  // own read of the members
  for (int t0 = 0; t0 < n_threshold; t0 += g.thresholds_per_launch) {
    const int nt = n_threshold - t0 < g.thresholds_per_launch
                       ? n_threshold - t0 : g.thresholds_per_launch;
    for (int t = 0; t < kEventThr; ++t) {
      p.thr[t] = t < nt ? threshold[t0 + t] : nullptr;
      p.thr_slab[t] = (t < nt && thr_slab)
          ? reinterpret_cast<const long long*>(thr_slab) +
                (long long)(t0 + t) * n_outer
          : nullptr;
    }
    p.cnt = cnt + t0 * p.cnt_thr_stride;
    const size_t lds = (size_t)nt * g.rows_per_group * n_class * n_code * 4;
    for_field(dtype, wide, [&](auto T0, auto V) {
      launch_counts<decltype(T0), decltype(V)::value>(nt, grid, lds, s, p);
    });
    WB2_HIP_OK(hipGetLastError());
  }
  return 0;
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
