// K14 of libwb2hip.so: day-of-year climatology from one read
// (scripts/compute_climatology.py, weatherbench2/utils.py:73-287).
//
//   wb2_group_moments  count, sum and sum of squares, about a per-point pivot,
//                      of every group of time steps of every point
//   wb2_first_finite   the pivot plane: the first finite sample of every point
//   wb2_cycle_smooth   the moments (or per-position statistics) combined over a
//                      cyclic, weighted window into mean and std
//
// The reference stacks the years, pads the day-of-year axis cyclically, builds
// a W-wide window and takes a weighted mean or std over (window, year).  The
// weights do not depend on the year and the padding wraps inside each year's
// row, so the statistic is a cyclic weighted combination of per-day-of-year
// moments over the years; nothing is read W times.
//
// Semantics (weatherbench2_amd/climatology.py holds the same text):
//   explicit  per hour and point, A the sorted union of the days of year
//             present (n of them, 365 among them), X[y, a] the sample of year
//             y or NaN; a NaN X[y, a] is replaced by X[y, doy 365] (fillna:
//             day 366 of a common year, gap days and data NaNs alike).  Over
//             the entries that are not NaN, positions mod n, H = W / 2:
//               mean[a] = S_y S_k w[k+H] X[y, a+k] / S_y S_k w[k+H]
//               std[a]  = sqrt(S w (X - mean[a])^2 / S w),  k = -H .. H
//             NaN where no entry is left.
//   fast      m[a], s[a] the NaN-skipping mean and ddof=0 std of the group of
//             day a (no fill, no year alignment); the result at a is the
//             NaN-skipping plain mean over i = -H .. H of
//             v[(a - i) mod n] * w[i+H].
// With p the pivot of the point, y = double(x) - p, (C, S, Q) = (count, sum y,
// sum y^2) of a group: mean = p + S/C, variance = Q/C - (S/C)^2; the window
// form replaces (C, S, Q) by their weighted sums.  Moments about zero lose the
// variance of data far from zero (offset 1e5: 4e-7 relative in the std); about
// a sample of the point itself they do not.
//
// The data is T[n_outer][n_time][n_point] as in K13: time step t of outer
// index o starts `slab[o * n_time + t] * n_point` elements after the input's
// base (identity when the table is NULL).  A thread owns VEC adjacent points
// and requests kAhead members before it combines any; a workgroup handles one
// point tile of one group; no atomics, no LDS.  All sums run in member order
// in float64 without FMA contraction (-ffp-contract=off), so a NumPy loop in
// the same order has the same bits.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kMomThreads = 256;
constexpr int kAhead = 4;  // members loaded before any is combined

struct MomentParams {
  const void* in;
  const long long* slab;   // [n_outer][n_time] or null
  const int* group_begin;  // [n_group + 1]
  const int* member;       // [n_member] time steps; outside [0, n_time): absent
  const int* fill;         // [n_member] or null
  const double* pivot;     // [n_outer][n_point] or null
  double* out[3];          // count, sum, sumsq: [n_outer][n_group][n_point]
  long long n_outer, n_point, n_tile;
  int n_time, n_group, n_member;
};

template <typename T, int VEC>
__global__ void __launch_bounds__(kMomThreads)
    group_moments_kernel(const MomentParams p) {
  const long long tile = blockIdx.x % p.n_tile;
  const int g = (int)(blockIdx.x / p.n_tile);
  const long long q = (tile * kMomThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  constexpr int U = kAhead;
  const long long row = o * p.n_time;
  const T* in = static_cast<const T*>(p.in) + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  // (a list that does not fit the members is cut to them, never followed)
  const int begin = max(0, min(p.group_begin[g], p.n_member));
  const int end = max(begin, min(p.group_begin[g + 1], p.n_member));
  double piv[VEC], cnt[VEC], sum[VEC], sq[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    piv[e] = p.pivot ? p.pivot[o * p.n_point + q + e] : 0.0;
    cnt[e] = sum[e] = sq[e] = 0.0;
  }
  const T nan = quiet_nan<T>();
  for (int j0 = begin; j0 < end; j0 += U) {
    T cur[U][VEC];
    int fl[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      // (members past the end are read from the last one and dropped)
      const int j = min(j0 + k, end - 1);
      const int t = p.member[j];
      const int f = p.fill ? p.fill[j] : -1;
      fl[k] = f >= 0 && f < p.n_time ? f : -1;
      if (t >= 0 && t < p.n_time) {
        load_v<T, VEC>(in + (slab ? slab[t] : row + t) * p.n_point, cur[k]);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) cur[k][e] = nan;
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (j0 + k < end) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || cur[k][e] != cur[k][e];
        if (any && fl[k] >= 0) {
          T sub[VEC];
          load_cached<T, VEC>(
              in + (slab ? slab[fl[k]] : row + fl[k]) * p.n_point, sub);
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            cur[k][e] = cur[k][e] != cur[k][e] ? sub[e] : cur[k][e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const T x = cur[k][e];
          if (x == x) {
            const double y = (double)x - piv[e];
            cnt[e] += 1.0;
            sum[e] += y;
            sq[e] += y * y;
          }
        }
      }
    }
  }
  const long long at = (o * p.n_group + g) * p.n_point + q;
  store_v<double, VEC>(p.out[0] + at, cnt);
  store_v<double, VEC>(p.out[1] + at, sum);
  store_v<double, VEC>(p.out[2] + at, sq);
}

struct PivotParams {
  const void* in;
  const long long* slab;
  const int* member;
  double* pivot;  // [n_outer][n_point]
  long long n_outer, n_point, n_tile;
  int n_time, n_member;
};

template <typename T, int VEC>
__global__ void __launch_bounds__(kMomThreads)
    first_finite_kernel(const PivotParams p) {
  const long long q = ((long long)blockIdx.x * kMomThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const long long row = o * p.n_time;
  const T* in = static_cast<const T*>(p.in) + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  double piv[VEC];
  bool found[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    piv[e] = 0.0;
    found[e] = false;
  }
  for (int j = 0; j < p.n_member; ++j) {
    const int t = p.member[j];
    if (t < 0 || t >= p.n_time) continue;
    T cur[VEC];
    load_cached<T, VEC>(in + (slab ? slab[t] : row + t) * p.n_point, cur);
    bool all = true;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const T x = cur[e];
      // (x - x is 0 for a finite x, NaN for NaN and +-inf)
      if (!found[e] && x - x == T(0)) {
        piv[e] = (double)x;
        found[e] = true;
      }
      all = all && found[e];
    }
    if (all) break;
  }
  store_v<double, VEC>(p.pivot + o * p.n_point + q, piv);
}

struct SmoothParams {
  const double* mom[3];  // count, sum, sumsq: [n_outer][n_group][n_point]
  const double* pivot;   // [n_outer][n_point] or null
  const double* w;       // [n_w]
  double* mean;          // [n_outer][n_group][n_point] or null
  double* std;           // the same
  long long n_outer, n_point, n_tile;
  int n_cycle, n_pos, n_w, fast;
};

__device__ __forceinline__ double clamped_sqrt(double v) {
  // (written so, a NaN v stays NaN)
  return sqrt_rn(v < 0.0 ? 0.0 : v);
}

__global__ void __launch_bounds__(kMomThreads)
    cycle_smooth_kernel(const SmoothParams p) {
  const long long tile = blockIdx.x % p.n_tile;
  const int g = (int)(blockIdx.x / p.n_tile);
  const long long q = tile * kMomThreads + threadIdx.x;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const int n_group = p.n_cycle * p.n_pos;
  const int c = g / p.n_pos, a = g % p.n_pos;
  const int half = p.n_w / 2;
  const double piv = p.pivot ? p.pivot[o * p.n_point + q] : 0.0;
  const double nan = __builtin_nan("");
  const long long base = (o * n_group + (long long)c * p.n_pos) * p.n_point + q;
  double mean, std;
  if (!p.fast) {
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    for (int k = -half; k <= half; ++k) {
      int at = (a + k) % p.n_pos;
      at += at < 0 ? p.n_pos : 0;
      const long long i = base + at * p.n_point;
      const double w = p.w[k + half];
      w0 += w * p.mom[0][i];
      w1 += w * p.mom[1][i];
      w2 += w * p.mom[2][i];
    }
    const double m = w1 / w0;
    const double v = w2 / w0 - m * m;
    mean = w0 == 0.0 ? nan : piv + m;
    std = w0 == 0.0 ? nan : clamped_sqrt(v);
  } else {
    double tm = 0.0, ts = 0.0;
    int nm = 0, ns = 0;
    for (int k = -half; k <= half; ++k) {
      int at = (a - k) % p.n_pos;
      at += at < 0 ? p.n_pos : 0;
      const long long i = base + at * p.n_point;
      const double w = p.w[k + half];
      const double cn = p.mom[0][i];
      const double m = p.mom[1][i] / cn;
      const double v = p.mom[2][i] / cn - m * m;
      const double pm = (cn == 0.0 ? nan : piv + m) * w;
      const double ps = (cn == 0.0 ? nan : clamped_sqrt(v)) * w;
      if (pm == pm) {
        tm += pm;
        ++nm;
      }
      if (ps == ps) {
        ts += ps;
        ++ns;
      }
    }
    mean = nm ? tm / (double)nm : nan;
    std = ns ? ts / (double)ns : nan;
  }
  const long long out = (o * n_group + g) * p.n_point + q;
  if (p.mean) p.mean[out] = mean;
  if (p.std) p.std[out] = std;
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_climatology_geometry(int dtype, int wide, int32_t* tile_points,
                             int32_t* members_ahead, int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && members_ahead && max_grid_outer,
              "null pointer argument");
  *tile_points = kMomThreads * (wide ? wide_lanes(dtype) : 1);
  *members_ahead = kAhead;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_group_moments(int dtype, const void* in, const int64_t* slab,
                      int64_t n_outer, int32_t n_time, int64_t n_point,
                      const int32_t* group_begin,
                      const int32_t* group_begin_host, int32_t n_group,
                      const int32_t* member, const int32_t* fill,
                      int32_t n_member, const double* pivot, double* count,
                      double* sum, double* sumsq, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_time >= 0 && n_member >= 0,
              "bad sizes: n_time=%d or n_member=%d is negative", (int)n_time,
              (int)n_member);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_group);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(group_begin && group_begin_host && count && sum && sumsq,
              "null pointer argument");
  WB2_REQUIRE((in || n_time == 0) && (member || n_member == 0),
              "null pointer argument");
  WB2_REQUIRE(group_begin_host[0] == 0 && group_begin_host[n_group] == n_member,
              "group_begin does not fit the members: it runs from %d to %d, "
              "n_member=%d", (int)group_begin_host[0],
              (int)group_begin_host[n_group], (int)n_member);
  for (int g = 0; g < n_group; ++g)
    WB2_REQUIRE(group_begin_host[g] <= group_begin_host[g + 1],
                "group_begin does not fit the members: it decreases at group "
                "%d", g);
  const int w = wide_lanes(dtype);
  const bool wide = n_point % w == 0 &&
                    all_aligned16(in, count, sum, sumsq) &&
                    reinterpret_cast<uintptr_t>(pivot) % 8 == 0;
  const int vec = wide ? w : 1;
  MomentParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.group_begin = group_begin;
  p.member = member;
  p.fill = fill;
  p.pivot = pivot;
  p.out[0] = count;
  p.out[1] = sum;
  p.out[2] = sumsq;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_tile = point_tiles(n_point, vec, kMomThreads);
  p.n_time = n_time;
  p.n_group = n_group;
  p.n_member = n_member;
  dim3 grid;
  WB2_REQUIRE(p.n_tile < (1ll << 31) && outer_grid(n_outer, p.n_tile * n_group,
                                                    &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL((group_moments_kernel<T, V>), grid, dim3(kMomThreads),
                       0, s, p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_first_finite(int dtype, const void* in, const int64_t* slab,
                     int64_t n_outer, int32_t n_time, int64_t n_point,
                     const int32_t* member, int32_t n_member, double* pivot,
                     void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_time >= 0 && n_member >= 0,
              "bad sizes: n_time=%d or n_member=%d is negative", (int)n_time,
              (int)n_member);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(pivot, "null pointer argument");
  WB2_REQUIRE((in || n_time == 0) && (member || n_member == 0),
              "null pointer argument");
  const int w = wide_lanes(dtype);
  const bool wide = n_point % w == 0 && all_aligned16(in, pivot);
  const int vec = wide ? w : 1;
  PivotParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.member = member;
  p.pivot = pivot;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_tile = point_tiles(n_point, vec, kMomThreads);
  p.n_time = n_time;
  p.n_member = n_member;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_outer, p.n_tile, &grid), "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL((first_finite_kernel<T, V>), grid, dim3(kMomThreads),
                       0, s, p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_cycle_smooth(int mode, const double* count, const double* sum,
                     const double* sumsq, const double* pivot, int64_t n_outer,
                     int32_t n_cycle, int32_t n_pos, int64_t n_point,
                     const double* weights, int32_t n_w, double* mean,
                     double* std, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(mode == WB2_SMOOTH_EXPLICIT || mode == WB2_SMOOTH_FAST,
              "unknown smoothing mode %d", mode);
  WB2_REQUIRE(n_w > 0 && n_w % 2 == 1,
              "the window must have an odd, positive number of weights: "
              "n_w=%d", (int)n_w);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_cycle);
  WB2_EMPTY_OK(n_pos);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(count && sum && sumsq && weights, "null pointer argument");
  if (!mean && !std) return 0;
  SmoothParams p{};
  p.mom[0] = count;
  p.mom[1] = sum;
  p.mom[2] = sumsq;
  p.pivot = pivot;
  p.w = weights;
  p.mean = mean;
  p.std = std;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_tile = point_tiles(n_point, 1, kMomThreads);
  p.n_cycle = n_cycle;
  p.n_pos = n_pos;
  p.n_w = n_w;
  p.fast = mode == WB2_SMOOTH_FAST;
  const long long n_group = (long long)n_cycle * n_pos;
  dim3 grid;
  WB2_REQUIRE(n_group < (1ll << 31) && p.n_tile < (1ll << 31) &&
                  outer_grid(n_outer, p.n_tile * n_group, &grid),
              "bad sizes");
  hipLaunchKernelGGL(cycle_smooth_kernel, grid, dim3(kMomThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
