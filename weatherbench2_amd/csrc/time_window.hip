// K13 of libwb2hip.so: statistics over runs of a time axis
// (scripts/resample_in_time.py:270-309, xarray's resample(...) and
// rolling(...) followed by mean / min / max / sum).
//
//   wb2_time_bin_stats  sum, mean, min and max of every bin [begin, end) of the
//                       time steps of every point, all from one read
//
// The data is [n_outer][n_time][n_point]: consecutive time steps of a point lie
// a whole slab apart.  A thread owns VEC adjacent points of the contiguous
// inner block; time step t of outer index o starts `slab[o * n_time + t] *
// n_point` elements after the input's base (identity when the table is NULL),
// so contiguous tensors, time-sliced views, gathers and permuted time orders
// are read where they lie.  A workgroup handles one tile of points and
// bins_per_group consecutive bins, one after another; every bin is computed
// afresh, oldest sample first, in the field's dtype T (-ffp-contract=off), so
// disjoint bins (resampling) and overlapping ones (rolling windows) are the
// same code and a NaN touches exactly the bins that hold it.  As in K9/K10 a
// thread requests kStepsAhead time steps before it combines any.  A group of
// several bins reads with cached loads (the terms that neighbouring windows
// share come from the workgroup's own cache lines), a group of one streams.
//
// All four statistics are always formed (the kernel is bound by its loads);
// the mask only decides which are stored, so a statistic has the same bits
// whatever else was asked for.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kBinThreads = 256;
constexpr int kStepsAhead = 4;  // time steps loaded before any is combined

struct BinParams {
  const void* in;
  const long long* slab;  // [n_outer][n_time] or null
  const int* range;       // [n_bin][2]
  void* out[4];           // sum, mean, min, max; null = not stored
  long long n_outer, n_point, n_tile;
  int n_time, n_bin, bins_per_group;
};

template <typename T, int VEC, bool SKIPNA>
__global__ void __launch_bounds__(kBinThreads)
    time_bin_kernel(const BinParams p) {
  const long long tile = blockIdx.x % p.n_tile;
  const int group = (int)(blockIdx.x / p.n_tile);
  const long long q = (tile * kBinThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  constexpr int U = kStepsAhead;
  const long long row = o * p.n_time;
  const T* in = static_cast<const T*>(p.in) + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  const bool reuse = p.bins_per_group > 1;
  const int b0 = group * p.bins_per_group;
  const int b1 = min(b0 + p.bins_per_group, p.n_bin);
  for (int b = b0; b < b1; ++b) {
    const int begin = p.range[2 * b], end = p.range[2 * b + 1];
    // (a range that leaves the series is treated as incomplete, not read)
    const bool valid = begin >= 0 && begin < end && end <= p.n_time;
    T sum[VEC], mn[VEC], mx[VEC];
    int count[VEC];
    bool nan[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      sum[e] = T(0);
      mn[e] = T(__builtin_inff());
      mx[e] = -T(__builtin_inff());
      count[e] = 0;
      nan[e] = false;
    }
    if (valid) {
      for (int t0 = begin; t0 < end; t0 += U) {
        T cur[U][VEC];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          // (steps past the end are read from the last one and dropped)
          const int t = min(t0 + k, end - 1);
          const T* src = in + (slab ? slab[t] : row + t) * p.n_point;
          if (reuse)
            load_cached<T, VEC>(src, cur[k]);
          else
            load_v<T, VEC>(src, cur[k]);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          if (t0 + k < end) {
            const bool first = t0 + k == begin;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const T x = cur[k][e];
              const bool isnan = x != x;
              const T term = SKIPNA && isnan ? T(0) : x;
              sum[e] = first ? term : sum[e] + term;
              nan[e] = nan[e] || isnan;
              count[e] += isnan ? 0 : 1;
              mn[e] = x < mn[e] ? x : mn[e];  // (a NaN never compares)
              mx[e] = x > mx[e] ? x : mx[e];
            }
          }
        }
      }
    }
    T r[4][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int n = SKIPNA ? count[e] : end - begin;
      const bool none = !valid || (SKIPNA ? count[e] == 0 : nan[e]);
      r[0][e] = valid ? sum[e] : quiet_nan<T>();
      r[1][e] = !valid || n == 0 ? quiet_nan<T>() : sum[e] / T(n);
      r[2][e] = none ? quiet_nan<T>() : mn[e];
      r[3][e] = none ? quiet_nan<T>() : mx[e];
    }
    const long long at = (o * p.n_bin + b) * p.n_point + q;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (p.out[s]) store_v<T, VEC>(static_cast<T*>(p.out[s]) + at, r[s]);
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_time_window_geometry(int dtype, int wide, int32_t* tile_points,
                             int32_t* steps_ahead, int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && steps_ahead && max_grid_outer,
              "null pointer argument");
  *tile_points = kBinThreads * (wide ? wide_lanes(dtype) : 1);
  *steps_ahead = kStepsAhead;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_time_bin_stats(int stat_mask, int dtype, int skipna, const void* in,
                       const int64_t* slab, int64_t n_outer, int32_t n_time,
                       int64_t n_point, const int32_t* bin_range,
                       int32_t n_bin, int32_t bins_per_group,
                       void* const* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(stat_mask > 0 && stat_mask <= WB2_STAT_ALL,
              "bad statistic mask %d", stat_mask);
  WB2_REQUIRE(bins_per_group >= 1, "bad sizes: %d bins per group",
              (int)bins_per_group);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_time);
  WB2_EMPTY_OK(n_bin);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(out, "null pointer argument");
  for (int s = 0; s < 4; ++s)
    WB2_REQUIRE(!(stat_mask >> s & 1) || out[s],
                "statistic %d is asked for but has no output", s);
  WB2_REQUIRE(in && bin_range, "null pointer argument");
  const int w = wide_lanes(dtype);
  bool wide = n_point % w == 0 && aligned16(in);
  for (int s = 0; s < 4; ++s)
    if (stat_mask >> s & 1) wide = wide && aligned16(out[s]);
  const int vec = wide ? w : 1;
  BinParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.range = bin_range;
  for (int s = 0; s < 4; ++s) p.out[s] = (stat_mask >> s & 1) ? out[s] : nullptr;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_tile = point_tiles(n_point, vec, kBinThreads);
  p.n_time = n_time;
  p.n_bin = n_bin;
  p.bins_per_group = bins_per_group;
  const long long n_group =
      ((long long)n_bin + bins_per_group - 1) / bins_per_group;
  dim3 grid;
  WB2_REQUIRE(p.n_tile < (1ll << 31) &&
                  outer_grid(n_outer, p.n_tile * n_group, &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    if (skipna)
      hipLaunchKernelGGL((time_bin_kernel<T, V, true>), grid,
                         dim3(kBinThreads), 0, s, p);
    else
      hipLaunchKernelGGL((time_bin_kernel<T, V, false>), grid,
                         dim3(kBinThreads), 0, s, p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
