// K23 of libwb2hip.so: count-weighted means of a time axis, one per bootstrap
// replicate (the block bootstrap of weatherbench2_amd/bootstrap.py; the
// reference has no counterpart).
//
//   wb2_resampled_means  out[b][o][p] = sum_t n[b][t] x[o][t][p] / sum_t n[b][t]
//                        in the order stated in wb2hip.h
//
// The data is K13's [n_outer][n_time][n_point] with K13's slab table, read
// where it lies.  A thread owns VEC adjacent points and keeps the chains of
// kRepsPerGroup replicates in registers, so every value it loads serves that
// many replicates.  It requests the steps_ahead time steps after the ones it
// is combining before it combines any of them.  The counts of a (replicate
// group, time step) do not depend on the thread: they arrive widened to
// float64 as [n_group][n_time padded][kRepsPerGroup], so the counts a group
// needs next are the next bytes, two steps' are one batch of scalar loads, and
// a zero count (all its bits are zero) is a branch the whole wave takes.  The
// workgroups of one point tile (its replicate groups) are neighbours in the
// grid: they run together and share the tile's cache lines.
//
// Two identities keep the inner loop to one operation per (count, value):
//   * a chain starts at -0.0: (-0.0) + term has the bits of term for every
//     term (+-0.0, +-inf and NaN included), so "the first used term starts the
//     chain" needs no flag, and no used term leaves -0.0 / 0.0 = NaN;
//   * with skipna a NaN enters as -0.0: n * (-0.0) = -0.0 and S + (-0.0) has
//     the bits of S for every S, which is "left out".  Its count is
//     subtracted from W in an integer per point, in a branch a wave takes only
//     at a step where one of its points holds a NaN.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kMeanThreads = 256;
// time steps requested ahead of the combining: 4 of float64; 2 of float32,
// whose 4 points a thread leave fewer registers (a third wave per SIMD fits)
constexpr int steps_ahead(int dtype) { return dtype == WB2_F32 ? 2 : 4; }
constexpr int kMaxStepsAhead = 4;
constexpr int kRepsPerGroup = 16;  // replicates whose chains a thread keeps
constexpr int kCountSteps = 2;     // time steps per batch of scalar loads

struct MeanParams {
  const void* in;
  const long long* slab;  // [n_outer][n_time] or null
  const double* weights;  // [n_group][n_time_pad][kRepsPerGroup]
  const double* totals;   // [n_group * kRepsPerGroup]
  double* out;            // [n_rep][n_outer][n_point]
  long long n_outer, n_point;
  int n_time, n_time_pad, n_rep, n_group;
};

template <typename T, int VEC, bool SKIPNA>
__global__ void __launch_bounds__(kMeanThreads)
    resampled_means_kernel(const MeanParams p) {
  constexpr int U = steps_ahead(sizeof(T) == 4 ? WB2_F32 : WB2_F64);
  constexpr int G = kRepsPerGroup, H = kCountSteps;
  constexpr int NM = SKIPNA ? VEC : 1;
  const int group = (int)(blockIdx.x % (unsigned)p.n_group);
  const long long tile = blockIdx.x / (unsigned)p.n_group;
  const long long q = (tile * kMeanThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const long long row = o * p.n_time;
  const T* in = static_cast<const T*>(p.in) + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  const int b0 = group * G;
  // (the constant address space: scalar loads whatever else the loop holds)
  // and the bits of a count: the zero test is an integer's, on the scalar unit
  typedef const unsigned long long __attribute__((address_space(4))) * Uniform;
  const Uniform weights =
      (Uniform)(p.weights + (long long)group * p.n_time_pad * G);
  double sum[G][VEC];
  int missed[G][NM];  // (skipna) the counts of the NaNs of a point
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) sum[g][e] = -0.0;
#pragma unroll
    for (int e = 0; e < NM; ++e) missed[g][e] = 0;
  }
  // (steps past the end are read from the last one; their counts, the padding
  // of the table, are zero)
  auto request = [&](int t0, T (&v)[U][VEC]) {
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int t = min(t0 + k, p.n_time - 1);
      load_cached<T, VEC>(in + (slab ? slab[t] : row + t) * p.n_point, v[k]);
    }
  };
  T cur[U][VEC], nxt[U][VEC];
  request(0, cur);
  for (int t0 = 0; t0 < p.n_time; t0 += U) {
    request(t0 + U, nxt);
#pragma unroll
    for (int h = 0; h < U; h += H) {
      unsigned long long weight[H][G];
#pragma unroll
      for (int j = 0; j < H; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g)
          weight[j][g] = weights[(long long)(t0 + h + j) * G + g];
#pragma unroll
      for (int j = 0; j < H; ++j) {
        double x[VEC];
        bool isnan[VEC];
        bool some = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          x[e] = (double)cur[h + j][e];
          isnan[e] = SKIPNA && x[e] != x[e];
          some = some || isnan[e];
          if (isnan[e]) x[e] = -0.0;
        }
        const bool any_nan = SKIPNA && __any(some);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          // a step the replicate did not draw is left out
          if (weight[j][g] != 0) {
            const double w = __builtin_bit_cast(double, weight[j][g]);
            // (keeps the branch a branch: turned into selects, the skipped
            // terms would cost as much as the used ones, and twice)
            asm volatile("");
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              // (float32: n * x is exact in float64, the fma has the same bits)
              if constexpr (sizeof(T) == 4)
                sum[g][e] = __builtin_fma(w, x[e], sum[g][e]);
              else
                sum[g][e] = sum[g][e] + w * x[e];
            }
            if constexpr (SKIPNA) {
              if (any_nan) {
                const int n = (int)w;
#pragma unroll
                for (int e = 0; e < VEC; ++e) missed[g][e] += isnan[e] ? n : 0;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) cur[k][e] = nxt[k][e];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (b0 + g < p.n_rep) {
      const double total =
          __builtin_bit_cast(double, ((Uniform)p.totals)[b0 + g]);
      double r[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        r[e] = sum[g][e] / (total - (double)missed[g][SKIPNA ? e : 0]);
      store_v<double, VEC>(
          p.out + ((long long)(b0 + g) * p.n_outer + o) * p.n_point + q, r);
    }
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_resampled_means_geometry(int dtype, int wide, int32_t* tile_points,
                                 int32_t* replicates_per_group,
                                 int32_t* steps_ahead,
                                 int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && replicates_per_group && steps_ahead &&
                  max_grid_outer,
              "null pointer argument");
  *tile_points = kMeanThreads * (wide ? wide_lanes(dtype) : 1);
  *replicates_per_group = kRepsPerGroup;
  *steps_ahead = wb2::steps_ahead(dtype);
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_resampled_means(int dtype, int skipna, const void* in,
                        const int64_t* slab, int64_t n_outer, int32_t n_time,
                        int64_t n_point, const double* weights,
                        const double* totals, int32_t n_rep, double* out,
                        void* stream) {
  WB2_TRACE();
  using namespace wb2;
  static_assert(steps_ahead(WB2_F32) % kCountSteps == 0 &&
                    steps_ahead(WB2_F64) % kCountSteps == 0,
                "whole batches of counts");
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_rep >= 1 && n_time >= 1 && n_point >= 1 && n_outer >= 0 &&
                  n_time <= INT32_MAX - kMaxStepsAhead,
              "bad sizes: n_rep=%d n_time=%d n_point=%lld n_outer=%lld",
              (int)n_rep, (int)n_time, (long long)n_point,
              (long long)n_outer);
  WB2_EMPTY_OK(n_outer);
  WB2_REQUIRE(in && weights && totals && out, "null pointer argument");
  const int w = wide_lanes(dtype);
  const bool wide = n_point % w == 0 && aligned16(in) && aligned16(out);
  const int vec = wide ? w : 1;
  MeanParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.weights = weights;
  p.totals = totals;
  p.out = out;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_time = n_time;
  const int ahead = steps_ahead(dtype);
  p.n_time_pad = (n_time + ahead - 1) / ahead * ahead;
  p.n_rep = n_rep;
  p.n_group = (n_rep + kRepsPerGroup - 1) / kRepsPerGroup;
  const long long n_tile = point_tiles(n_point, vec, kMeanThreads);
  dim3 grid;
  WB2_REQUIRE(n_tile < (1ll << 31) &&
                  outer_grid(n_outer, n_tile * p.n_group, &grid),
              "bad sizes: the problem does not fit a grid");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    if (skipna)
      hipLaunchKernelGGL((resampled_means_kernel<T, V, true>), grid,
                         dim3(kMeanThreads), 0, s, p);
    else
      hipLaunchKernelGGL((resampled_means_kernel<T, V, false>), grid,
                         dim3(kMeanThreads), 0, s, p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
