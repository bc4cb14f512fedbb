// K10 of libwb2hip.so: derived variables that act along the lead-time axis
// (weatherbench2/derived_variables.py).
//
//   wb2_derived_lead_window  PrecipitationAccumulation :504-528 (the rolling
//                            sum of lead-to-lead differences, clamped at zero)
//                            and AggregatePrecipitationAccumulation :709-720
//                            (the rolling sum itself)
//
// The data is [n_outer][n_lead][n_point]: consecutive leads of a point lie a
// whole slab apart.  A thread owns VEC adjacent points of the contiguous inner
// block and walks the leads; lead l of outer index o starts `slab[o * n_lead +
// l] * n_point` elements after the input's base (identity when the table is
// NULL), so contiguous tensors, lead-sliced views and gathers are read where
// they lie.  Every lead is written, unlike the reducing modes of K9.
//
// xarray's rolling(dim=w).sum() with min_periods = w: a window with a NaN
// gives NaN and the result recovers once the NaN has left, so every window is
// summed afresh, oldest term first, in the field's dtype T (-ffp-contract=off)
// -- no running update.  The last w terms live in a register ring; the lead
// loop is unrolled by a multiple of w so that every ring index is static (a
// dynamically indexed ring would live in scratch).  As in K9 a launch has few
// workgroups per CU, so a thread requests kLeadAhead leads before it combines
// any.  Windows without an instantiation re-read their terms from memory.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kLeadThreads = 256;
constexpr int kLeadAhead = 4;  // leads loaded before any is combined
// window counts with a register ring: 6-hourly data (1, 4), 12-hourly (2),
// 3-hourly (2, 8), hourly (6, 24)
constexpr int32_t kLeadWindows[] = {1, 2, 4, 6, 8, 24};
constexpr int kNumLeadWindows = sizeof(kLeadWindows) / sizeof(kLeadWindows[0]);

struct LeadParams {
  const void* in;
  const long long* slab;  // [n_outer][n_lead] or null
  void* out;
  long long n_outer, n_point;
  int n_lead, window, clamp;
};

constexpr int lead_block(int w) {  // the least common multiple of w and Ahead
  int b = w;
  while (b % kLeadAhead) b += w;
  return b;
}

template <typename T, int VEC, int W, int MODE>
__global__ void __launch_bounds__(kLeadThreads)
    lead_window_kernel(const LeadParams p) {
  const long long q =
      ((long long)blockIdx.x * kLeadThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  constexpr bool DIFF = MODE == WB2_LEAD_DIFF_SUM;
  constexpr int U = kLeadAhead;
  constexpr int B = lead_block(W);
  constexpr int first = DIFF ? W : W - 1;  // the first lead with a full window
  const int n_lead = p.n_lead;
  const long long row = o * n_lead;
  const T* in = static_cast<const T*>(p.in) + q;
  T* out = static_cast<T*>(p.out) + row * p.n_point + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  const bool clamp = p.clamp != 0;
  // term l = x[l] - x[l - 1] (DIFF) or x[l], kept in ring[l % W]
  T ring[W][VEC], prev[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    prev[e] = T(0);
#pragma unroll
    for (int k = 0; k < W; ++k) ring[k][e] = T(0);
  }
  for (int lb = 0; lb < n_lead; lb += B) {
#pragma unroll
    for (int g = 0; g < B; g += U) {
      if (lb + g >= n_lead) break;
      T cur[U][VEC];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        // (leads past the end are read from the last one and dropped)
        const int l = min(lb + g + k, n_lead - 1);
        load_v<T, VEC>(in + (slab ? slab[l] : row + l) * p.n_point, cur[k]);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int l = lb + g + k;
        if (l < n_lead) {
          const int slot = (g + k) % W;  // == l % W: lb is a multiple of W
          T r[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            ring[slot][e] = DIFF ? cur[k][e] - prev[e] : cur[k][e];
            prev[e] = cur[k][e];
            T s = ring[(slot + 1) % W][e];  // the oldest term of the window
#pragma unroll
            for (int j = 2; j <= W; ++j) s = s + ring[(slot + j) % W][e];
            if (DIFF && clamp && s < T(0)) s = T(0);  // (NaN, -0.0: kept)
            r[e] = l < first ? quiet_nan<T>() : s;
          }
          store_v<T, VEC>(out + (long long)l * p.n_point, r);
        }
      }
    }
  }
}

// Any window count: the terms of every window are read again (from cache,
// mostly).  One point per thread; correct, not fast.
template <typename T, int MODE>
__global__ void __launch_bounds__(kLeadThreads)
    lead_window_reread_kernel(const LeadParams p) {
  const long long q = (long long)blockIdx.x * kLeadThreads + threadIdx.x;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  constexpr bool DIFF = MODE == WB2_LEAD_DIFF_SUM;
  const int n_lead = p.n_lead, w = p.window;
  const long long row = o * n_lead;
  const T* in = static_cast<const T*>(p.in) + q;
  T* out = static_cast<T*>(p.out) + row * p.n_point + q;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  const long long first = DIFF ? (long long)w : (long long)w - 1;
  for (int l = 0; l < n_lead; ++l) {
    T s = quiet_nan<T>();
    if (l >= first) {
      int j = l - w + 1;
      T before = T(0);
      if (DIFF) before = in[(slab ? slab[j - 1] : row + j - 1) * p.n_point];
      for (; j <= l; ++j) {
        const T x = in[(slab ? slab[j] : row + j) * p.n_point];
        const T term = DIFF ? x - before : x;
        before = x;
        s = j == l - w + 1 ? term : s + term;
      }
      if (DIFF && p.clamp && s < T(0)) s = T(0);
    }
    out[(long long)l * p.n_point] = s;
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_derived_lead_geometry(int dtype, int wide, int32_t* tile_points,
                              int32_t* leads_ahead, const int32_t** windows,
                              int32_t* n_windows) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && leads_ahead && windows && n_windows,
              "null pointer argument");
  *tile_points = kLeadThreads * (wide ? wide_lanes(dtype) : 1);
  *leads_ahead = kLeadAhead;
  *windows = kLeadWindows;
  *n_windows = kNumLeadWindows;
  return 0;
}

int wb2_derived_lead_window(int mode, int dtype, const void* in,
                            const int64_t* slab, int64_t n_outer,
                            int32_t n_lead, int64_t n_point, int32_t window,
                            int clamp_negative, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(mode == WB2_LEAD_DIFF_SUM || mode == WB2_LEAD_SUM,
              "unknown mode %d", mode);
  WB2_REQUIRE(window >= 1, "bad sizes: a window of %d leads", (int)window);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_lead);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(in && out, "null pointer argument");
  WB2_REQUIRE((n_point + kLeadThreads - 1) / kLeadThreads < (1ll << 31),
              "bad sizes");
  LeadParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.out = out;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_lead = n_lead;
  p.window = window;
  p.clamp = clamp_negative;
  bool ring = false;
  for (int k = 0; k < kNumLeadWindows; ++k) ring = ring || kLeadWindows[k] == window;
  const int w = wide_lanes(dtype);
  const bool wide = ring && n_point % w == 0 && all_aligned16(in, out);
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_outer,
                         point_tiles(n_point, wide ? w : 1, kLeadThreads),
                         &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kLeadThreads), 0, s, p);
  };
  auto launch_ring = [&](auto window_of) {
    constexpr int W = decltype(window_of)::value;
    for_field(dtype, wide, [&](auto t, auto v) {
      using T = decltype(t);
      constexpr int V = decltype(v)::value;
      if (mode == WB2_LEAD_DIFF_SUM)
        launch(lead_window_kernel<T, V, W, WB2_LEAD_DIFF_SUM>);
      else
        launch(lead_window_kernel<T, V, W, WB2_LEAD_SUM>);
    });
  };
  // (a switch and not a loop: the window is a template argument)
  switch (ring ? window : 0) {
    case 1: launch_ring(std::integral_constant<int, 1>{}); break;
    case 2: launch_ring(std::integral_constant<int, 2>{}); break;
    case 4: launch_ring(std::integral_constant<int, 4>{}); break;
    case 6: launch_ring(std::integral_constant<int, 6>{}); break;
    case 8: launch_ring(std::integral_constant<int, 8>{}); break;
    case 24: launch_ring(std::integral_constant<int, 24>{}); break;
    default:
      for_field(dtype, false, [&](auto t, auto) {
        using T = decltype(t);
        if (mode == WB2_LEAD_DIFF_SUM)
          launch(lead_window_reread_kernel<T, WB2_LEAD_DIFF_SUM>);
        else
          launch(lead_window_reread_kernel<T, WB2_LEAD_SUM>);
      });
  }
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
