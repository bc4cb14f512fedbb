// The launch vocabulary of the derived kernels (K7 - K16): how outer indices
// are spread over the grid, when a launch may use 16-byte lanes and how a
// (dtype, width) pair picks a kernel instance.
#pragma once

#include <type_traits>
#include <utility>

#include "common.hpp"
#include "wb2hip.h"

namespace wb2 {

// Outer indices (slabs, columns, leads ...) per grid row: gridDim.y takes at
// most this many, gridDim.z the rest.
constexpr long long kGridOuter = 32768;

// the outer index of a workgroup of a grid made by outer_grid()
__device__ __forceinline__ long long outer_index() {
  return blockIdx.y + (long long)blockIdx.z * gridDim.y;
}

// grid rows of outer indices; false if the problem does not fit a grid
inline bool outer_grid(long long n_outer, long long blocks_x, dim3* grid) {
  const long long gy = n_outer < kGridOuter ? n_outer : kGridOuter;
  const long long gz = (n_outer + gy - 1) / gy;
  if (blocks_x >= (1ll << 31) || gz > 65535) return false;
  *grid = dim3((unsigned)blocks_x, (unsigned)gy, (unsigned)gz);
  return true;
}

// elements of a 16-byte lane
inline int wide_lanes(int dtype) { return dtype == WB2_F32 ? 4 : 2; }

inline bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

template <class... P>
inline bool all_aligned16(const P*... p) {
  return (aligned16(p) && ...);
}

// workgroups of `threads` threads of `vec` adjacent points each
inline long long point_tiles(long long n_point, int vec, int threads) {
  return ((n_point + vec - 1) / vec + threads - 1) / threads;
}

template <typename T>
__device__ __forceinline__ T quiet_nan() {
  return (T)__builtin_nanf("");
}

// f(T{}, std::integral_constant<int, VEC>{}) for the field's dtype, with VEC =
// wide_lanes(dtype) when `wide` and 1 otherwise.
template <class F>
void for_field(int dtype, bool wide, F&& f) {
  if (dtype == WB2_F32) {
    if (wide) f(float{}, std::integral_constant<int, 4>{});
    else f(float{}, std::integral_constant<int, 1>{});
  } else {
    if (wide) f(double{}, std::integral_constant<int, 2>{});
    else f(double{}, std::integral_constant<int, 1>{});
  }
}

}  // namespace wb2
