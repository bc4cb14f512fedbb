// Helpers shared by the derived-variable kernels (derived_fields.hip,
// derived_column.hip): streaming loads and stores of VEC adjacent points and
// np.gradient at one point.
#pragma once

#include "common.hpp"

namespace wb2 {

template <typename T, int VEC>
__device__ __forceinline__ void load_v(const T* p, T (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = __builtin_nontemporal_load(p);
  } else {
    typedef T V __attribute__((ext_vector_type(VEC)));
    const V x = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = x[e];
  }
}

// (rows that are read again by the neighbouring lanes / the next row chunk)
template <typename T, int VEC>
__device__ __forceinline__ void load_cached(const T* p, T (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = *p;
  } else {
    typedef T V __attribute__((ext_vector_type(VEC)));
    const V x = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = x[e];
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void store_v(T* p, const T (&v)[VEC]) {
  if constexpr (VEC == 1) {
    __builtin_nontemporal_store(v[0], p);
  } else if constexpr (sizeof(T) * VEC > 16) {
    // 32 bytes per lane (four doubles): two 16-byte stores
    T lo[VEC / 2], hi[VEC / 2];
#pragma unroll
    for (int e = 0; e < VEC / 2; ++e) {
      lo[e] = v[e];
      hi[e] = v[VEC / 2 + e];
    }
    store_v<T, VEC / 2>(p, lo);
    store_v<T, VEC / 2>(p + VEC / 2, hi);
  } else {
    typedef T V __attribute__((ext_vector_type(VEC)));
    V x;
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = v[e];
    __builtin_nontemporal_store(x, reinterpret_cast<V*>(p));
  }
}

// correctly rounded (IEEE) square roots, whatever the fast-math defaults are
__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sqrt_rn(double x) { return __builtin_sqrt(x); }

// np.gradient(edge_order=1) at one point: `lo`, `mid`, `hi` are the values at
// i - 1, i, i + 1 with the index clamped to the axis, so that the one-sided
// ends are (hi - lo) / den as well.
template <typename T>
__device__ __forceinline__ T gradient_at(T lo, T mid, T hi, bool diff_form,
                                         double a, double b, double c,
                                         double den) {
  if (diff_form) return (T)((double)(T)(hi - lo) / den);
  return (T)((a * (double)lo + b * (double)mid) + c * (double)hi);
}

}  // namespace wb2
