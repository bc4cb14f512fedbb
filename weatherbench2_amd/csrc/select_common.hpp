// Selection by counting passes, shared by K12 (quantile.hip) and K15
// (climatology_quantile.hip): order-preserving unsigned keys, the common
// leading bits of a series, and sums / extremes over the lanes of a wave that
// share a point.
#pragma once

#include "common.hpp"

namespace wb2 {

constexpr int kQBits = 2;                  // key bits fixed per counting pass
constexpr int kQCand = (1 << kQBits) - 1;  // candidates (counters) per target

template <typename T> struct QKey;
template <> struct QKey<float> { typedef unsigned int type; };
template <> struct QKey<double> { typedef unsigned long long type; };

template <typename T>
__device__ __forceinline__ typename QKey<T>::type to_key(T x) {
  typedef typename QKey<T>::type K;
  if (is_nan(x)) return ~K(0);
  const K b = __builtin_bit_cast(K, x);
  const K sign = K(1) << (sizeof(K) * 8 - 1);
  return (b & sign) ? ~b : (b | sign);
}

template <typename T>
__device__ __forceinline__ T from_key(typename QKey<T>::type k) {
  typedef typename QKey<T>::type K;
  const K sign = K(1) << (sizeof(K) * 8 - 1);
  const K b = (k & sign) ? (k ^ sign) : ~k;
  return __builtin_bit_cast(T, b);
}

__device__ __forceinline__ int leading_zeros(unsigned int x) {
  return __builtin_clz(x);
}
__device__ __forceinline__ int leading_zeros(unsigned long long x) {
  return __builtin_clzll(x);
}

// The number of low key bits the counting passes have to settle: the bits
// below the common prefix of the smallest and the largest key, rounded up to
// whole steps.
template <typename K>
__device__ __forceinline__ int first_shift(K kmin, K kmax) {
  const K x = kmin ^ kmax;
  const int nb = x ? (int)sizeof(K) * 8 - leading_zeros(x) : 0;
  return (nb + kQBits - 1) / kQBits * kQBits;
}

template <typename K>
__device__ __forceinline__ K prefix_above(K key, int shift) {
  return shift >= (int)sizeof(K) * 8 ? K(0) : (key >> shift) << shift;
}

// Sums / extremes over the lanes of a wave that share a point: lane = slice *
// P + point, so the partners differ in the lane bits at and above P.
template <int P, typename V>
__device__ __forceinline__ V slices_sum(V v) {
#pragma unroll
  for (int off = P; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
template <int P, typename K>
__device__ __forceinline__ K slices_min(K v) {
#pragma unroll
  for (int off = P; off < kWave; off <<= 1) {
    const K w = __shfl_xor(v, off, kWave);
    v = w < v ? w : v;
  }
  return v;
}
template <int P, typename K>
__device__ __forceinline__ K slices_max(K v) {
#pragma unroll
  for (int off = P; off < kWave; off <<= 1) {
    const K w = __shfl_xor(v, off, kWave);
    v = w > v ? w : v;
  }
  return v;
}

}  // namespace wb2
