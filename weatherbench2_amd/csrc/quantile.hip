// K12 of libwb2hip.so: exact quantiles along one axis (the numerical content
// of scripts/compute_quantiles.py: xarray's quantile, i.e. NumPy's quantile /
// nanquantile with method='linear').
//
//   wb2_quantile_select    out[q][o][i] = the q-quantile of the series
//                          in[o][0 .. n_red - 1][i]
//
// The data is [n_outer][n_red][n_inner]: consecutive samples of a point lie a
// whole block of n_inner elements apart, and sample r of outer index o starts
// `slab[o * n_red + r] * n_inner` elements after the input's base (identity
// when the table is NULL), so contiguous tensors, sliced views, gathers and
// permuted sample orders are read where they lie.
//
// Selection is exact and sorts nothing.  Every value becomes an unsigned key
// of its own width whose order is the order of the values (sign bit flipped
// for non-negative values, all bits for negative ones); every NaN becomes the
// all-ones key, which no other value maps to, so NaNs sit above +inf and are
// counted in the first pass.  The key of rank `lo` is then found from the
// most significant bit down, kQBits bits per counting pass: with the bits
// above `shift` fixed as `prefix`, the pass counts the keys below each of the
// kQCand candidates prefix | (j << shift); the next digit is the number of
// candidates whose count does not exceed `lo`.  The first pass also takes the
// smallest and largest key of the series: their common leading bits need no
// counting pass (fields like temperature share sign and exponent).  A last
// pass counts the keys <= the found key and takes the smallest key above it:
// s[hi] is the found key again when that count exceeds lo + 1, the key above
// it otherwise.  Values are recovered from keys bit for bit.
//
// Two regimes share the key mapping, the counting step and the interpolation:
//
//   resident   n_red <= kQLdsBytes / 64.  A workgroup stages its tile of
//              P = 64 / sizeof(T) adjacent points (64 bytes per sample row)
//              into LDS once,
//              as keys: the input is read from memory once.  Every pass
//              reads LDS.  A wave serves one quantile of the tile at a time
//              (the four waves four quantiles): its lanes are 64 / P
//              slices of the samples x P points, read 256 consecutive
//              bytes of LDS per step and add the counters of a point up by
//              lane exchange, so the number of quantiles costs waves and not
//              registers.  The LDS of a launch is n_red * 64 bytes, so short
//              series (ensembles) put many workgroups on a CU.
//   streaming  any longer n_red.  A workgroup owns the same tile; its lanes
//              are spread over (point, slice of the samples), walk the
//              samples through the slab table once per pass and add their
//              counters up in LDS (integer atomics: any order gives the same
//              sums).  kQTargets quantiles share a pass, so the input is read
//              1 + ceil(n_q / kQTargets) * (passes + 1) times: from L2 or the
//              Infinity Cache when the tile set fits there.  Correct and
//              simple, not the tuned path.

#include <cmath>

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kQResThreads = 256;
constexpr int kQStrThreads = 512;
constexpr int kQTargets = 4;        // streaming: quantiles that share a pass
constexpr int kQMaxQ = 64;          // quantiles per launch (kernel arguments)
constexpr int kQRowBytes = 64;      // one sample row of a tile
constexpr int kQLdsBytes = 160 * 1024;
constexpr int kQAhead = 4;          // rows requested before any is stored

struct QuantileParams {
  const void* in;
  const long long* slab;  // [n_outer][n_red] or null
  double* out;            // [n_q][n_outer][n_inner]
  long long n_outer, n_inner;
  int n_red, n_q, skipna;
  double q[kQMaxQ];
};

template <typename T>
constexpr int q_tile() { return kQRowBytes / (int)sizeof(T); }

// ---- shared device functions ----------------------------------------------
// One key against the candidates of a step.
template <typename K>
__device__ __forceinline__ void count_below(K k, K prefix, int shift,
                                            unsigned int (&cnt)[kQCand]) {
#pragma unroll
  for (int j = 0; j < kQCand; ++j)
    cnt[j] += k < (prefix | (K(j + 1) << shift)) ? 1u : 0u;
}

__device__ __forceinline__ int digit_of(const unsigned int (&cnt)[kQCand],
                                        int lo) {
  int d = 0;
#pragma unroll
  for (int j = 0; j < kQCand; ++j) d += cnt[j] <= (unsigned int)lo ? 1 : 0;
  return d;
}

// v = q (m - 1): lo = floor(v), hi = min(lo + 1, m - 1), t = v - lo.
__device__ __forceinline__ void rank_of(double q, int m, int& lo, int& hi,
                                        double& t) {
  const double v = q * (double)(m - 1);
  const double f = __builtin_floor(v);
  lo = (int)f;
  hi = lo + 1 < m ? lo + 1 : m - 1;
  t = v - f;
}

// NumPy's _lerp: the difference in T, the rest in float64, no contraction.
template <typename T>
__device__ __forceinline__ double interpolate(T a, T b, double t) {
  const T d = b - a;
  return t < 0.5 ? (double)a + (double)d * t
                 : (double)b - (double)d * (1.0 - t);
}

// s[hi] from the key of rank lo, the count of keys <= it and the key above.
template <typename T>
__device__ __forceinline__ double finish(typename QKey<T>::type key,
                                         unsigned int n_le,
                                         typename QKey<T>::type above, int lo,
                                         int hi, double t) {
  const T a = from_key<T>(key);
  const T b = (hi == lo || n_le > (unsigned int)lo + 1u) ? a
                                                         : from_key<T>(above);
  return interpolate<T>(a, b, t);
}

__device__ __forceinline__ double q_nan() { return __builtin_nan(""); }

// ---- resident regime ------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(kQResThreads)
    quantile_resident_kernel(const QuantileParams p) {
  typedef typename QKey<T>::type K;
  constexpr int P = q_tile<T>();
  constexpr int LPR = P / VEC;             // lanes per sample row
  constexpr int RPP = kQResThreads / LPR;  // rows per pass of the workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
  K* keys = reinterpret_cast<K*>(q_lds);  // [n_red][P]
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const long long i0 = (long long)blockIdx.x * P;
  const int valid = p.n_inner - i0 < P ? (int)(p.n_inner - i0) : P;
  const int n_red = p.n_red;
  const long long row = o * n_red;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  {
    const int c = (int)(threadIdx.x % LPR) * VEC;
    const T* in = static_cast<const T*>(p.in) + i0 + c;
    if (c < valid) {  // (a wide row holds whole vectors: n_inner % VEC == 0)
      for (int rb = threadIdx.x / LPR; rb < n_red; rb += RPP * kQAhead) {
        T v[kQAhead][VEC];
#pragma unroll
        for (int u = 0; u < kQAhead; ++u) {
          // (rows past the end are read from the last one and dropped)
          const int r = min(rb + u * RPP, n_red - 1);
          load_v<T, VEC>(in + (slab ? slab[r] : row + r) * p.n_inner, v[u]);
        }
#pragma unroll
        for (int u = 0; u < kQAhead; ++u) {
          const int r = rb + u * RPP;
          if (r < n_red) {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
              keys[(long long)r * P + c + e] = to_key<T>(v[u][e]);
          }
        }
      }
    }
  }
  __syncthreads();
  // a wave = S slices of the samples x P points, one quantile at a time: the
  // S lanes of a point add their counters up by lane exchange (they run the
  // same passes: everything that steers them is a reduced value)
  constexpr int S = kWave / P;
  constexpr int n_wave = kQResThreads / kWave;
  const int lane = threadIdx.x % kWave;
  const int wave = threadIdx.x / kWave;
  const int pt = lane % P;
  const int sl = lane / P;
  if (pt >= valid || wave >= p.n_q) return;
  const K* col = keys + sl * P + pt;  // sample r = sl + k S at col[k S P]
  const int n_mine = (n_red - sl + S - 1) / S;
  unsigned int n_nan = 0;
  K kmin = ~K(0), kmax = 0;
#pragma unroll 8
  for (int k = 0; k < n_mine; ++k) {
    const K key = col[k * (S * P)];
    if (key == ~K(0)) {
      ++n_nan;
    } else {
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
    }
  }
  n_nan = slices_sum<P>(n_nan);
  kmin = slices_min<P, K>(kmin);
  kmax = slices_max<P, K>(kmax);
  const int m = p.skipna ? n_red - (int)n_nan : n_red;
  const bool none = m == 0 || (!p.skipna && n_nan != 0);
  const int start = none ? 0 : first_shift<K>(kmin, kmax);
  double* out = p.out + o * p.n_inner + i0 + pt;
  const long long q_stride = p.n_outer * p.n_inner;
  for (int jq = wave; jq < p.n_q; jq += n_wave) {
    double res = q_nan();
    if (!none) {
      int lo, hi;
      double t;
      rank_of(p.q[jq], m, lo, hi, t);
      K prefix = prefix_above<K>(kmax, start);
      for (int shift = start - kQBits; shift >= 0; shift -= kQBits) {
        unsigned int cnt[kQCand] = {};
#pragma unroll 8
        for (int k = 0; k < n_mine; ++k)
          count_below<K>(col[k * (S * P)], prefix, shift, cnt);
#pragma unroll
        for (int j = 0; j < kQCand; ++j) cnt[j] = slices_sum<P>(cnt[j]);
        prefix |= (K)digit_of(cnt, lo) << shift;
      }
      unsigned int n_le = 0;
      K above = ~K(0);
      if (hi != lo) {
#pragma unroll 8
        for (int k = 0; k < n_mine; ++k) {
          const K key = col[k * (S * P)];
          n_le += key <= prefix ? 1u : 0u;
          above = (key > prefix && key < above) ? key : above;
        }
        n_le = slices_sum<P>(n_le);
        above = slices_min<P, K>(above);
      }
      res = finish<T>(prefix, n_le, above, lo, hi, t);
    }
    if (sl == 0) out[jq * q_stride] = res;
  }
}

// ---- streaming regime -----------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kQStrThreads)
    quantile_stream_kernel(const QuantileParams p) {
  typedef typename QKey<T>::type K;
  constexpr int P = q_tile<T>();
  constexpr int S = kQStrThreads / P;  // slices of the sample axis
  __shared__ unsigned int s_cnt[P][kQTargets * kQCand];
  __shared__ unsigned int s_nan[P];
  __shared__ K s_lo[P], s_hi[P];
  __shared__ K s_above[P][kQTargets];
  __shared__ int s_start;
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const long long i0 = (long long)blockIdx.x * P;
  const int valid = p.n_inner - i0 < P ? (int)(p.n_inner - i0) : P;
  const int n_red = p.n_red;
  const long long row = o * n_red;
  const long long* slab = p.slab ? p.slab + row : nullptr;
  const int pt = threadIdx.x % P;
  const int sl = threadIdx.x / P;
  const bool live = pt < valid;
  const bool head = sl == 0;  // the lane that speaks for its point
  const T* in = static_cast<const T*>(p.in) + i0 + pt;
  auto key_at = [&](int r) -> K {
    return to_key<T>(in[(slab ? slab[r] : row + r) * p.n_inner]);
  };
  if (head) {
    s_nan[pt] = 0;
    s_lo[pt] = ~K(0);
    s_hi[pt] = 0;
  }
  if (threadIdx.x == 0) s_start = 0;
  __syncthreads();
  if (live) {
    unsigned int n_nan = 0;
    K kmin = ~K(0), kmax = 0;
#pragma unroll 4
    for (int r = sl; r < n_red; r += S) {
      const K k = key_at(r);
      if (k == ~K(0)) {
        ++n_nan;
      } else {
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    }
    atomicAdd(&s_nan[pt], n_nan);
    atomicMin(&s_lo[pt], kmin);
    atomicMax(&s_hi[pt], kmax);
  }
  __syncthreads();
  const unsigned int n_nan = s_nan[pt];
  const int m = p.skipna ? n_red - (int)n_nan : n_red;
  const bool none = !live || m == 0 || (!p.skipna && n_nan != 0);
  const K kmax = s_hi[pt];
  // one step count for the whole workgroup (the barriers below): the largest
  // any of its points needs; a higher start is a shorter common prefix
  if (head && !none) atomicMax(&s_start, first_shift<K>(s_lo[pt], kmax));
  __syncthreads();
  const int start = s_start;
  double* out = p.out + o * p.n_inner + i0 + pt;
  const long long q_stride = p.n_outer * p.n_inner;
  for (int g = 0; g < p.n_q; g += kQTargets) {
    int lo[kQTargets], hi[kQTargets];
    double t[kQTargets];
    K prefix[kQTargets];
#pragma unroll
    for (int j = 0; j < kQTargets; ++j) {
      lo[j] = hi[j] = 0;
      t[j] = 0.0;
      if (!none && g + j < p.n_q) rank_of(p.q[g + j], m, lo[j], hi[j], t[j]);
      prefix[j] = prefix_above<K>(kmax, start);
    }
    for (int shift = start - kQBits; shift >= 0; shift -= kQBits) {
      if (head) {
#pragma unroll
        for (int c = 0; c < kQTargets * kQCand; ++c) s_cnt[pt][c] = 0;
      }
      __syncthreads();
      if (!none) {
        unsigned int cnt[kQTargets][kQCand] = {};
#pragma unroll 4
        for (int r = sl; r < n_red; r += S) {
          const K k = key_at(r);
#pragma unroll
          for (int j = 0; j < kQTargets; ++j)
            count_below<K>(k, prefix[j], shift, cnt[j]);
        }
#pragma unroll
        for (int j = 0; j < kQTargets; ++j) {
#pragma unroll
          for (int c = 0; c < kQCand; ++c)
            atomicAdd(&s_cnt[pt][j * kQCand + c], cnt[j][c]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kQTargets; ++j) {
        unsigned int cnt[kQCand];
#pragma unroll
        for (int c = 0; c < kQCand; ++c) cnt[c] = s_cnt[pt][j * kQCand + c];
        prefix[j] |= (K)digit_of(cnt, lo[j]) << shift;
      }
      __syncthreads();
    }
    if (head) {
#pragma unroll
      for (int j = 0; j < kQTargets; ++j) {
        s_cnt[pt][j] = 0;
        s_above[pt][j] = ~K(0);
      }
    }
    __syncthreads();
    if (!none) {
      unsigned int n_le[kQTargets] = {};
      K above[kQTargets];
#pragma unroll
      for (int j = 0; j < kQTargets; ++j) above[j] = ~K(0);
#pragma unroll 4
      for (int r = sl; r < n_red; r += S) {
        const K k = key_at(r);
#pragma unroll
        for (int j = 0; j < kQTargets; ++j) {
          n_le[j] += k <= prefix[j] ? 1u : 0u;
          above[j] = (k > prefix[j] && k < above[j]) ? k : above[j];
        }
      }
#pragma unroll
      for (int j = 0; j < kQTargets; ++j) {
        atomicAdd(&s_cnt[pt][j], n_le[j]);
        atomicMin(&s_above[pt][j], above[j]);
      }
    }
    __syncthreads();
    if (head && live) {
#pragma unroll
      for (int j = 0; j < kQTargets; ++j) {
        if (g + j < p.n_q)
          out[(g + j) * q_stride] =
              none ? q_nan()
                   : finish<T>(prefix[j], s_cnt[pt][j], s_above[pt][j], lo[j],
                               hi[j], t[j]);
      }
    }
    __syncthreads();
  }
}

template <typename F>
hipError_t allow_lds(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             kQLdsBytes);
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_quantile_geometry(int dtype, int wide, int32_t* tile_points,
                          int64_t* max_resident, int32_t* targets_per_pass,
                          int32_t* key_bits_per_pass) {
  using namespace wb2;
  (void)wide;  // wide loads change the staging of a tile, not its extent
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && max_resident && targets_per_pass &&
                  key_bits_per_pass,
              "null pointer argument");
  *tile_points = dtype == WB2_F32 ? q_tile<float>() : q_tile<double>();
  *max_resident = kQLdsBytes / kQRowBytes;
  *targets_per_pass = kQTargets;
  *key_bits_per_pass = kQBits;
  return 0;
}

int wb2_quantile_select(int dtype, int skipna, const void* in,
                        const int64_t* slab, int64_t n_outer, int64_t n_red,
                        int64_t n_inner, const double* q, int32_t n_q,
                        double* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_outer >= 1 && n_red >= 1 && n_inner >= 1 && n_q >= 1,
              "bad sizes: n_outer=%lld n_red=%lld n_inner=%lld n_q=%d",
              (long long)n_outer, (long long)n_red, (long long)n_inner,
              (int)n_q);
  WB2_REQUIRE(in && out && q, "null pointer argument");
  for (int32_t j = 0; j < n_q; ++j)
    WB2_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0,
                "quantile %d = %g is not in [0, 1]", (int)j, q[j]);
  const int tile = dtype == WB2_F32 ? q_tile<float>() : q_tile<double>();
  const long long gx = (n_inner + tile - 1) / tile;
  dim3 grid;
  WB2_REQUIRE(n_red < (1ll << 31) && outer_grid(n_outer, gx, &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool resident = n_red <= kQLdsBytes / kQRowBytes;
  const bool wide = n_inner % wide_lanes(dtype) == 0 && aligned16(in);
  if (resident) {
    static const hipError_t allowed = [] {
      hipError_t e = allow_lds(quantile_resident_kernel<float, 4>);
      if (e == hipSuccess) e = allow_lds(quantile_resident_kernel<float, 1>);
      if (e == hipSuccess) e = allow_lds(quantile_resident_kernel<double, 2>);
      if (e == hipSuccess) e = allow_lds(quantile_resident_kernel<double, 1>);
      return e;
    }();
    WB2_HIP_OK(allowed);
  }
  QuantileParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.n_outer = n_outer;
  p.n_inner = n_inner;
  p.n_red = (int)n_red;
  p.skipna = skipna;
  const size_t lds = (size_t)n_red * kQRowBytes;
  // (more quantiles than the kernel arguments hold: one launch per group)
  for (int32_t j0 = 0; j0 < n_q; j0 += kQMaxQ) {
    p.n_q = n_q - j0 < kQMaxQ ? n_q - j0 : kQMaxQ;
    for (int j = 0; j < p.n_q; ++j) p.q[j] = q[j0 + j];
    p.out = out + (long long)j0 * n_outer * n_inner;
    for_field(dtype, wide, [&](auto t, auto v) {
      using T = decltype(t);
      constexpr int V = decltype(v)::value;
      if (resident)
        hipLaunchKernelGGL((quantile_resident_kernel<T, V>), grid,
                           dim3(kQResThreads), lds, s, p);
      else
        hipLaunchKernelGGL((quantile_stream_kernel<T>), grid,
                           dim3(kQStrThreads), 0, s, p);
    });
    WB2_HIP_OK(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
