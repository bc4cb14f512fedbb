// K15 of libwb2hip.so: weighted quantiles and SEEPS thresholds over the
// rolling day-of-year window (scripts/compute_climatology.py:130-216 through
// weatherbench2/utils.py:88-124 with a callable stat_fn).
//
//   wb2_window_quantile  for every (outer, cycle, position a, point): the
//                        weighted quantiles of the window's samples and,
//                        optionally, the fraction of them below a threshold
//
// The samples of position a are X[y, (a + k) mod n_pos], k = -H .. H, of K14's
// groups (the fill applied), sample (k, y) with the integer weight m[k + H].
// The reference's weights are proportional to m = H - |k| and xarray's
// weighted quantile normalises them, so with M = S m and Q = S m^2 over the
// samples kept (not NaN, not dry, m > 0), all exact integers:
//   n = M M / Q (Kish's effective sample size),  h = (n - 1) q + 1,
//   A = (h - 1) / n M,  B = h / n M,
//   result = n / M * S_v v |[C<(v), C<=(v)] ^ [A, B]|
// over the distinct values v, C<(v) and C<=(v) the weight below and up to v:
// n times the integral of the step function "sorted value over cumulative
// weight" over [A, B].  Equal values need no order.  The values the interval
// touches are found by selection, nothing is sorted: kA is the smallest value
// with C<= > A, kB the smallest with C<= >= B (K12's counting passes with
// weights as increments, both targets in one pass), and one last pass takes
// C<=(kA), C<(kB) and the sum of x m strictly between them in float64:
//   kA == kB:  s = kA (B - A)
//   else       s = (kA (C<=(kA) - A) + mid) + kB (B - C<(kB))
//   result = n / M * s, NaN where M == 0.
// The dry fraction is (number of window samples below the threshold, weight
// zero included, NaN not) / denominator.
//
// A workgroup owns (outer, cycle, tile of P adjacent points, block of D
// consecutive positions).  It stages the D + n_w - 1 cyclic positions' member
// rows into LDS once, as keys [slot][year][P], short groups padded: a NaN or
// absent sample is the all-ones key, a dry one the key below it (a NaN bit
// pattern no value maps to), so that "kept" is one compare.  The window of
// position d is then the contiguous run of n_w * n_year rows from slot d, and
// an LDS table gives the weight of every row of a window.  A wave serves one
// (position, quantile) at a time; its lanes are 64 / P slices of the window's
// samples x P points that add their integer counters up by lane exchange.
// Every trip count comes from the arguments, no wave waits on another after
// the staging barrier, there are no atomics, and every sum has a fixed order.

#include <cmath>

#include "common.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kWqThreads = 256;
constexpr int kWqMaxQ = 64;         // quantiles per launch (kernel arguments)
constexpr int kWqMaxW = 511;        // window weights (kernel arguments)
constexpr int kWqRowBytes = 64;     // the widest sample row of a tile
constexpr int kWqLdsBytes = 160 * 1024;
constexpr int kWqMinD = 4;   // positions a tile wider than one point must hold
constexpr int kWqMaxD = 32;  // positions per workgroup

struct WindowParams {
  const void* in;
  const long long* slab;   // [n_outer][n_time] or null
  const int* group_begin;  // [n_cycle * n_pos + 1]
  const int* member;       // [n_member]
  const int* fill;         // [n_member] or null
  double* quant;           // [n_q][n_outer][n_group][n_point]
  double* dry;             // [n_outer][n_group][n_point] or null
  long long n_outer, n_point, n_tile;
  int n_time, n_cycle, n_pos, n_member, n_w, n_q, n_year, n_d, n_block;
  int use_dry, denominator;
  double dry_threshold;
  double q[kWqMaxQ];
  int m[kWqMaxW];
};

template <typename K>
__device__ __forceinline__ void weight_below(K k, unsigned int w, K prefix,
                                             int shift,
                                             unsigned int (&cnt)[kQCand]) {
#pragma unroll
  for (int j = 0; j < kQCand; ++j)
    cnt[j] += k < (prefix | (K(j + 1) << shift)) ? w : 0u;
}

__device__ __forceinline__ int digit_at(const unsigned int (&cnt)[kQCand],
                                        unsigned int target) {
  int d = 0;
#pragma unroll
  for (int j = 0; j < kQCand; ++j) d += cnt[j] <= target ? 1 : 0;
  return d;
}

template <typename T, int P>
__global__ void __launch_bounds__(kWqThreads)
    window_quantile_kernel(const WindowParams p) {
  typedef typename QKey<T>::type K;
  constexpr K kNanKey = ~K(0);
  constexpr K kDryKey = ~K(0) - 1;
  constexpr int S = kWave / P;
  constexpr int n_wave = kWqThreads / kWave;
  extern __shared__ __attribute__((aligned(16))) unsigned char wq_lds[];
  const long long o = outer_index();
  if (o >= p.n_outer) return;
  const long long tile = blockIdx.x % p.n_tile;
  const int rest = (int)(blockIdx.x / p.n_tile);
  const int blk = rest % p.n_block;
  const int c = rest / p.n_block;
  const int Y = p.n_year;
  const int half = p.n_w / 2;
  const int a0 = blk * p.n_d;
  const int n_slot = p.n_d + p.n_w - 1;
  const int n_win = p.n_w * Y;  // rows of one window
  K* keys = reinterpret_cast<K*>(wq_lds);  // [n_slot][Y][P]
  int* wrow = reinterpret_cast<int*>(wq_lds +
                                     (size_t)n_slot * Y * P * sizeof(K));
  const long long i0 = tile * P;
  const int valid = p.n_point - i0 < P ? (int)(p.n_point - i0) : P;
  {
    const long long row = o * p.n_time;
    const long long* slab = p.slab ? p.slab + row : nullptr;
    const T* in = static_cast<const T*>(p.in) + i0;
    const T thr = (T)p.dry_threshold;
    const int total = n_slot * Y * P;
    for (int e = threadIdx.x; e < total; e += kWqThreads) {
      const int pt = e % P;
      const int ry = e / P;
      const int s = ry / Y;
      const int y = ry - s * Y;
      int pos = (a0 - half + s) % p.n_pos;
      pos += pos < 0 ? p.n_pos : 0;
      K key = kNanKey;
      if (pt < valid) {
        const int g = c * p.n_pos + pos;
        // (a list that does not fit the members is cut to them)
        const int begin = max(0, min(p.group_begin[g], p.n_member));
        const int end = max(begin, min(p.group_begin[g + 1], p.n_member));
        const int j = begin + y;
        if (j < end) {
          const int t = p.member[j];
          const int f = p.fill ? p.fill[j] : -1;
          T x = quiet_nan<T>();
          if (t >= 0 && t < p.n_time)
            x = in[(slab ? slab[t] : row + t) * p.n_point + pt];
          if (is_nan(x) && f >= 0 && f < p.n_time)
            x = in[(slab ? slab[f] : row + f) * p.n_point + pt];
          key = is_nan(x) ? kNanKey
                          : (p.use_dry && x < thr) ? kDryKey : to_key<T>(x);
        }
      }
      keys[e] = key;
    }
    for (int i = threadIdx.x; i < n_win; i += kWqThreads) wrow[i] = p.m[i / Y];
  }
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int wave = threadIdx.x / kWave;
  const int pt = lane % P;
  const int sl = lane / P;
  const int n_mine = n_win > sl ? (n_win - sl + S - 1) / S : 0;
  const int n_group = p.n_cycle * p.n_pos;
  const int n_task = p.n_d * p.n_q;
  const long long q_stride = p.n_outer * n_group * p.n_point;
  for (int task = wave; task < n_task; task += n_wave) {
    const int d = task / p.n_q;
    const int jq = task - d * p.n_q;
    const int a = a0 + d;
    if (a >= p.n_pos) continue;  // (the same for the whole wave)
    // row i = sl + k S of the window lies at col[k S P], its weight at wv[k S]
    const K* col = keys + ((long long)d * Y + sl) * P + pt;
    const int* wv = wrow + sl;
    unsigned int wsum = 0, wsq = 0, n_dry = 0;
    K kmin = kNanKey, kmax = 0;
#pragma unroll 4
    for (int k = 0; k < n_mine; ++k) {
      const K key = col[k * (S * P)];
      const unsigned int w = (unsigned int)wv[k * S];
      const bool kept = key < kDryKey;
      const unsigned int wk = kept ? w : 0u;
      wsum += wk;
      wsq += wk * w;
      n_dry += key == kDryKey ? 1u : 0u;
      kmin = (kept && key < kmin) ? key : kmin;
      kmax = (kept && key > kmax) ? key : kmax;
    }
    wsum = slices_sum<P>(wsum);
    wsq = slices_sum<P>(wsq);
    n_dry = slices_sum<P>(n_dry);
    kmin = slices_min<P, K>(kmin);
    kmax = slices_max<P, K>(kmax);
    double res = __builtin_nan("");
    if (wsum != 0) {  // (the same for the lanes of a point)
      const double M = (double)wsum, Q = (double)wsq;
      const double n = M * M / Q;
      const double h = (n - 1.0) * p.q[jq] + 1.0;
      double A = (h - 1.0) / n * M;
      double B = h / n * M;
      A = A < 0.0 ? 0.0 : A;
      B = B > M ? M : B;
      const double fa = __builtin_floor(A), cb = __builtin_ceil(B);
      unsigned int ta = (unsigned int)fa;
      unsigned int tb = cb < 1.0 ? 0u : (unsigned int)cb - 1u;
      ta = ta > wsum - 1u ? wsum - 1u : ta;
      tb = tb > wsum - 1u ? wsum - 1u : tb;
      tb = tb < ta ? ta : tb;
      const int start = first_shift<K>(kmin, kmax);
      K pa = prefix_above<K>(kmax, start), pb = pa;
      for (int shift = start - kQBits; shift >= 0; shift -= kQBits) {
        unsigned int ca[kQCand] = {}, cb2[kQCand] = {};
#pragma unroll 4
        for (int k = 0; k < n_mine; ++k) {
          const K key = col[k * (S * P)];
          const unsigned int w = (unsigned int)wv[k * S];
          weight_below<K>(key, w, pa, shift, ca);
          weight_below<K>(key, w, pb, shift, cb2);
        }
#pragma unroll
        for (int j = 0; j < kQCand; ++j) {
          ca[j] = slices_sum<P>(ca[j]);
          cb2[j] = slices_sum<P>(cb2[j]);
        }
        pa |= (K)digit_at(ca, ta) << shift;
        pb |= (K)digit_at(cb2, tb) << shift;
      }
      unsigned int le_a = 0, lt_b = 0;
      double mid = 0.0;
#pragma unroll 4
      for (int k = 0; k < n_mine; ++k) {
        const K key = col[k * (S * P)];
        const unsigned int w = (unsigned int)wv[k * S];
        le_a += key <= pa ? w : 0u;
        lt_b += key < pb ? w : 0u;
        if (key > pa && key < pb && w != 0u)
          mid += (double)from_key<T>(key) * (double)w;
      }
      le_a = slices_sum<P>(le_a);
      lt_b = slices_sum<P>(lt_b);
      mid = slices_sum<P>(mid);
      const double xa = (double)from_key<T>(pa);
      const double xb = (double)from_key<T>(pb);
      const double s = pa == pb ? xa * (B - A)
                                : (xa * ((double)le_a - A) + mid) +
                                      xb * (B - (double)lt_b);
      res = n / M * s;
    }
    if (sl == 0 && pt < valid) {
      const long long at = ((long long)o * n_group + (long long)c * p.n_pos +
                            a) * p.n_point + i0 + pt;
      p.quant[jq * q_stride + at] = res;
      if (p.dry && jq == 0)
        p.dry[at] = (double)n_dry / (double)p.denominator;
    }
  }
}

// The widest tile whose staging holds kWqMinD positions (one point: any), and
// the positions of a workgroup; false if even one position of one point does
// not fit.
bool window_geometry(int dtype, long long n_year, int n_w, int* tile,
                     int* positions, long long* lds) {
  const int size = dtype == WB2_F32 ? 4 : 8;
  n_year = n_year < 1 ? 1 : n_year;
  const long long table = (long long)n_w * n_year * 4;
  for (int pw = kWqRowBytes / size; pw >= 1; pw /= 2) {
    const long long slot = n_year * pw * size;
    const long long slots = (kWqLdsBytes - table) / slot;
    const long long fit = slots - (n_w - 1);
    if (table < kWqLdsBytes && fit >= (pw > 1 ? kWqMinD : 1)) {
      *tile = pw;
      *positions = (int)(fit < kWqMaxD ? fit : kWqMaxD);
      *lds = (*positions + n_w - 1) * slot + table;
      return true;
    }
  }
  return false;
}

template <typename F>
hipError_t allow_window_lds(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             kWqLdsBytes);
}

template <typename T, int P>
hipError_t launch_window(dim3 grid, size_t lds, hipStream_t s,
                         const WindowParams& p) {
  static const hipError_t allowed =
      allow_window_lds(window_quantile_kernel<T, P>);
  if (allowed != hipSuccess) return allowed;
  hipLaunchKernelGGL((window_quantile_kernel<T, P>), grid, dim3(kWqThreads),
                     lds, s, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_window_quantile_geometry(int dtype, int64_t n_year, int32_t n_w,
                                 int32_t* tile_points, int32_t* positions,
                                 int64_t* lds_bytes,
                                 int32_t* key_bits_per_pass) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && positions && lds_bytes && key_bits_per_pass,
              "null pointer argument");
  WB2_REQUIRE(n_year >= 0 && n_w > 0 && n_w % 2 == 1 && n_w <= kWqMaxW,
              "bad sizes: n_year=%lld, n_w=%d (odd, at most %d)",
              (long long)n_year, (int)n_w, kWqMaxW);
  int tile = 0, pos = 0;
  long long lds = 0;
  WB2_REQUIRE(window_geometry(dtype, n_year, n_w, &tile, &pos, &lds),
              "a window of %d x %lld samples does not fit the LDS", (int)n_w,
              (long long)n_year);
  *tile_points = tile;
  *positions = pos;
  *lds_bytes = lds;
  *key_bits_per_pass = kQBits;
  return 0;
}

int wb2_window_quantile(int dtype, const void* in, const int64_t* slab,
                        int64_t n_outer, int32_t n_time, int64_t n_point,
                        const int32_t* group_begin,
                        const int32_t* group_begin_host, int32_t n_cycle,
                        int32_t n_pos, const int32_t* member,
                        const int32_t* fill, int32_t n_member,
                        const int32_t* weights, int32_t n_w, int use_dry,
                        double dry_threshold, int32_t denominator,
                        const double* q, int32_t n_q, double* quantile,
                        double* dry_fraction, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_time >= 0 && n_member >= 0,
              "bad sizes: n_time=%d or n_member=%d is negative", (int)n_time,
              (int)n_member);
  WB2_REQUIRE(n_w > 0 && n_w % 2 == 1 && n_w <= kWqMaxW,
              "the window must have an odd, positive number of weights, at "
              "most %d: n_w=%d", kWqMaxW, (int)n_w);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_cycle);
  WB2_EMPTY_OK(n_pos);
  WB2_EMPTY_OK(n_point);
  WB2_EMPTY_OK(n_q);
  const long long n_group = (long long)n_cycle * n_pos;
  WB2_REQUIRE(n_group < (1ll << 31), "bad sizes");
  WB2_REQUIRE(group_begin && group_begin_host && weights && q && quantile,
              "null pointer argument");
  WB2_REQUIRE((in || n_time == 0) && (member || n_member == 0),
              "null pointer argument");
  WB2_REQUIRE(!dry_fraction || (use_dry && denominator > 0),
              "the dry fraction needs a dry threshold and a positive "
              "denominator: %d", (int)denominator);
  WB2_REQUIRE(group_begin_host[0] == 0 && group_begin_host[n_group] == n_member,
              "group_begin does not fit the members: it runs from %d to %d, "
              "n_member=%d", (int)group_begin_host[0],
              (int)group_begin_host[n_group], (int)n_member);
  long long n_year = 0;
  for (long long g = 0; g < n_group; ++g) {
    WB2_REQUIRE(group_begin_host[g] <= group_begin_host[g + 1],
                "group_begin does not fit the members: it decreases at group "
                "%lld", g);
    const long long size = group_begin_host[g + 1] - group_begin_host[g];
    n_year = size > n_year ? size : n_year;
  }
  long long wsum = 0, wsq = 0;
  for (int32_t k = 0; k < n_w; ++k) {
    WB2_REQUIRE(weights[k] >= 0, "weight %d = %d is negative", (int)k,
                (int)weights[k]);
    wsum += weights[k];
    wsq += (long long)weights[k] * weights[k];
  }
  n_year = n_year < 1 ? 1 : n_year;
  WB2_REQUIRE(wsum * n_year <= 0x7fffffffll && wsq * n_year <= 0x7fffffffll,
              "the weights of a window (%lld years) exceed the integer "
              "counters", n_year);
  for (int32_t j = 0; j < n_q; ++j)
    WB2_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0,
                "quantile %d = %g is not in [0, 1]", (int)j, q[j]);
  int tile = 0, pos = 0;
  long long lds = 0;
  WB2_REQUIRE(window_geometry(dtype, n_year, n_w, &tile, &pos, &lds),
              "a window of %d x %lld samples does not fit the LDS", (int)n_w,
              n_year);
  WindowParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.group_begin = group_begin;
  p.member = member;
  p.fill = fill;
  p.n_outer = n_outer;
  p.n_point = n_point;
  p.n_tile = (n_point + tile - 1) / tile;
  p.n_time = n_time;
  p.n_cycle = n_cycle;
  p.n_pos = n_pos;
  p.n_member = n_member;
  p.n_w = n_w;
  p.n_year = (int)n_year;
  p.n_d = pos < n_pos ? pos : n_pos;
  p.n_block = (n_pos + p.n_d - 1) / p.n_d;
  p.use_dry = use_dry != 0;
  p.denominator = denominator;
  p.dry_threshold = dry_threshold;
  for (int32_t k = 0; k < n_w; ++k) p.m[k] = weights[k];
  const size_t bytes =
      (size_t)(p.n_d + n_w - 1) * n_year * tile * (dtype == WB2_F32 ? 4 : 8) +
      (size_t)n_w * n_year * 4;
  dim3 grid;
  WB2_REQUIRE(p.n_tile < (1ll << 31) &&
                  outer_grid(n_outer, p.n_tile * p.n_block * n_cycle, &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (more quantiles than the kernel arguments hold: one launch per group)
  for (int32_t j0 = 0; j0 < n_q; j0 += kWqMaxQ) {
    p.n_q = n_q - j0 < kWqMaxQ ? n_q - j0 : kWqMaxQ;
    for (int j = 0; j < p.n_q; ++j) p.q[j] = q[j0 + j];
    p.quant = quantile + (long long)j0 * n_outer * n_group * n_point;
    p.dry = j0 == 0 ? dry_fraction : nullptr;
    hipError_t e = hipSuccess;
    if (dtype == WB2_F32) {
      switch (tile) {
        case 16: e = launch_window<float, 16>(grid, bytes, s, p); break;
        case 8: e = launch_window<float, 8>(grid, bytes, s, p); break;
        case 4: e = launch_window<float, 4>(grid, bytes, s, p); break;
        case 2: e = launch_window<float, 2>(grid, bytes, s, p); break;
        default: e = launch_window<float, 1>(grid, bytes, s, p); break;
      }
    } else {
      switch (tile) {
        case 8: e = launch_window<double, 8>(grid, bytes, s, p); break;
        case 4: e = launch_window<double, 4>(grid, bytes, s, p); break;
        case 2: e = launch_window<double, 2>(grid, bytes, s, p); break;
        default: e = launch_window<double, 1>(grid, bytes, s, p); break;
      }
    }
    WB2_HIP_OK(e);
  }
  return 0;
}

}  // extern "C"
