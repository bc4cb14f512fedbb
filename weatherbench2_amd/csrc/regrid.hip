// K11 of libwb2hip.so: horizontal regridding (weatherbench2/regridding.py).
//
//   wb2_regrid_separable  ConservativeRegridder :502-536 (WB2_REGRID_NANMEAN)
//                         and BilinearRegridder :256-294 (WB2_REGRID_LINEAR)
//   wb2_regrid_gather     NearestRegridder :230-248
//
// The reference contracts every slab with two dense weight matrices.  The
// matrices are banded (at most 7 source cells per target cell and axis for
// 0.25 -> 1.5 degrees), so the work is one streaming read of the slab: the
// kernels are bound by input bytes and every source element should leave HBM
// about once.  The defined order of include/wb2hip.h (latitude sum inside,
// longitude sum outside, both in table order, float64, -ffp-contract=off)
// holds in both layouts, so the two workgroup kernels differ in which sum a
// thread can walk:
//
//   (lat, lon) slabs  one workgroup per (slab, target latitude).  A thread owns
//     VEC adjacent source longitudes and walks the latitude band of the target
//     row, kBand rows requested before any is combined; the per-longitude
//     partial sums go to LDS and the threads then own target longitudes and
//     sum their bands from LDS.  A source row on a band boundary is read by
//     two workgroups (the second time from L2: a slab is 4 MB): 1 row in 7 at
//     0.25 -> 1.5 degrees.
//   (lon, lat) slabs  one workgroup per (slab, target longitude, 256 target
//     latitudes).  The latitude sum runs along the contiguous axis, so the
//     meridians of the longitude band are staged in LDS as they are, kBand at
//     a time, and a thread owns one target latitude: it walks its latitude
//     band once per piece, the staged meridians side by side.
//
// The band entries of the LDS phases differ per thread (vector loads from the
// tables), so kBand of them are requested before any is used as well.
//
// 13 levels of 1440 x 721 -> 240 x 121 are 1573 workgroups ((lat, lon)) or
// 3120 ((lon, lat)); -> 64 x 32: 416 or 832: more than the 256 CUs.  A
// contiguous axis too long for the LDS of either takes the kernel of one
// thread per target cell: the same values, every band re-read from cache.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kRegridThreads = 256;
constexpr int kBand = 8;               // band entries requested before combining
constexpr int kRegridLds = 64 * 1024;  // bytes of LDS a workgroup may ask for

struct RegridParams {
  const void* in;
  const long long* slab;  // [n_slab] or null
  void* out;
  long long n_slab;
  int n_src_lon, n_src_lat, n_tgt_lon, n_tgt_lat;
  const int* lon_ptr;
  const int* lon_idx;
  const double* lon_w;
  const unsigned char* lon_nan;
  const int* lat_ptr;
  const int* lat_idx;
  const double* lat_w;
  const unsigned char* lat_nan;
};

__device__ __forceinline__ double regrid_nan() { return __builtin_nan(""); }

// a target node on a source node takes the node's value
__device__ __forceinline__ double lerp(double f0, double f1, double t) {
  return t == 0.0 ? f0 : f0 + t * (f1 - f0);
}

// one term of the NaN-skipping sums: s += w * value, n += w * (value present)
template <typename T>
__device__ __forceinline__ void nan_term(T x, double w, double& s, double& n) {
  const bool missing = x != x;
  s = s + w * (missing ? 0.0 : (double)x);
  n = n + w * (missing ? 0.0 : 1.0);
}

// (lat, lon) slabs: see the head of this file.  LDS: double[2][n_src_lon].
template <typename T, int VEC, int MODE>
__global__ void __launch_bounds__(kRegridThreads)
    regrid_rows_kernel(const RegridParams p) {
  extern __shared__ __align__(16) double regrid_lds[];
  const long long o = outer_index();
  if (o >= p.n_slab) return;
  constexpr bool MEAN = MODE == WB2_REGRID_NANMEAN;
  const int c = blockIdx.x;
  const int n_lon = p.n_src_lon;
  T* out = static_cast<T*>(p.out) + (o * p.n_tgt_lat + c) * (long long)p.n_tgt_lon;
  if (p.lat_nan[c]) {  // (the whole workgroup)
    for (int a = threadIdx.x; a < p.n_tgt_lon; a += kRegridThreads)
      out[a] = (T)regrid_nan();
    return;
  }
  const T* in = static_cast<const T*>(p.in) +
                (p.slab ? p.slab[o] : o) * (long long)p.n_src_lat * n_lon;
  double* tot = regrid_lds;
  double* cnt = regrid_lds + n_lon;
  const int k0 = p.lat_ptr[c], k1 = p.lat_ptr[c + 1];
  for (int b0 = threadIdx.x * VEC; b0 < n_lon; b0 += kRegridThreads * VEC) {
    double s[VEC], n[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = n[e] = 0.0;
    if (MEAN) {
      for (int k = k0; k < k1; k += kBand) {
        T v[kBand][VEC];
#pragma unroll
        for (int j = 0; j < kBand; ++j) {
          // (entries past the band are read from its last one and dropped)
          const int kk = min(k + j, k1 - 1);
          load_cached<T, VEC>(in + (long long)p.lat_idx[kk] * n_lon + b0, v[j]);
        }
#pragma unroll
        for (int j = 0; j < kBand; ++j) {
          if (k + j < k1) {
            const double w = p.lat_w[k + j];
#pragma unroll
            for (int e = 0; e < VEC; ++e) nan_term(v[j][e], w, s[e], n[e]);
          }
        }
      }
    } else {
      T f0[VEC], f1[VEC];
      load_cached<T, VEC>(in + (long long)p.lat_idx[k0] * n_lon + b0, f0);
      load_cached<T, VEC>(in + (long long)p.lat_idx[k0 + 1] * n_lon + b0, f1);
      const double t = p.lat_w[k0];
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] = lerp((double)f0[e], (double)f1[e], t);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      tot[b0 + e] = s[e];
      if (MEAN) cnt[b0 + e] = n[e];
    }
  }
  __syncthreads();
  for (int a = threadIdx.x; a < p.n_tgt_lon; a += kRegridThreads) {
    double r;
    const int q0 = p.lon_ptr[a], q1 = p.lon_ptr[a + 1];
    if (p.lon_nan[a]) {
      r = regrid_nan();
    } else if (MEAN) {
      double t = 0.0, m = 0.0;
      for (int q = q0; q < q1; q += kBand) {
        // (the entries differ per thread: all requested before any is used)
        int b[kBand];
        double w[kBand];
#pragma unroll
        for (int i = 0; i < kBand; ++i) {
          const int qq = min(q + i, q1 - 1);
          b[i] = p.lon_idx[qq];
          w[i] = p.lon_w[qq];
        }
#pragma unroll
        for (int i = 0; i < kBand; ++i) {
          if (q + i < q1) {
            t = t + w[i] * tot[b[i]];
            m = m + w[i] * cnt[b[i]];
          }
        }
      }
      r = t / m;
    } else {
      r = lerp(tot[p.lon_idx[q0]], tot[p.lon_idx[q0 + 1]], p.lon_w[q0]);
    }
    out[a] = (T)r;
  }
}

// (lon, lat) slabs: see the head of this file.  LDS: T[kBand][n_src_lat].
template <typename T, int VEC, int MODE>
__global__ void __launch_bounds__(kRegridThreads)
    regrid_cols_kernel(const RegridParams p, const int n_ctile) {
  extern __shared__ __align__(16) unsigned char regrid_lds_raw[];
  T* rows = reinterpret_cast<T*>(regrid_lds_raw);
  const long long o = outer_index();
  if (o >= p.n_slab) return;
  constexpr bool MEAN = MODE == WB2_REGRID_NANMEAN;
  const int a = blockIdx.x / n_ctile;
  const int c = (blockIdx.x % n_ctile) * kRegridThreads + threadIdx.x;
  const int n_lat = p.n_src_lat;
  const bool mine = c < p.n_tgt_lat;
  T* out = static_cast<T*>(p.out) + (o * p.n_tgt_lon + a) * (long long)p.n_tgt_lat;
  if (p.lon_nan[a]) {  // (the whole workgroup)
    if (mine) out[c] = (T)regrid_nan();
    return;
  }
  const T* in = static_cast<const T*>(p.in) +
                (p.slab ? p.slab[o] : o) * (long long)p.n_src_lon * n_lat;
  const bool live = mine && !p.lat_nan[c];
  const int q0 = live ? p.lat_ptr[c] : 0, q1 = live ? p.lat_ptr[c + 1] : 0;
  const int k0 = p.lon_ptr[a], k1 = p.lon_ptr[a + 1];
  double t = 0.0, m = 0.0, g0 = 0.0, g1 = 0.0;
  for (int k = k0; k < k1; k += kBand) {
    const int nb = min(kBand, k1 - k);
    if (k > k0) __syncthreads();  // the last piece has been read
    for (int d0 = threadIdx.x * VEC; d0 < n_lat; d0 += kRegridThreads * VEC) {
      T v[kBand][VEC];
#pragma unroll
      for (int j = 0; j < kBand; ++j) {
        const int kk = min(k + j, k1 - 1);
        load_cached<T, VEC>(in + (long long)p.lon_idx[kk] * n_lat + d0, v[j]);
      }
#pragma unroll
      for (int j = 0; j < kBand; ++j) {
        if (j < nb) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) rows[(long long)j * n_lat + d0 + e] = v[j][e];
        }
      }
    }
    __syncthreads();
    if (live && MEAN) {
      // the latitude sums of the nb meridians side by side: every table entry
      // (they differ per thread) is read once per piece, each sum still runs
      // in table order
      double s[kBand], n[kBand];
#pragma unroll
      for (int j = 0; j < kBand; ++j) s[j] = n[j] = 0.0;
      for (int q = q0; q < q1; q += kBand) {
        int d[kBand];
        double w[kBand];
#pragma unroll
        for (int i = 0; i < kBand; ++i) {
          const int qq = min(q + i, q1 - 1);
          d[i] = p.lat_idx[qq];
          w[i] = p.lat_w[qq];
        }
#pragma unroll
        for (int i = 0; i < kBand; ++i) {
          if (q + i < q1) {
#pragma unroll
            for (int j = 0; j < kBand; ++j)
              if (j < nb) nan_term(rows[(long long)j * n_lat + d[i]], w[i], s[j], n[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kBand; ++j) {
        if (j < nb) {
          const double w = p.lon_w[k + j];
          t = t + w * s[j];
          m = m + w * n[j];
        }
      }
    } else if (live) {
      const int i0 = p.lat_idx[q0], i1 = p.lat_idx[q0 + 1];
      const double u = p.lat_w[q0];
      g0 = lerp((double)rows[i0], (double)rows[i1], u);
      g1 = lerp((double)rows[(long long)n_lat + i0],
                (double)rows[(long long)n_lat + i1], u);
    }
  }
  if (!mine) return;
  double r = regrid_nan();
  if (live) r = MEAN ? t / m : lerp(g0, g1, p.lon_w[k0]);
  out[c] = (T)r;
}

// Any extents, either layout: one thread per target cell re-reads its bands
// (from cache, mostly).  The same order, the same values; correct, not fast.
template <typename T, int MODE>
__global__ void __launch_bounds__(kRegridThreads)
    regrid_cell_kernel(const RegridParams p, const int lat_rows) {
  const long long o = outer_index();
  if (o >= p.n_slab) return;
  constexpr bool MEAN = MODE == WB2_REGRID_NANMEAN;
  const long long n_tgt = (long long)p.n_tgt_lon * p.n_tgt_lat;
  const long long cell = (long long)blockIdx.x * kRegridThreads + threadIdx.x;
  if (cell >= n_tgt) return;
  const int a = lat_rows ? cell % p.n_tgt_lon : cell / p.n_tgt_lat;
  const int c = lat_rows ? cell / p.n_tgt_lon : cell % p.n_tgt_lat;
  const long long sb = lat_rows ? 1 : p.n_src_lat;  // stride of a longitude
  const long long sd = lat_rows ? p.n_src_lon : 1;  // stride of a latitude
  const T* in = static_cast<const T*>(p.in) +
                (p.slab ? p.slab[o] : o) * (long long)p.n_src_lon * p.n_src_lat;
  double r = regrid_nan();
  if (!p.lon_nan[a] && !p.lat_nan[c]) {
    const int k0 = p.lon_ptr[a], k1 = p.lon_ptr[a + 1];
    const int q0 = p.lat_ptr[c], q1 = p.lat_ptr[c + 1];
    if (MEAN) {
      double t = 0.0, m = 0.0;
      for (int k = k0; k < k1; ++k) {
        const T* col = in + p.lon_idx[k] * sb;
        double s = 0.0, n = 0.0;
        for (int q = q0; q < q1; ++q)
          nan_term(col[p.lat_idx[q] * sd], p.lat_w[q], s, n);
        const double w = p.lon_w[k];
        t = t + w * s;
        m = m + w * n;
      }
      r = t / m;
    } else {
      const long long d0 = p.lat_idx[q0] * sd, d1 = p.lat_idx[q0 + 1] * sd;
      const double u = p.lat_w[q0];
      const T* col0 = in + p.lon_idx[k0] * sb;
      const T* col1 = in + p.lon_idx[k0 + 1] * sb;
      r = lerp(lerp((double)col0[d0], (double)col0[d1], u),
               lerp((double)col1[d0], (double)col1[d1], u), p.lon_w[k0]);
    }
  }
  static_cast<T*>(p.out)[o * n_tgt + cell] = (T)r;
}

template <typename U>
__global__ void __launch_bounds__(kRegridThreads)
    regrid_gather_kernel(const U* in, const long long* slab, long long n_slab,
                         long long n_src, const int* index, long long n_tgt,
                         U* out) {
  const long long o = outer_index();
  const long long j = (long long)blockIdx.x * kRegridThreads + threadIdx.x;
  if (o >= n_slab || j >= n_tgt) return;
  out[o * n_tgt + j] = in[(slab ? slab[o] : o) * n_src + index[j]];
}

int regrid_max_contig(int dtype, int lat_rows) {
  const int elem = dtype == WB2_F32 ? 4 : 8;
  return lat_rows ? kRegridLds / (2 * (int)sizeof(double))
                  : kRegridLds / (kBand * elem);
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_regrid_geometry(int dtype, int lat_rows, int wide, int32_t* tile_elems,
                        int32_t* run_targets, int32_t* band_ahead,
                        int32_t* max_contig, int32_t* grid_slabs) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_elems && run_targets && band_ahead && max_contig &&
              grid_slabs, "null pointer argument");
  *tile_elems = kRegridThreads * (wide ? wide_lanes(dtype) : 1);
  *run_targets = 1;
  *band_ahead = kBand;
  *max_contig = regrid_max_contig(dtype, lat_rows);
  *grid_slabs = (int32_t)kGridOuter;
  return 0;
}

int wb2_regrid_separable(int mode, int dtype, int lat_rows, const void* in,
                         const int64_t* slab, int64_t n_slab,
                         int32_t n_src_lon, int32_t n_src_lat,
                         int32_t n_tgt_lon, int32_t n_tgt_lat,
                         const int32_t* lon_ptr, const int32_t* lon_idx,
                         const double* lon_w, const uint8_t* lon_nan,
                         const int32_t* lat_ptr, const int32_t* lat_idx,
                         const double* lat_w, const uint8_t* lat_nan,
                         void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(mode == WB2_REGRID_NANMEAN || mode == WB2_REGRID_LINEAR,
              "unknown mode %d", mode);
  WB2_EMPTY_OK(n_slab);
  WB2_EMPTY_OK(n_tgt_lon);
  WB2_EMPTY_OK(n_tgt_lat);
  WB2_REQUIRE(n_src_lon >= 1 && n_src_lat >= 1,
              "bad sizes: a source grid of %d x %d", (int)n_src_lon,
              (int)n_src_lat);
  WB2_REQUIRE(in && out && lon_ptr && lon_nan && lat_ptr && lat_nan,
              "null pointer argument");
  // (idx and w are empty, and may be null, where every index is uncovered)
  const long long n_tgt = (long long)n_tgt_lon * n_tgt_lat;
  WB2_REQUIRE(n_slab <= kGridOuter * 65535 &&
              (n_tgt + kRegridThreads - 1) / kRegridThreads < (1ll << 31),
              "bad sizes");
  RegridParams p{};
  p.in = in;
  p.slab = reinterpret_cast<const long long*>(slab);
  p.out = out;
  p.n_slab = n_slab;
  p.n_src_lon = n_src_lon;
  p.n_src_lat = n_src_lat;
  p.n_tgt_lon = n_tgt_lon;
  p.n_tgt_lat = n_tgt_lat;
  p.lon_ptr = lon_ptr;
  p.lon_idx = lon_idx;
  p.lon_w = lon_w;
  p.lon_nan = lon_nan;
  p.lat_ptr = lat_ptr;
  p.lat_idx = lat_idx;
  p.lat_w = lat_w;
  p.lat_nan = lat_nan;
  const int elem = dtype == WB2_F32 ? 4 : 8;
  const int n_contig = lat_rows ? n_src_lon : n_src_lat;
  const bool wide = n_contig % wide_lanes(dtype) == 0 && aligned16(in);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kRegridThreads);
  dim3 grid;
  if (n_contig > regrid_max_contig(dtype, lat_rows)) {
    WB2_REQUIRE(outer_grid(n_slab, point_tiles(n_tgt, 1, kRegridThreads),
                           &grid),
                "bad sizes");
    for_field(dtype, false, [&](auto t, auto) {
      using T = decltype(t);
      if (mode == WB2_REGRID_NANMEAN)
        hipLaunchKernelGGL((regrid_cell_kernel<T, WB2_REGRID_NANMEAN>), grid,
                           block, 0, s, p, lat_rows);
      else
        hipLaunchKernelGGL((regrid_cell_kernel<T, WB2_REGRID_LINEAR>), grid,
                           block, 0, s, p, lat_rows);
    });
  } else if (lat_rows) {
    WB2_REQUIRE(outer_grid(n_slab, n_tgt_lat, &grid), "bad sizes");
    const size_t lds = 2 * sizeof(double) * (size_t)n_src_lon;
    for_field(dtype, wide, [&](auto t, auto v) {
      using T = decltype(t);
      constexpr int V = decltype(v)::value;
      if (mode == WB2_REGRID_NANMEAN)
        hipLaunchKernelGGL((regrid_rows_kernel<T, V, WB2_REGRID_NANMEAN>),
                           grid, block, lds, s, p);
      else
        hipLaunchKernelGGL((regrid_rows_kernel<T, V, WB2_REGRID_LINEAR>),
                           grid, block, lds, s, p);
    });
  } else {
    const int n_ctile = (int)point_tiles(n_tgt_lat, 1, kRegridThreads);
    WB2_REQUIRE(outer_grid(n_slab, (long long)n_tgt_lon * n_ctile, &grid),
                "bad sizes");
    const size_t lds = (size_t)kBand * elem * (size_t)n_src_lat;
    for_field(dtype, wide, [&](auto t, auto v) {
      using T = decltype(t);
      constexpr int V = decltype(v)::value;
      if (mode == WB2_REGRID_NANMEAN)
        hipLaunchKernelGGL((regrid_cols_kernel<T, V, WB2_REGRID_NANMEAN>),
                           grid, block, lds, s, p, n_ctile);
      else
        hipLaunchKernelGGL((regrid_cols_kernel<T, V, WB2_REGRID_LINEAR>),
                           grid, block, lds, s, p, n_ctile);
    });
  }
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_regrid_gather(int elem_size, const void* in, const int64_t* slab,
                      int64_t n_slab, int64_t n_src, const int32_t* index,
                      int64_t n_tgt, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(elem_size == 1 || elem_size == 2 || elem_size == 4 ||
              elem_size == 8, "bad sizes: elements of %d bytes", elem_size);
  WB2_EMPTY_OK(n_slab);
  WB2_EMPTY_OK(n_tgt);
  WB2_REQUIRE(n_src >= 1 && n_src < (1ll << 31),
              "bad sizes: a source slab of %lld elements", (long long)n_src);
  WB2_REQUIRE(in && out && index, "null pointer argument");
  WB2_REQUIRE(n_slab <= kGridOuter * 65535 &&
              (n_tgt + kRegridThreads - 1) / kRegridThreads < (1ll << 31),
              "bad sizes");
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_slab, point_tiles(n_tgt, 1, kRegridThreads), &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long* table = reinterpret_cast<const long long*>(slab);
#define WB2_G(U)                                                              \
  hipLaunchKernelGGL((regrid_gather_kernel<U>), grid, dim3(kRegridThreads), 0, \
                     s, static_cast<const U*>(in), table, (long long)n_slab,  \
                     (long long)n_src, index, (long long)n_tgt,               \
                     static_cast<U*>(out))
  switch (elem_size) {
    case 1: WB2_G(uint8_t); break;
    case 2: WB2_G(uint16_t); break;
    case 4: WB2_G(uint32_t); break;
    default: WB2_G(uint64_t);
  }
#undef WB2_G
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
