// K22 of libwb2hip.so: box pooling of (latitude, longitude) slabs, the mean or
// the maximum over an odd window n = 2 h + 1 in grid points ("upscaling",
// Ebert 2008; the pooled scores of Price et al. 2025).  The reference has no
// counterpart.
//
//   wb2_pool_fields  out[w][o][m][i][j] = the pool of window w around point
//                    (i, j) of member m of outer index o, in the input dtype
//
// The window of (i, j) is K19's: the rows r0 = max(0, i - h) .. r1 = min(n_row
// - 1, i + h) (clipped at the poles), the columns (j - h .. j + h) mod n_col
// (cyclic), N_i = n (r1 - r0 + 1) points.  Two passes in ONE fixed order:
//   mean  float64 after an exact widening.  H[r][j] = the sequential chain s =
//         s + x over the column offsets -h, ..., +h, started from the first
//         term; V[i][j] = the sequential chain of H[r][j] over r = r0 .. r1,
//         started from H[r0][j]; out = V / (double)N_i, rounded once to the
//         input dtype.  No fused multiply-add.  NaN and +-inf follow IEEE.
//   max   the input dtype, the same two passes with m = first; m = (v > m ||
//         v != v) ? v : m: a NaN propagates, the first zero met keeps its sign.
// Running or prefix sums round differently and are not used.
//
// A workgroup of 1024 threads owns one field and a tile of tile_rows x 64
// outputs.  It stages the tile and its halo for the LARGEST window of the
// launch in LDS once -- rows clipped, the column index wrapped --, then per
// window: every thread walks horizontal chains of staged rows into a second
// LDS tile (float64 for mean), the workgroup meets, every thread walks the
// vertical chains of its outputs and stores them.  Consecutive lanes hold
// consecutive columns in both passes: every LDS access of a wave is to
// consecutive addresses, free of bank conflicts.  Up to 4 windows share one
// staging.  Plain stores, no atomics: two runs are bit-equal.

#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kPoolThreads = 1024;
constexpr int kPoolCols = 64;      // tile_cols: one wave per tile row
constexpr int kPoolWin = 4;        // windows that share one staging
constexpr int kPoolMaxWindow = 255;
constexpr int kPoolMaxMember = 128;
constexpr long long kPoolLds = 160 * 1024;
constexpr int kPoolTileRows[] = {32, 16, 8};  // tried in this order

struct PoolParams {
  const void* in;
  void* out;                  // the first window of this launch
  const long long* in_slab;   // [n_outer] or null: slab o
  long long member_stride, n_field, slab;
  int n_member, n_row, n_col;
  int tile_rows, tiles_c;
  int nw, hmax;               // windows of this launch, their largest half
  int half[kPoolWin];
};

// the staging of one workgroup: the input tile with its halo, then the
// horizontal chains (8 bytes each, whatever the kind)
inline long long pool_stage_elems(int tile_rows, int hmax) {
  return (long long)(tile_rows + 2 * hmax) * (kPoolCols + 2 * hmax);
}
inline long long pool_lds_bytes(int dtype, int tile_rows, int hmax) {
  const long long esz = dtype == WB2_F32 ? 4 : 8;
  const long long stage = (pool_stage_elems(tile_rows, hmax) * esz + 7) / 8 * 8;
  return stage + (long long)(tile_rows + 2 * hmax) * kPoolCols * 8;
}

template <bool MEAN, typename A>
__device__ __forceinline__ A pool_step(A m, A v) {
  if constexpr (MEAN) return m + v;
  else return (v > m || v != v) ? v : m;
}

template <typename T, int VEC, bool MEAN>
__global__ void __launch_bounds__(kPoolThreads)
    pool_kernel(const PoolParams p) {
  extern __shared__ double pool_lds[];
  using A = std::conditional_t<MEAN, double, T>;
  const long long f = outer_index();
  if (f >= p.n_field) return;
  const int tid = threadIdx.x;
  const int tile_r = (int)blockIdx.x / p.tiles_c;
  const int tile_c = (int)blockIdx.x - tile_r * p.tiles_c;
  const int i0 = tile_r * p.tile_rows, j0 = tile_c * kPoolCols;
  const int rows = p.n_row - i0 < p.tile_rows ? p.n_row - i0 : p.tile_rows;
  const int cols = p.n_col - j0 < kPoolCols ? p.n_col - j0 : kPoolCols;
  const int hm = p.hmax;
  // the staged rows rs0 .. rs1, at most tile_rows + 2 hm of them
  const int rs0 = i0 - hm > 0 ? i0 - hm : 0;
  const int rs1 = i0 + rows - 1 + hm < p.n_row - 1 ? i0 + rows - 1 + hm
                                                   : p.n_row - 1;
  const int srows = rs1 - rs0 + 1;
  const int pitch = kPoolCols + 2 * hm;
  T* stage = reinterpret_cast<T*>(pool_lds);
  A* chain = reinterpret_cast<A*>(
      pool_lds + ((long long)(p.tile_rows + 2 * hm) * pitch * sizeof(T) + 7) / 8);

  const long long o = f / p.n_member;
  const long long m = f - o * p.n_member;
  const T* x = static_cast<const T*>(p.in) +
               (p.in_slab ? p.in_slab[o] : o) * p.slab + m * p.member_stride;

  // staged column c of a row is the column (j0 - hm + c) mod n_col; hm <
  // n_col, so one step brings it home
  auto wrapped = [&](int col) {
    return col < 0 ? col + p.n_col : col >= p.n_col ? col - p.n_col : col;
  };
  if constexpr (VEC == 1) {
    const int scols = cols + 2 * hm;
    for (int idx = tid; idx < srows * scols; idx += kPoolThreads) {
      const int r = idx / scols, c = idx - r * scols;
      stage[r * pitch + c] =
          x[(long long)(rs0 + r) * p.n_col + wrapped(j0 - hm + c)];
    }
  } else {
    // the tile's own columns start at a multiple of 64 in a row of a multiple
    // of VEC columns: 16-byte loads; the halo one element at a time
    const int vpr = cols / VEC;
    for (int idx = tid; idx < srows * vpr; idx += kPoolThreads) {
      const int r = idx / vpr, v = idx - r * vpr;
      T val[VEC];
      load_cached<T, VEC>(x + (long long)(rs0 + r) * p.n_col + j0 + v * VEC,
                          val);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        stage[r * pitch + hm + v * VEC + e] = val[e];
    }
    const int halo = 2 * hm;
    for (int idx = tid; idx < srows * halo; idx += kPoolThreads) {
      const int r = idx / halo, c = idx - r * halo;
      const int sc = c < hm ? c : c + cols;  // left of the tile, right of it
      stage[r * pitch + sc] =
          x[(long long)(rs0 + r) * p.n_col + wrapped(j0 - hm + sc)];
    }
  }
  __syncthreads();

  T* y = static_cast<T*>(p.out) + f * p.slab;
  for (int w = 0; w < p.nw; ++w) {
    const int h = p.half[w];
    const int n = 2 * h + 1;
    // horizontal chains of the rows this window reaches
    const int ra = i0 - h > 0 ? i0 - h : 0;
    const int rb = i0 + rows - 1 + h < p.n_row - 1 ? i0 + rows - 1 + h
                                                   : p.n_row - 1;
    for (int idx = tid; idx < (rb - ra + 1) * kPoolCols; idx += kPoolThreads) {
      const int r = ra - rs0 + (idx >> 6), jj = idx & (kPoolCols - 1);
      if (jj >= cols) continue;
      const T* src = stage + r * pitch + jj + hm - h;
      A s = (A)src[0];
      for (int k = 1; k < n; ++k) s = pool_step<MEAN, A>(s, (A)src[k]);
      chain[r * kPoolCols + jj] = s;
    }
    __syncthreads();
    // vertical chains of the tile's outputs
    constexpr int kGroups = kPoolCols / VEC;
    for (int idx = tid; idx < rows * kGroups; idx += kPoolThreads) {
      const int ii = idx / kGroups, jj = (idx - ii * kGroups) * VEC;
      if (jj >= cols) continue;
      const int i = i0 + ii;
      const int r0 = i - h > 0 ? i - h : 0;
      const int r1 = i + h < p.n_row - 1 ? i + h : p.n_row - 1;
      const A* src = chain + (r0 - rs0) * kPoolCols + jj;
      A v[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = src[e];
      for (int r = r0 + 1; r <= r1; ++r) {
        src += kPoolCols;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = pool_step<MEAN, A>(v[e], src[e]);
      }
      T res[VEC];
      if constexpr (MEAN) {
        const double cnt = (double)(n * (r1 - r0 + 1));
#pragma unroll
        for (int e = 0; e < VEC; ++e) res[e] = (T)(v[e] / cnt);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) res[e] = v[e];
      }
      store_v<T, VEC>(y + (long long)i * p.n_col + j0 + jj, res);
    }
    // (the next window overwrites the chains)
    __syncthreads();
    y += p.n_field * p.slab;
  }
}

struct PoolGeometry {
  int tile_rows, windows_per_launch, max_window;
  long long lds_bytes;
};

// The checks that need no operand, and the tile: the first of kPoolTileRows
// whose staging for the largest window of the call fits kPoolLds.  0 or
// fail()'s negative.
inline int pool_shape(int dtype, int n_col, const int32_t* windows,
                      int n_window, PoolGeometry* g) {
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_window >= 1, "n_window=%d", n_window);
  WB2_REQUIRE(n_col >= 0, "n_col=%lld is negative", (long long)n_col);
  WB2_REQUIRE(windows, "null pointer argument");
  constexpr int kSmallest =
      kPoolTileRows[sizeof(kPoolTileRows) / sizeof(int) - 1];
  int max_window = 1;
  for (int n = 3; n <= kPoolMaxWindow; n += 2)
    if (pool_lds_bytes(dtype, kSmallest, n / 2) <= kPoolLds) max_window = n;
  int top = 1;
  for (int w = 0; w < n_window; ++w) {
    const int n = windows[w];
    // (no column, no point: the no-op of the entry point)
    WB2_REQUIRE(n >= 1 && n <= kPoolMaxWindow && n % 2 == 1 &&
                    (n <= n_col || n_col == 0),
                "window=%d: a window is odd, 1 to %d and at most n_col=%d", n,
                kPoolMaxWindow, n_col);
    WB2_REQUIRE(n <= max_window,
                "window=%d: the halo of a window above max_window=%d does not "
                "fit the LDS", n, max_window);
    top = n > top ? n : top;
  }
  g->tile_rows = kSmallest;
  for (int tr : kPoolTileRows)
    if (pool_lds_bytes(dtype, tr, top / 2) <= kPoolLds) {
      g->tile_rows = tr;
      break;
    }
  g->windows_per_launch = n_window < kPoolWin ? n_window : kPoolWin;
  g->max_window = max_window;
  g->lds_bytes = pool_lds_bytes(dtype, g->tile_rows, top / 2);
  return 0;
}

template <class F>
hipError_t pool_allow_lds(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kPoolLds);
}

// f(kernel) for the instantiation of (dtype, wide, mean)
template <class F>
void for_pool(int dtype, bool wide, bool mean, F&& f) {
  for_field(dtype, wide, [&](auto T0, auto V) {
    using T = decltype(T0);
    constexpr int VEC = decltype(V)::value;
    if (mean) f(pool_kernel<T, VEC, true>);
    else f(pool_kernel<T, VEC, false>);
  });
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_pool_geometry(int dtype, int32_t n_col, const int32_t* windows,
                      int32_t n_window, int32_t* windows_per_launch,
                      int32_t* tile_rows, int32_t* tile_cols,
                      int64_t* lds_bytes, int32_t* max_window,
                      int32_t* max_grid_outer) {
  using namespace wb2;
  PoolGeometry g;
  if (const int rc = pool_shape(dtype, n_col, windows, n_window, &g)) return rc;
  WB2_REQUIRE(windows_per_launch && tile_rows && tile_cols && lds_bytes &&
              max_window && max_grid_outer, "null pointer argument");
  *windows_per_launch = g.windows_per_launch;
  *tile_rows = g.tile_rows;
  *tile_cols = kPoolCols;
  *lds_bytes = g.lds_bytes;
  *max_window = g.max_window;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_pool_fields(int dtype, const void* in, const int64_t* in_slab,
                    int32_t n_member, int64_t member_stride, int64_t n_outer,
                    int32_t n_row, int32_t n_col, const int32_t* windows,
                    int32_t n_window, int kind, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(kind == WB2_POOL_MEAN || kind == WB2_POOL_MAX,
              "kind=%d: the pooling takes 0 (mean) or 1 (max)", kind);
  WB2_REQUIRE(n_member >= 1 && n_member <= kPoolMaxMember,
              "n_member=%d: the pooling takes 1 to %d members", (int)n_member,
              kPoolMaxMember);
  WB2_REQUIRE(n_window >= 1, "n_window=%d", (int)n_window);
  WB2_REQUIRE(member_stride >= 0, "member_stride=%lld is negative",
              (long long)member_stride);
  WB2_REQUIRE(n_outer >= 0, "n_outer=%lld is negative", (long long)n_outer);
  WB2_REQUIRE(n_row >= 0, "n_row=%lld is negative", (long long)n_row);
  PoolGeometry g;
  if (const int rc = pool_shape(dtype, n_col, windows, n_window, &g)) return rc;
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_row);
  WB2_EMPTY_OK(n_col);
  WB2_REQUIRE(in && out, "null pointer argument");
  const long long n_field = (long long)n_outer * n_member;
  const int tiles_r = (n_row + g.tile_rows - 1) / g.tile_rows;
  const int tiles_c = (n_col + kPoolCols - 1) / kPoolCols;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_field, (long long)tiles_r * tiles_c, &grid),
              "the grid does not fit: %lld fields of %lld tiles", n_field,
              (long long)tiles_r * tiles_c);
  const int lanes = wide_lanes(dtype);
  const bool wide = all_aligned16(in, out) && n_col % lanes == 0 &&
                    member_stride % lanes == 0;
  const bool mean = kind == WB2_POOL_MEAN;
  if (g.lds_bytes > 64 * 1024) {
    // (once per PROCESS, as in quantile.hip: the attribute belongs to the
    // function of the device that is current at the first such call)
    static const hipError_t allowed = [] {
      hipError_t e = hipSuccess;
      for (int d : {WB2_F32, WB2_F64})
        for (bool w : {false, true})
          for (bool mn : {false, true})
            for_pool(d, w, mn, [&](auto kernel) {
              if (e == hipSuccess) e = pool_allow_lds(kernel);
            });
      return e;
    }();
    WB2_HIP_OK(allowed);
  }
  PoolParams p{};
  p.in = in;
  p.in_slab = reinterpret_cast<const long long*>(in_slab);
  p.member_stride = member_stride;
  p.n_field = n_field;
  p.slab = (long long)n_row * n_col;
  p.n_member = n_member;
  p.n_row = n_row;
  p.n_col = n_col;
  p.tile_rows = g.tile_rows;
  p.tiles_c = tiles_c;
  const long long esz = dtype == WB2_F32 ? 4 : 8;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // more windows than one staging serves: further launches, each staged for
  // its own largest window
  for (int w0 = 0; w0 < n_window; w0 += kPoolWin) {
    p.nw = n_window - w0 < kPoolWin ? n_window - w0 : kPoolWin;
    p.hmax = 0;
    for (int w = 0; w < kPoolWin; ++w) {
      p.half[w] = w < p.nw ? windows[w0 + w] / 2 : 0;
      p.hmax = p.half[w] > p.hmax ? p.half[w] : p.hmax;
    }
    p.out = static_cast<char*>(out) + (long long)w0 * n_field * p.slab * esz;
    const size_t lds = (size_t)pool_lds_bytes(dtype, g.tile_rows, p.hmax);
    for_pool(dtype, wide, mean, [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kPoolThreads), lds, s, p);
    });
    WB2_HIP_OK(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
