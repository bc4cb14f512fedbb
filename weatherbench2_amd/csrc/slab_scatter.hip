// K16 of libwb2hip.so: time re-indexing as a one-read slab scatter
// (scripts/expand_climatology.py, scripts/index_on_valid_time.py,
// scripts/compute_probabilistic_climatological_forecasts.py: a forecast-shaped
// dataset built by re-indexing whole slabs along time).
//
//   wb2_slab_scatter  every source slab is read once and stored, cast to the
//                     output dtype, to each of its destination slabs
//
// The table is a CSR over sources: source s is the n_point elements that start
// `src_slab[s] * n_point` after the input's base (K13's slab convention; -1 =
// read nothing, store quiet NaN) and goes to the output slabs
// dst_slab[dst_begin[s] .. dst_begin[s + 1]).  A thread owns VEC adjacent
// points, loads them before its first store and keeps them in registers; a
// workgroup owns one tile of points of one source and blocks of
// dests_per_group consecutive destinations of it.  The destination counts live
// on the device only, so the grid cannot be cut to them: it is (tiles x lanes)
// x sources, the workgroup of lane j takes the blocks j, j + lanes, ... and
// leaves before it loads anything if it has none.  One lane where sources x
// tiles fill the device by themselves (every workgroup then stores all the
// destinations of its source), more where they do not (a few sources with many
// destinations each).  Destinations are disjoint by contract, so there are no
// atomics and no LDS, and neither the lane count nor dests_per_group changes a
// bit.  Loads and stores stream (nontemporal): a source is read by one
// workgroup per lane and an output slab is written once.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kScatterThreads = 256;
// workgroups that keep every CU busy (256 CUs x 8 resident workgroups): below
// this many (source, tile) pairs the destination blocks are spread over lanes
constexpr long long kFillGroups = 2048;
constexpr long long kMaxLanes = 64;

struct ScatterParams {
  const void* in;
  const long long* src_slab;   // [n_source]
  const long long* dst_begin;  // [n_source + 1]
  const long long* dst_slab;   // [dst_begin[n_source]]
  void* out;
  long long n_source, n_point, n_tile;
  int n_lane, dests_per_group;
};

template <typename TI, typename TO, int VEC>
__global__ void __launch_bounds__(kScatterThreads)
    slab_scatter_kernel(const ScatterParams p) {
  const long long tile = blockIdx.x % p.n_tile;
  const long long lane = blockIdx.x / p.n_tile;
  const long long q = (tile * kScatterThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long s = outer_index();
  if (s >= p.n_source) return;
  const long long end = p.dst_begin[s + 1];
  const long long first = p.dst_begin[s] + lane * p.dests_per_group;
  if (first >= end) return;  // (no block for this lane: nothing is read)
  const long long src = p.src_slab[s];
  TO v[VEC];
  if (src < 0) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = quiet_nan<TO>();
  } else {
    TI x[VEC];
    load_v<TI, VEC>(static_cast<const TI*>(p.in) + src * p.n_point + q, x);
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = (TO)x[e];  // (round to nearest even)
  }
  TO* out = static_cast<TO*>(p.out) + q;
  const long long step = (long long)p.n_lane * p.dests_per_group;
  for (long long b = first; b < end; b += step) {
    const long long stop = min(b + p.dests_per_group, end);
    for (long long d = b; d < stop; ++d)
      store_v<TO, VEC>(out + p.dst_slab[d] * p.n_point, v);
  }
}

// points of a 16-byte lane of the pair: the wider of the two dtypes' lanes, so
// that the narrower side moves 16 bytes at once as well (f64 -> f32: two
// 16-byte loads, one 16-byte store)
inline int pair_lanes(int in_dtype, int out_dtype) {
  return in_dtype == WB2_F32 || out_dtype == WB2_F32 ? 4 : 2;
}

inline bool pair_supported(int in_dtype, int out_dtype) {
  return (in_dtype == WB2_F32 && out_dtype == WB2_F32) ||
         (in_dtype == WB2_F64 && (out_dtype == WB2_F64 || out_dtype == WB2_F32));
}

#define WB2_REQUIRE_PAIR(in_dtype, out_dtype)                                 \
  do {                                                                        \
    WB2_REQUIRE((in_dtype == WB2_F32 || in_dtype == WB2_F64) &&               \
                    (out_dtype == WB2_F32 || out_dtype == WB2_F64),           \
                "unknown dtype pair %d -> %d", in_dtype, out_dtype);          \
    WB2_REQUIRE(pair_supported(in_dtype, out_dtype),                          \
                "unsupported dtype pair %d -> %d (f32 -> f32, f64 -> f64 and " \
                "f64 -> f32 only)", in_dtype, out_dtype);                     \
  } while (0)

template <typename TI, typename TO, int W>
void launch_pair(bool wide, dim3 grid, hipStream_t s, const ScatterParams& p) {
  if (wide)
    hipLaunchKernelGGL((slab_scatter_kernel<TI, TO, W>), grid,
                       dim3(kScatterThreads), 0, s, p);
  else
    hipLaunchKernelGGL((slab_scatter_kernel<TI, TO, 1>), grid,
                       dim3(kScatterThreads), 0, s, p);
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_slab_scatter_geometry(int in_dtype, int out_dtype, int wide,
                              int32_t* tile_points, int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE_PAIR(in_dtype, out_dtype);
  WB2_REQUIRE(tile_points && max_grid_outer, "null pointer argument");
  *tile_points = kScatterThreads * (wide ? pair_lanes(in_dtype, out_dtype) : 1);
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_slab_scatter(int in_dtype, int out_dtype, const void* in,
                     const int64_t* src_slab, const int64_t* dst_begin,
                     const int64_t* dst_slab, int64_t n_source, int64_t n_point,
                     int32_t dests_per_group, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE_PAIR(in_dtype, out_dtype);
  WB2_REQUIRE(dests_per_group >= 1, "bad sizes: %d destinations per group",
              (int)dests_per_group);
  WB2_EMPTY_OK(n_source);
  WB2_EMPTY_OK(n_point);
  // (`in` may be null where every source is -1; the tables say so, not the
  // host, so it is required all the same)
  WB2_REQUIRE(in && src_slab && dst_begin && dst_slab && out,
              "null pointer argument");
  const int w = pair_lanes(in_dtype, out_dtype);
  const bool wide = n_point % w == 0 && all_aligned16(in, out);
  ScatterParams p{};
  p.in = in;
  p.src_slab = reinterpret_cast<const long long*>(src_slab);
  p.dst_begin = reinterpret_cast<const long long*>(dst_begin);
  p.dst_slab = reinterpret_cast<const long long*>(dst_slab);
  p.out = out;
  p.n_source = n_source;
  p.n_point = n_point;
  p.n_tile = point_tiles(n_point, wide ? w : 1, kScatterThreads);
  p.dests_per_group = dests_per_group;
  WB2_REQUIRE(p.n_tile < (1ll << 31), "bad sizes");
  const long long pairs =
      n_source < kFillGroups ? n_source * p.n_tile : kFillGroups;
  const long long lanes = (kFillGroups + pairs - 1) / pairs;
  p.n_lane = (int)(lanes < kMaxLanes ? lanes : kMaxLanes);
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_source, p.n_tile * p.n_lane, &grid), "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (in_dtype == WB2_F32)
    launch_pair<float, float, 4>(wide, grid, s, p);
  else if (out_dtype == WB2_F64)
    launch_pair<double, double, 2>(wide, grid, s, p);
  else
    launch_pair<double, float, 4>(wide, grid, s, p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
