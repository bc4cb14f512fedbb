// K26 of libwb2hip.so: the joint frequency table of forecast and truth
// categories (Murphy & Winkler 1987), the sufficient statistic of the
// multi-category scores (proportion correct, Heidke, Peirce, Gerrity), of both
// marginal histograms and of the calibration-refinement and likelihood-base-
// rate factorisations.  The reference has no counterpart.
//
//   wb2_joint_counts  cnt[o][i][c][code]: over the columns j of class c in row
//                     i of outer index o, code = bin(y) * B + bin(x_m) gets +1
//                     PER MEMBER of a valid point, code = B * B +1 per invalid
//                     point; B = n_edge + 1, n_code = B * B + 1
//
// bin(v) = #{k : edge_k <= v} (side 0, searchsorted side='right') or #{k :
// edge_k < v} (side 1, 'left'), IEEE comparisons in float64 after an exact
// widening; +-inf are ordinary values.  The point is invalid iff the truth or
// any member is NaN (K18's rule).  The fold is K18's (wb2_event_fold with
// n_code = B * B + 1): the kernel adds integers only.
//
// Counting: a workgroup of 256 threads owns rows_per_group adjacent rows of one
// outer index -- one contiguous run of every slab -- and walks it with 16-byte
// lanes (or one element per access), as K18 does.  The edges are wave-uniform:
// each is read ONCE per workgroup with a uniform load and stays in a register;
// the ones past n_edge are NaN, which no value is at or above.  side 1 is
// turned into side 0 there: for a finite edge e, e < v holds exactly where
// succ(e) <= v does (succ = the next float64 up), whatever v is.
// A point's validity is known only after its last member, so nothing reaches
// the histogram before: per point a thread keeps, for every edge k, the number
// of members at or above it (g_k <= M <= 128: packed 8-bit counters, four to a
// register, every index a compile-time constant).  The edges increase, so the
// members of category b number g_{b-1} - g_b (g_{-1} = M, g_B = 0); the
// non-zero ones are added to the LDS histogram [row][class][code] with
// workgroup-scope integer atomics.  After a barrier the histogram goes to
// memory with plain stores.  Integer adds commute: two runs are bit-equal.  No
// global atomics, no float atomics.  Members and truth are read ONCE: (M + 1)
// elements per point.

#include <cstdint>

#include "common.hpp"
#include "event_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kJointThreads = 256;
constexpr int kJointRows = 4;     // rows of one workgroup, at most
constexpr long long kJointLds = 64 * 1024;  // K18's budget of histogram bytes
constexpr int kJointMaxEdge = 31;
constexpr char kJointTakes[] = "the joint table takes";

struct JointParams {
  const void* ens;
  const void* truth;
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const int* col_class;         // [n_col]
  const double* edges;          // [n_edge], finite and increasing
  int* cnt;                     // [n_outer][n_row][n_class][n_code]
  long long member_stride, n_outer;
  int n_member, n_row, n_col, n_class, n_edge, side, rows_per_group;
};

// The next float64 above a finite e (both zeros: the least subnormal).
__device__ __forceinline__ double joint_succ(double e) {
  const long long b = __builtin_bit_cast(long long, e);
  if (e == 0.0) return __builtin_bit_cast(double, 1ll);
  return __builtin_bit_cast(double, b >= 0 ? b + 1 : b - 1);
}

// One value against the NE edges: +1 in the packed counter of every edge it
// is at or above.
template <int NE>
__device__ __forceinline__ void joint_member(const double (&edge)[NE], double x,
                                             unsigned (&ge)[(NE + 3) / 4]) {
#pragma unroll
  for (int k = 0; k < NE; ++k)
    ge[k / 4] += edge[k] <= x ? 1u << (8 * (k % 4)) : 0u;
}

template <typename T, int VEC, int NE>
__global__ void __launch_bounds__(kJointThreads)
    joint_counts_kernel(const JointParams p) {
  extern __shared__ int hist[];  // [rows_per_group][n_class][n_code]
  constexpr int NW = (NE + 3) / 4;
  const long long o = outer_index();
  if (o >= p.n_outer) return;  // (the whole workgroup)
  const int M = p.n_member;
  const int B = p.n_edge + 1;
  const int n_code = B * B + 1;
  const int row0 = (int)blockIdx.x * p.rows_per_group;
  const int nrow = p.n_row - row0 < p.rows_per_group ? p.n_row - row0
                                                     : p.rows_per_group;
  const int row_bins = p.n_class * n_code;
  for (int i = threadIdx.x; i < p.rows_per_group * row_bins; i += kJointThreads)
    hist[i] = 0;

  // the edges: uniform loads, once; NaN past n_edge
  double edge[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    edge[k] = __builtin_nan("");
    if (k < p.n_edge) {
      const double e = p.edges[k];
      edge[k] = p.side ? joint_succ(e) : e;
    }
  }
  __syncthreads();

  // (once per workgroup: the element loop below loads no table)
  const long long slab = (long long)p.n_row * p.n_col;
  const long long first = (long long)row0 * p.n_col;
  const T* xb = exceed_slab<T>(p.ens, p.ens_slab, o, slab, first);
  const T* tb = exceed_slab<T>(p.truth, p.truth_slab, o, slab, first);
  const int n_elem = nrow * p.n_col;  // (the host checked that it fits)
  for (int e = (int)threadIdx.x * VEC; e < n_elem; e += kJointThreads * VEC) {
    T tv[VEC];
    load_v<T, VEC>(tb + e, tv);
    unsigned ge[VEC][NW];
    bool bad[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      bad[v] = false;
#pragma unroll
      for (int w = 0; w < NW; ++w) ge[v][w] = 0u;
    }
    // the members are requested kExceedAhead at a time, all before any is
    // compared, then the tail
    const T* xe = xb + e;
    int m = 0;
    for (; m + kExceedAhead <= M; m += kExceedAhead) {
      T x[kExceedAhead][VEC];
#pragma unroll
      for (int u = 0; u < kExceedAhead; ++u)
        load_v<T, VEC>(xe + (m + u) * p.member_stride, x[u]);
#pragma unroll
      for (int u = 0; u < kExceedAhead; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          bad[v] = bad[v] || is_nan(x[u][v]);
          joint_member<NE>(edge, (double)x[u][v], ge[v]);
        }
    }
    for (; m < M; ++m) {
      T x[VEC];
      load_v<T, VEC>(xe + m * p.member_stride, x);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        bad[v] = bad[v] || is_nan(x[v]);
        joint_member<NE>(edge, (double)x[v], ge[v]);
      }
    }
    // (VEC divides n_col on the wide path: a lane never spans two rows)
    const int r = e / p.n_col;
    const int c = e - r * p.n_col;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      int* h = hist + r * row_bins + p.col_class[c + v] * n_code;
      if (bad[v] || is_nan(tv[v])) {
        __hip_atomic_fetch_add(h + B * B, 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        continue;
      }
      const double y = (double)tv[v];
      int yb = 0;
#pragma unroll
      for (int k = 0; k < NE; ++k) yb += edge[k] <= y ? 1 : 0;
      int* hy = h + yb * B;
      // category b holds the members at or above edge b - 1 and not edge b
      // (a category past B - 1 holds none: its edges are NaN)
      int above = M;
#pragma unroll
      for (int b = 0; b <= NE; ++b) {
        const int next = b < NE ? (int)((ge[v][b / 4] >> (8 * (b % 4))) & 0xffu)
                                : 0;
        const int n = above - next;
        if (n != 0)
          __hip_atomic_fetch_add(hy + b, n, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        above = next;
      }
    }
  }
  __syncthreads();
  const int n_out = nrow * row_bins;
  int* dst = p.cnt + (o * p.n_row + row0) * (long long)row_bins;
  for (int i = threadIdx.x; i < n_out; i += kJointThreads) dst[i] = hist[i];
}

struct JointGeometry {
  int rows_per_group;
  long long lds_bytes;
};

// The most of 4, 2, 1 rows whose histogram fits the budget.  False: not even
// one row fits.
inline bool joint_geometry(int n_class, int n_edge, JointGeometry* g) {
  const long long n_bin = n_edge + 1;
  const long long row_bytes = 4ll * n_class * (n_bin * n_bin + 1);
  for (int rows = kJointRows; rows >= 1; rows /= 2)
    if (rows * row_bytes <= kJointLds) {
      *g = {rows, rows * row_bytes};
      return true;
    }
  return false;
}

// The checks of the geometry query, which the counting call makes first too.
inline int joint_shape(int dtype, int n_member, int n_class, int n_edge,
                       JointGeometry* g) {
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_member >= 1 && n_member <= kExceedMaxMember,
              "n_member=%d: %s 1 to %d members", n_member, kJointTakes,
              kExceedMaxMember);
  WB2_REQUIRE(n_class >= 1 && n_class <= kExceedMaxClass,
              "n_class=%d: %s 1 to %d column classes", n_class, kJointTakes,
              kExceedMaxClass);
  WB2_REQUIRE(n_edge >= 0 && n_edge <= kJointMaxEdge,
              "n_edge=%d: %s 0 to %d bin edges", n_edge, kJointTakes,
              kJointMaxEdge);
  WB2_REQUIRE(joint_geometry(n_class, n_edge, g),
              "the histogram of %d classes x %d codes does not fit the LDS "
              "budget of %lld bytes", n_class, (n_edge + 1) * (n_edge + 1) + 1,
              kJointLds);
  return 0;
}

// f(T{}, integral_constant<VEC>{}, integral_constant<NE>{}): for_field() and
// the least instantiated edge count that holds n_edge.
template <class F>
void for_joint(int dtype, bool wide, int n_edge, F&& f) {
  for_field(dtype, wide, [&](auto T0, auto V) {
    if (n_edge <= 4) f(T0, V, std::integral_constant<int, 4>{});
    else if (n_edge <= 8) f(T0, V, std::integral_constant<int, 8>{});
    else if (n_edge <= 12) f(T0, V, std::integral_constant<int, 12>{});
    else if (n_edge <= 16) f(T0, V, std::integral_constant<int, 16>{});
    else if (n_edge <= 24) f(T0, V, std::integral_constant<int, 24>{});
    else f(T0, V, std::integral_constant<int, 32>{});
  });
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_joint_counts_geometry(int dtype, int32_t n_member, int32_t n_class,
                              int32_t n_edge, int wide,
                              int32_t* rows_per_group, int64_t* lds_bytes,
                              int32_t* max_edges, int32_t* max_grid_outer) {
  using namespace wb2;
  (void)wide;  // the lane width changes neither the rows nor the histogram
  JointGeometry g;
  if (const int rc = joint_shape(dtype, n_member, n_class, n_edge, &g))
    return rc;
  WB2_REQUIRE(rows_per_group && lds_bytes && max_edges && max_grid_outer,
              "null pointer argument");
  *rows_per_group = g.rows_per_group;
  *lds_bytes = g.lds_bytes;
  *max_edges = kJointMaxEdge;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_joint_counts(int dtype, const void* ens, const int64_t* ens_slab,
                     const void* truth, const int64_t* truth_slab,
                     int32_t n_member, int64_t member_stride, int64_t n_outer,
                     int32_t n_row, int32_t n_col, const int32_t* col_class,
                     int32_t n_class, const double* edges, int32_t n_edge,
                     int side, int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  JointGeometry g;
  if (const int rc = joint_shape(dtype, n_member, n_class, n_edge, &g))
    return rc;
  WB2_REQUIRE(side == 0 || side == 1, "side=%d: %s 0 (right: an edge belongs "
              "to the upper category) or 1 (left)", side, kJointTakes);
  JointParams p{};
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, &p);
  if (go <= 0) return go;
  WB2_REQUIRE(col_class && cnt && (edges || n_edge == 0),
              "null pointer argument");
  // (the walk over a row group counts in int, one stride past its end)
  WB2_REQUIRE((long long)g.rows_per_group * n_col < (1ll << 30),
              "n_col=%d: a group of %d rows is too long", (int)n_col,
              g.rows_per_group);
  const int w = wide_lanes(dtype);
  const bool wide = all_aligned16(ens, truth) && n_col % w == 0 &&
                    member_stride % w == 0;
  p.col_class = col_class;
  p.edges = edges;
  p.cnt = cnt;
  p.n_row = n_row;
  p.n_col = n_col;
  p.n_class = n_class;
  p.n_edge = n_edge;
  p.side = side;
  p.rows_per_group = g.rows_per_group;
  const long long groups = (n_row + g.rows_per_group - 1) / g.rows_per_group;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_outer, groups, &grid),
              "the grid does not fit: %lld outer indices of %lld row groups",
              (long long)n_outer, groups);
  for_joint(dtype, wide, n_edge, [&](auto T0, auto V, auto NE) {
    hipLaunchKernelGGL(
        (joint_counts_kernel<decltype(T0), decltype(V)::value,
                             decltype(NE)::value>),
        grid, dim3(kJointThreads), (size_t)g.lds_bytes,
        static_cast<hipStream_t>(stream), p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
