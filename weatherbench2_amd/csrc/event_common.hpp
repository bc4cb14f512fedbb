// The exceedance layer under K18 (event_table.hip) and K19 (neighborhood.hip):
// the per-point compare both front ends rest on, stated once.
//
// For one point under threshold t: k = members with x > thr (IEEE: a NaN
// threshold exceeds nothing, equality is not exceedance), obs = truth > thr,
// the point is invalid iff the truth or any member is NaN.  Member m of outer
// index o is the slab that starts ens_slab[o] slabs and m * member_stride
// ELEMENTS after `ens`; truth_slab and thr_slab[t] address the truth and
// threshold t likewise (null = identity).  Up to kExceedThr thresholds share
// one read of the members, which are requested kExceedAhead at a time.
//
// Device: exceed_slab() resolves one slab of an outer index, reading its table
// once; a kernel requests the truth and the thresholds of its points from
// those, and exceed_points() turns them and the members into (k, obs, bad).
// What a kernel does with those -- K18 counts them, K19 stores them -- is all
// that is its own.  Host: the checks, the wide decision, the threshold batches
// and the NT dispatch that the two entry points share.
// The class-sums kernels (class_sums.hpp: K20, K21, K24) address their members
// and truth likewise: exceed_slab() and member_operands() serve them too.
#pragma once

#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "wb2hip.h"

namespace wb2 {

constexpr int kExceedThr = 4;     // thresholds that share one read
constexpr int kExceedAhead = 4;   // members requested before any is compared
constexpr int kExceedMaxMember = 128;
constexpr int kExceedMaxClass = 64;

// What both parameter structs start with.
struct ExceedOperands {
  const void* ens;
  const void* truth;
  const void* thr[kExceedThr];  // the thresholds of this launch
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const long long* thr_slab[kExceedThr];  // each [n_outer] or null
  long long member_stride, n_outer;
  int n_member;
};

// The slab of outer index o, `first` elements in: one test of the table
// pointer, one read of the table.  (It takes the fields, not the parameter
// struct: a kernel whose parameter struct goes to a function by reference
// loads ALL of it at its entry, and holds the scalar registers for that.)
template <typename T>
__device__ __forceinline__ const T* exceed_slab(
    const void* x, const long long* table, long long o, long long slab_elems,
    long long first) {
  return static_cast<const T*>(x) + (table ? table[o] : o) * slab_elems + first;
}

// VEC adjacent points: `tv` and `hv` are their truth and thresholds, which the
// kernel has requested already (each right after it resolved that slab, so
// that the loads of one are in flight while the next is resolved), `xe` is
// member 0.  The M members are requested kExceedAhead at a time, all before
// any is compared, then the tail.  (The counts are kept in locals and handed
// over at the end: the compiler then treats them as it did when the loop
// stood in the kernels.)
template <typename T, int VEC, int NT>
__device__ __forceinline__ void exceed_points(
    const T* xe, long long member_stride, int M, const T (&tv)[VEC],
    const T (&hv)[NT][VEC], int (&k)[NT][VEC], bool (&obs)[NT][VEC],
    bool (&bad)[VEC]) {
  int kk[NT][VEC];
  bool bb[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    bb[v] = is_nan(tv[v]);
#pragma unroll
    for (int t = 0; t < NT; ++t) kk[t][v] = 0;
  }
  int m = 0;
  for (; m + kExceedAhead <= M; m += kExceedAhead) {
    T x[kExceedAhead][VEC];
#pragma unroll
    for (int u = 0; u < kExceedAhead; ++u)
      load_v<T, VEC>(xe + (m + u) * member_stride, x[u]);
#pragma unroll
    for (int u = 0; u < kExceedAhead; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        bb[v] = bb[v] || is_nan(x[u][v]);
#pragma unroll
        for (int t = 0; t < NT; ++t) kk[t][v] += x[u][v] > hv[t][v] ? 1 : 0;
      }
  }
  for (; m < M; ++m) {
    T x[VEC];
    load_v<T, VEC>(xe + m * member_stride, x);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      bb[v] = bb[v] || is_nan(x[v]);
#pragma unroll
      for (int t = 0; t < NT; ++t) kk[t][v] += x[v] > hv[t][v] ? 1 : 0;
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    bad[v] = bb[v];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      k[t][v] = kk[t][v];
      obs[t][v] = tv[v] > hv[t][v];
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// The checks that need no operand; `takes` words the message ("the event table
// takes").  0 or fail()'s negative.
inline int exceed_shape(const char* takes, int dtype, int n_member,
                        int n_threshold) {
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_member >= 1 && n_member <= kExceedMaxMember,
              "n_member=%d: %s 1 to %d members", n_member, takes,
              kExceedMaxMember);
  WB2_REQUIRE(n_threshold >= 1, "n_threshold=%d", n_threshold);
  return 0;
}

// After the shape checks: checks the members and the truth and fills the
// fields of *q that address them (any parameter struct that names them as
// ExceedOperands does: the class-sums kernels without thresholds keep their
// own).  1: go on; 0: no points, a legal no-op; negative: refused.
template <class P>
int member_operands(const void* ens, const int64_t* ens_slab,
                    const void* truth, const int64_t* truth_slab, int n_member,
                    long long member_stride, long long n_outer, int n_row,
                    int n_col, P* q) {
  WB2_REQUIRE(member_stride >= 0, "member_stride=%lld is negative",
              member_stride);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_row);
  WB2_EMPTY_OK(n_col);
  WB2_REQUIRE(ens && truth, "null pointer argument");
  q->ens = ens;
  q->truth = truth;
  q->ens_slab = reinterpret_cast<const long long*>(ens_slab);
  q->truth_slab = reinterpret_cast<const long long*>(truth_slab);
  q->member_stride = member_stride;
  q->n_outer = n_outer;
  q->n_member = n_member;
  return 1;
}

// member_operands() and the thresholds that wb2_event_counts, wb2_event_codes
// and wb2_twcrps_sums share (thr[] and thr_slab[] are exceed_batches()'s).
inline int exceed_operands(const void* ens, const int64_t* ens_slab,
                           const void* truth, const int64_t* truth_slab,
                           const void* const* threshold, int n_threshold,
                           int n_member, long long member_stride,
                           long long n_outer, int n_row, int n_col,
                           ExceedOperands* q) {
  const int go = member_operands(ens, ens_slab, truth, truth_slab, n_member,
                                 member_stride, n_outer, n_row, n_col, q);
  if (go <= 0) return go;
  WB2_REQUIRE(threshold, "null pointer argument");
  for (int t = 0; t < n_threshold; ++t)
    WB2_REQUIRE(threshold[t], "null pointer argument (threshold %d)", t);
  return 1;
}

// May the launches use 16-byte lanes?  (Every threshold of the call counts:
// its batches run the same instantiations.)
inline bool exceed_wide(int dtype, const void* ens, const void* truth,
                        const void* const* threshold, int n_threshold,
                        int n_col, long long member_stride) {
  const int w = wide_lanes(dtype);
  bool wide = all_aligned16(ens, truth) && n_col % w == 0 &&
              member_stride % w == 0;
  for (int t = 0; t < n_threshold; ++t) wide = wide && aligned16(threshold[t]);
  return wide;
}

// More thresholds than one launch takes: further launches, each with its own
// read of the members.  launch(t0, nt) enqueues thresholds t0 .. t0 + nt - 1,
// which q->thr[] and q->thr_slab[] then name.
template <class F>
int exceed_batches(ExceedOperands* q, const void* const* threshold,
                   const int64_t* thr_slab, int n_threshold, int per_launch,
                   F&& launch) {
  for (int t0 = 0; t0 < n_threshold; t0 += per_launch) {
    const int nt = n_threshold - t0 < per_launch ? n_threshold - t0
                                                 : per_launch;
    for (int t = 0; t < kExceedThr; ++t) {
      q->thr[t] = t < nt ? threshold[t0 + t] : nullptr;
      q->thr_slab[t] = (t < nt && thr_slab)
          ? reinterpret_cast<const long long*>(thr_slab) +
                (long long)(t0 + t) * q->n_outer
          : nullptr;
    }
    launch(t0, nt);
    WB2_HIP_OK(hipGetLastError());
  }
  return 0;
}

// f(T{}, std::integral_constant<int, VEC>{}, std::integral_constant<int,
// NT>{}): for_field() and the thresholds of a launch, 1 .. kExceedThr.
template <class F>
void for_exceed(int dtype, bool wide, int nt, F&& f) {
  for_field(dtype, wide, [&](auto T0, auto V) {
    switch (nt) {
      case 1: f(T0, V, std::integral_constant<int, 1>{}); break;
      case 2: f(T0, V, std::integral_constant<int, 2>{}); break;
      case 3: f(T0, V, std::integral_constant<int, 3>{}); break;
      default: f(T0, V, std::integral_constant<int, 4>{}); break;
    }
  });
}

}  // namespace wb2
