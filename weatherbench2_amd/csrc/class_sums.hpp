// The class-sums layer under K20 (crps_bins.hip), K21 (twcrps.hip) and K24
// (conditional_sums.hip): kernels in which one wave owns one row of one outer
// index, walks it in tiles of 64 columns and turns the points into per-(row,
// column class) sums, each ONE sequential chain over the columns of the class.
//
// Device: class_tile() requests a lane's class, truth and members, all before
// any is looked at; class_change() is the mask of the columns that open
// another class.  What a point contributes, the LDS tile and the walk that
// adds it are the kernel's own.  Two things stay copies, because the shared
// form tipped a kernel that is checked by registers and speed against its
// parent (profiles/NOTES.md): the walk in all three (as one function over the
// kernels' callables it gave K20 its registers back, K21 and K24 other ones),
// and K20's own tile requests and change mask (with either function inlined
// its float32 64-slot form was 1.6 % slower at equal registers).  Host: the
// checks, the operand fill (on event_common.hpp's member_operands()), the
// padded-network dispatch, the grid and the geometry fields that the three
// entry points share.
#pragma once

#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "ensemble_kernels.hpp"
#include "event_common.hpp"
#include "launch_common.hpp"
#include "wb2hip.h"

namespace wb2 {

// lane b owns bin b (K20), and the padded sorting networks end at 64
constexpr int kClassMaxMember = 64;

// One tile of a row, for the lane whose column is `colc` (the kernel's: a lane
// past the end of the row takes the last column again): `cls_v` is its class,
// `y` its truth and x[0 .. Mt) its members; also() makes the kernel's further
// requests (K21's thresholds) between the truth's and the members'.  The
// member bases are wave-uniform (K3's buffer loads); a slot >= Mt is switched
// off through its descriptor and costs no memory access.  The stride and the
// member count are made opaque per tile, or hipcc keeps NPAD bases and NPAD
// lane masks in SGPRs across the tile loop.  (Fields, not the parameter
// struct: see exceed_slab().  With `colc` formed in here K24's float32 32-slot
// form allocates two VGPRs fewer than its parent.)
template <typename T, int NPAD, class F>
__device__ __forceinline__ void class_tile(
    const T* xb, const T* tb, const int* col_class, long long member_stride,
    int M, int colc, int& cls_v, T& y, int& Mt, T (&x)[NPAD], F&& also) {
  cls_v = col_class[colc];
  y = tb[colc];
  also();
  long long stride = member_stride;
  Mt = M;
  asm volatile("" : "+s"(stride), "+s"(Mt));
  const int lane_bytes = colc * (int)sizeof(T);
#pragma unroll
  for (int m = 0; m < NPAD; ++m)
    x[m] = member_load<T, true>(xb + m * stride, lane_bytes,
                                m < Mt ? 0x7fffffff : 0);
}

// bit j: column j of the tile opens another class than column j - 1 (bit 0:
// than the running sums, whose class is `cur`)
__device__ __forceinline__ unsigned long long class_change(int cls_v, int cur,
                                                           int lane) {
  const int c_first = __builtin_amdgcn_readlane(cls_v, 0);
  const int cls_left = __shfl_up(cls_v, 1);
  return __ballot(lane > 0 && cls_v != cls_left) |
         (c_first != cur ? 1ull : 0ull);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// The checks that need no operand, worded with `takes`.  0 or negative.
inline int class_shape(const char* takes, int dtype, int n_member,
                       int n_class) {
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_member >= 1 && n_member <= kClassMaxMember,
              "n_member=%d: %s 1 to %d members", n_member, takes,
              kClassMaxMember);
  WB2_REQUIRE(n_class >= 1 && n_class <= kExceedMaxClass,
              "n_class=%d: %s 1 to %d column classes", n_class, takes,
              kExceedMaxClass);
  return 0;
}

// After member_operands() or exceed_operands() said "go on": what a class-sums
// parameter struct holds beside the members and the truth.  0 or negative.
template <class P>
int class_operands(const int32_t* col_class, double* sums, int32_t* cnt,
                   int n_row, int n_col, int n_class, P* q) {
  WB2_REQUIRE(col_class && sums && cnt, "null pointer argument");
  // (a lane's byte offset into its row is an int)
  WB2_REQUIRE((long long)n_col * 8 < (1ll << 31),
              "n_col=%d: the row is too long", n_col);
  q->col_class = col_class;
  q->sums = sums;
  q->cnt = cnt;
  q->n_row = n_row;
  q->n_col = n_col;
  q->n_class = n_class;
  return 0;
}

// f(T{}, std::integral_constant<int, NPAD>{}): the field's dtype and the
// padded network of `n_member` members, 2 .. kClassMaxMember.
template <class F>
void for_npad(int dtype, int n_member, F&& f) {
  auto padded = [&](auto T0) {
    if (n_member <= 2) f(T0, std::integral_constant<int, 2>{});
    else if (n_member <= 4) f(T0, std::integral_constant<int, 4>{});
    else if (n_member <= 8) f(T0, std::integral_constant<int, 8>{});
    else if (n_member <= 16) f(T0, std::integral_constant<int, 16>{});
    else if (n_member <= 32) f(T0, std::integral_constant<int, 32>{});
    else f(T0, std::integral_constant<int, 64>{});
  };
  if (dtype == WB2_F32) padded(float{});
  else padded(double{});
}

// one wave per row of every outer index; 0 or fail()'s negative
inline int class_grid(long long n_outer, int n_row, dim3* grid, dim3* block) {
  WB2_REQUIRE(outer_grid(n_outer, n_row, grid),
              "the grid does not fit: %lld outer indices of %d rows", n_outer,
              n_row);
  *block = dim3(kWave);
  return 0;
}

// the fields every *_geometry entry point of the layer reports
inline int class_geometry(int32_t* min_member, int32_t* max_member,
                          int32_t* tile_cols, int32_t* rows_per_group,
                          int32_t* max_grid_outer) {
  WB2_REQUIRE(min_member && max_member && tile_cols && rows_per_group &&
              max_grid_outer, "null pointer argument");
  *min_member = 1;
  *max_member = kClassMaxMember;
  *tile_cols = kWave;
  *rows_per_group = 1;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

}  // namespace wb2
