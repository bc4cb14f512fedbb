// K17 of libwb2hip.so: dataset slicing as one box gather
// (scripts/slice_dataset.py: .isel / .sel / .drop_sel on the last two dims of
// a variable, together with whatever was selected on the dims before them).
//
//   wb2_box_gather  out[s][i][j] = in[src_slab[s] * n_row_in * n_col_in
//                                     + row[i] * n_col_in + col(j)]
//
// A variable is [n_slab][n_row_in][n_col_in]; `src_slab` (K13's slab
// convention; null = identity) says which input slab an output slab is cut
// from, `row` (null = identity) which input row an output row is, and the
// columns are an affine run col0 + j * col_step or a list.  A pure bit copy of
// 4- or 8-byte elements: no holes, no casts, no atomics, no LDS.
//
// A thread owns VEC adjacent output columns of kAhead output rows; it requests
// all its rows before it stores the first.  A workgroup of 256 threads is
// tile_cols / VEC threads wide (a power of two, so a thread finds its row and
// column by a shift and a mask) and owns a tile of one output slab; the slabs
// go along the grid by outer_grid().  Column forms:
//   run       col_step == 1 and everything 16-byte aligned: 16-byte loads and
//             stores
//   reversed  col_step == -1, aligned likewise: a 16-byte load from the
//             mirrored address, reversed in registers, a 16-byte store
//   scalar    any other affine run (coalesced where |col_step| == 1; a strided
//             run reads part of each 128-byte request it touches)
//   list      the column table, scalar gathers
// Loads and stores stream (nontemporal): every output element is written once
// and an input element is read at most once per use.

#include <cstdint>

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kBoxThreads = 256;
constexpr int kAhead = 4;  // rows a thread requests before it stores any

struct BoxParams {
  const void* in;
  const long long* src_slab;  // [n_out_slab] or null
  const int* row;             // [n_row_out] or null
  const int* col;             // [n_col_out] or null (the affine run)
  void* out;
  long long n_out_slab, slab_in;  // slab_in = n_row_in * n_col_in
  int n_col_in, n_row_out, n_col_out, col0, col_step;
  int col_shift;   // log2 of the threads along the columns of a tile
  unsigned n_ctile;  // tiles along the columns
};

template <typename U, int VEC, int FORM>
__global__ void __launch_bounds__(kBoxThreads)
    box_gather_kernel(const BoxParams p) {
  const long long s = outer_index();
  if (s >= p.n_out_slab) return;
  // (one division per workgroup, none per element)
  const unsigned ctile = blockIdx.x % p.n_ctile;
  const unsigned rtile = blockIdx.x / p.n_ctile;
  const int tcol = threadIdx.x & ((1 << p.col_shift) - 1);
  const int trow = threadIdx.x >> p.col_shift;
  const int tile_rows = kBoxThreads >> p.col_shift;
  const long long j = (((long long)ctile << p.col_shift) + tcol) * VEC;
  if (j >= p.n_col_out) return;
  long long c;  // the input column of the first element this thread reads
  if constexpr (FORM == WB2_BOX_RUN) c = p.col0 + j;
  else if constexpr (FORM == WB2_BOX_REVERSED) c = p.col0 - j - (VEC - 1);
  else if constexpr (FORM == WB2_BOX_SCALAR) c = p.col0 + j * p.col_step;
  else c = p.col[j];
  const long long src = p.src_slab ? p.src_slab[s] : s;
  const U* in = static_cast<const U*>(p.in) + src * p.slab_in + c;
  U* out = static_cast<U*>(p.out) +
           s * ((long long)p.n_row_out * p.n_col_out) + j;
  const long long r0 = (long long)rtile * (tile_rows * kAhead) + trow;
  U v[kAhead][VEC];
#pragma unroll
  for (int k = 0; k < kAhead; ++k) {
    const long long r = r0 + k * tile_rows;
    if (r < p.n_row_out) {
      const long long ri = p.row ? p.row[r] : r;
      load_v<U, VEC>(in + ri * p.n_col_in, v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kAhead; ++k) {
    const long long r = r0 + k * tile_rows;
    if (r < p.n_row_out) {
      if constexpr (FORM == WB2_BOX_REVERSED) {
#pragma unroll
        for (int e = 0; e < VEC / 2; ++e) {
          const U a = v[k][e];
          v[k][e] = v[k][VEC - 1 - e];
          v[k][VEC - 1 - e] = a;
        }
      }
      store_v<U, VEC>(out + r * p.n_col_out, v[k]);
    }
  }
}

// threads along the columns of a tile: the least power of two that covers the
// output row, 256 at most (rows of a narrow box share a wavefront)
inline int col_shift_of(long long n_col_out, int vec) {
  const long long need = (n_col_out + vec - 1) / vec;
  int shift = 0;
  while (shift < 8 && (1ll << shift) < need) ++shift;
  return shift;
}

inline bool form_is_wide(int form) {
  return form == WB2_BOX_RUN || form == WB2_BOX_REVERSED;
}

#define WB2_REQUIRE_ELEM(elem_size)                                        \
  WB2_REQUIRE(elem_size == 4 || elem_size == 8,                            \
              "unsupported element size %d (4 or 8 bytes only)",           \
              (int)elem_size)

template <int FORM>
void launch_form(int elem_size, dim3 grid, hipStream_t s, const BoxParams& p) {
  // the (element size, width) dispatch of for_field() with the width fixed by
  // the form, so that only the eight instances that can run are built; the
  // elements travel as unsigned integers, so no bit pattern is touched
  constexpr bool wide = FORM == WB2_BOX_RUN || FORM == WB2_BOX_REVERSED;
  if (elem_size == 4)
    hipLaunchKernelGGL((box_gather_kernel<uint32_t, wide ? 4 : 1, FORM>), grid,
                       dim3(kBoxThreads), 0, s, p);
  else
    hipLaunchKernelGGL((box_gather_kernel<uint64_t, wide ? 2 : 1, FORM>), grid,
                       dim3(kBoxThreads), 0, s, p);
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_box_gather_geometry(int elem_size, int form, int32_t n_col_out,
                            int32_t* tile_rows, int32_t* tile_cols,
                            int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE_ELEM(elem_size);
  WB2_REQUIRE(form >= WB2_BOX_RUN && form <= WB2_BOX_LIST,
              "unknown column form %d", form);
  WB2_REQUIRE(n_col_out >= 0, "n_col_out=%d is negative", (int)n_col_out);
  WB2_REQUIRE(tile_rows && tile_cols && max_grid_outer,
              "null pointer argument");
  const int vec = form_is_wide(form) ? 16 / elem_size : 1;
  const int shift = col_shift_of(n_col_out, vec);
  *tile_rows = (kBoxThreads >> shift) * kAhead;
  *tile_cols = (1 << shift) * vec;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_box_gather_form(int elem_size, const void* in, const void* out,
                        int32_t n_col_in, int32_t col0, int32_t col_step,
                        int32_t has_col_list, int32_t n_col_out) {
  using namespace wb2;
  WB2_REQUIRE_ELEM(elem_size);
  if (has_col_list) return WB2_BOX_LIST;
  WB2_REQUIRE(col_step != 0, "col_step is zero");
  const int w = 16 / elem_size;
  // the one 16-byte-lane rule: both bases aligned and every row of the input
  // and of the output a whole number of lanes, the run starting on a lane
  const bool lanes = all_aligned16(in, out) && n_col_in % w == 0 &&
                     n_col_out % w == 0;
  if (col_step == 1 && lanes && col0 % w == 0) return WB2_BOX_RUN;
  if (col_step == -1 && lanes && (col0 + 1) % w == 0) return WB2_BOX_REVERSED;
  return WB2_BOX_SCALAR;
}

int wb2_box_gather(int elem_size, const void* in, const int64_t* src_slab,
                   int64_t n_out_slab, int32_t n_row_in, int32_t n_col_in,
                   const int32_t* row, int32_t n_row_out, int32_t col0,
                   int32_t col_step, const int32_t* col_list,
                   int32_t n_col_out, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE_ELEM(elem_size);
  WB2_REQUIRE(n_row_in >= 0 && n_col_in >= 0,
              "bad sizes: an input slab of %d x %d", (int)n_row_in,
              (int)n_col_in);
  WB2_REQUIRE(col_list || col_step != 0, "col_step is zero");
  WB2_EMPTY_OK(n_out_slab);
  WB2_EMPTY_OK(n_row_out);
  WB2_EMPTY_OK(n_col_out);
  WB2_REQUIRE(in && out, "null pointer argument");
  WB2_REQUIRE(row || n_row_out <= n_row_in,
              "without a row table the %d output rows leave [0, %d)",
              (int)n_row_out, (int)n_row_in);
  if (!col_list) {
    const long long last = col0 + (long long)(n_col_out - 1) * col_step;
    WB2_REQUIRE(col0 >= 0 && col0 < n_col_in && last >= 0 && last < n_col_in,
                "the column run %d + j * %d, j < %d, leaves [0, %d)",
                (int)col0, (int)col_step, (int)n_col_out, (int)n_col_in);
  }
  const int form = wb2_box_gather_form(elem_size, in, out, n_col_in, col0,
                                       col_step, col_list != nullptr,
                                       n_col_out);
  const int vec = form_is_wide(form) ? 16 / elem_size : 1;
  BoxParams p{};
  p.in = in;
  p.src_slab = reinterpret_cast<const long long*>(src_slab);
  p.row = row;
  p.col = col_list;
  p.out = out;
  p.n_out_slab = n_out_slab;
  p.slab_in = (long long)n_row_in * n_col_in;
  p.n_col_in = n_col_in;
  p.n_row_out = n_row_out;
  p.n_col_out = n_col_out;
  p.col0 = col0;
  p.col_step = col_step;
  p.col_shift = col_shift_of(n_col_out, vec);
  const long long tile_cols = (1ll << p.col_shift) * vec;
  const long long tile_rows = (long long)(kBoxThreads >> p.col_shift) * kAhead;
  const long long n_ctile = (n_col_out + tile_cols - 1) / tile_cols;
  const long long n_rtile = (n_row_out + tile_rows - 1) / tile_rows;
  p.n_ctile = (unsigned)n_ctile;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_out_slab, n_ctile * n_rtile, &grid),
              "the grid does not fit: %lld slabs of %lld x %lld tiles",
              (long long)n_out_slab, n_rtile, n_ctile);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (form) {
    case WB2_BOX_RUN: launch_form<WB2_BOX_RUN>(elem_size, grid, s, p); break;
    case WB2_BOX_REVERSED:
      launch_form<WB2_BOX_REVERSED>(elem_size, grid, s, p);
      break;
    case WB2_BOX_SCALAR:
      launch_form<WB2_BOX_SCALAR>(elem_size, grid, s, p);
      break;
    default: launch_form<WB2_BOX_LIST>(elem_size, grid, s, p); break;
  }
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
