// The LDS passes of the one-wave real FFT, shared by K4f (spectrum_fused.hip)
// and K25 (cross_spectrum.hip): the slab-store override of fft_core.hpp, the
// hand-scheduled inter-pass twiddle multiplies, the single-instruction slab
// read and a later Stockham pass over a wave's slab.  Device code; includes
// fft_core.hpp with the override in place, so it comes before any other
// include of that header.
#pragma once

#include "common.hpp"

// 8-byte LDS stores stay single ds_write_b64 (17 cycles per instruction and
// SIMD, tools/valu_rate.hip) instead of the ds_write2_b64 pairs hipcc's
// load/store optimiser makes of them (44): volatile stores in address space 3
#if defined(__HIP_DEVICE_COMPILE__)
namespace wb2 {
template <typename C>
__device__ __forceinline__ void fused_slab_store(C* p, C v) {
  *(__attribute__((address_space(3))) volatile C*)p = v;
}
}  // namespace wb2
#define WB2_FFT_SLAB_STORE(ptr, value) ::wb2::fused_slab_store(ptr, value)
#endif
#include "fft_core.hpp"

namespace wb2 {
namespace fused {

using namespace fftcore;

// ---- inter-pass twiddle multiplies --------------------------------------------
// a * w as v_pk_mul_f32 + v_pk_fma_f32 with the rotation (-w.y, w.x) expressed
// through op_sel / neg_lo (hipcc materialises it with two extra VALU moves per
// twiddle, or keeps a second register pair per twiddle alive).  gfx950 needs one
// wait state between a packed-fp32 write and a dependent VALU read; the compiler
// cannot see inside the asm, so the multiplies of a block are interleaved and the
// block ends with the wait state for whatever consumes the last result.
#define WB2_PK_MUL(t, a, w) "v_pk_mul_f32 " t ", " a ", " w " op_sel_hi:[0,1]\n\t"
#define WB2_PK_FMA(t, a, w)                                       \
  "v_pk_fma_f32 " t ", " a ", " w ", " t                          \
  " op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
__device__ __forceinline__ void cmul1_asm(cf& a0, cf w0) {
  cf t0;
  asm(WB2_PK_MUL("%0", "%1", "%2") "s_nop 0\n\t" WB2_PK_FMA("%0", "%1", "%2")
      "s_nop 0"
      : "=&v"(t0)
      : "v"(a0), "v"(w0));
  a0 = t0;
}
__device__ __forceinline__ void cmul2_asm(cf& a0, cf w0, cf& a1, cf w1) {
  cf t0, t1;
  asm(WB2_PK_MUL("%0", "%2", "%3") WB2_PK_MUL("%1", "%4", "%5")
      WB2_PK_FMA("%0", "%2", "%3") WB2_PK_FMA("%1", "%4", "%5") "s_nop 0"
      : "=&v"(t0), "=&v"(t1)
      : "v"(a0), "v"(w0), "v"(a1), "v"(w1));
  a0 = t0;
  a1 = t1;
}
__device__ __forceinline__ void cmul3_asm(cf& a0, cf w0, cf& a1, cf w1, cf& a2,
                                          cf w2) {
  cf t0, t1, t2;
  asm(WB2_PK_MUL("%0", "%3", "%4") WB2_PK_MUL("%1", "%5", "%6")
      WB2_PK_MUL("%2", "%7", "%8") WB2_PK_FMA("%0", "%3", "%4")
      WB2_PK_FMA("%1", "%5", "%6") WB2_PK_FMA("%2", "%7", "%8") "s_nop 0"
      : "=&v"(t0), "=&v"(t1), "=&v"(t2)
      : "v"(a0), "v"(w0), "v"(a1), "v"(w1), "v"(a2), "v"(w2));
  a0 = t0;
  a1 = t1;
  a2 = t2;
}
#undef WB2_PK_MUL
#undef WB2_PK_FMA

template <int N>
__device__ __forceinline__ void twiddle_block(cf* v, const cf* tw) {
  // v[0..N) *= tw[0..N)
  if constexpr (N >= 3) {
    cmul3_asm(v[0], tw[0], v[1], tw[1], v[2], tw[2]);
    twiddle_block<N - 3>(v + 3, tw + 3);
  } else if constexpr (N == 2) {
    cmul2_asm(v[0], tw[0], v[1], tw[1]);
  } else if constexpr (N == 1) {
    cmul1_asm(v[0], tw[0]);
  }
}

// float64 rows: plain complex multiplies (v_mul_f64 / v_fma_f64; there is no
// packed float64 arithmetic to hand-schedule)
template <int N>
__device__ __forceinline__ void twiddle_block(cd* v, const cd* tw) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = cmul(v[i], tw[i]);
}

// One read of a complex point from the wave's LDS slab (or the shared twiddle
// table): 8 bytes for float32 rows, 16 for float64 ones.
template <typename C>
__device__ __forceinline__ C lds_read(const C* p) {
  // its own ds_read_b64: hipcc's load/store optimiser otherwise pairs the
  // 8-byte slab reads into ds_read2_b64 / ds_read2st64_b64, which gfx950
  // services at 44 cycles per wave-instruction against 6.4 for a ds_read_b64
  // (tools/valu_rate.hip); volatile in address space 3 is the one thing the
  // optimiser does not merge
  typedef __attribute__((address_space(3))) const volatile C* lds_ptr;
  return *(lds_ptr)p;
}

// A later pass (NS > 1) over the wave's slab: strided reads, twiddle multiplies
// (the twiddles of a lane depend on the lane only: VGPR-resident for the whole
// kernel), butterflies, in-place writes.
template <typename P, int R, typename C>
__device__ __forceinline__ void lds_pass(C* __restrict__ z, int lane,
                                         C (&tw)[P::ROUNDS][R - 1]) {
  C v[P::ROUNDS][R];
  P::load([&](int i) { return lds_read(z + i); }, lane, v);
#pragma unroll
  for (int rd = 0; rd < P::ROUNDS; ++rd)
    twiddle_block<R - 1>(&v[rd][1], &tw[rd][0]);
  P::butterflies(v);
  // every read of this pass precedes every write (program order; the DS
  // operations of one wave execute in order) -- the fence only restrains the
  // compiler
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  P::store(z, lane, v);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

}  // namespace fused
}  // namespace wb2
