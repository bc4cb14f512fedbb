// K25 of libwb2hip.so: the zonal cross-spectrum of forecast and truth.
//
// One WAVE owns one row (outer index o, latitude row i).  It transforms the
// truth row as K4f does (spectrum_fused.hip: N/2 complex points, Plan<N/2>'s
// Stockham passes, pass 0 straight from memory with non-temporal loads) into a
// slab of its own, then every member row, in storage order, into a second
// slab.  Per member it recombines BOTH rows for the bin pairs (k, N/2 - k)
// from one pair of LDS reads each (fft_core.hpp: recombine_pair_complex) and
// forms, in the row dtype,
//   |F|^2 = F.x F.x + F.y F.y,   Re(F conj T) = F.x T.x + F.y T.y,
//   Im(F conj T) = F.y T.x - F.x T.y   (and |T|^2 once, with member 0),
// widens each product to float64, multiplies it once by s_k C_i (s_0 = 1, s_k =
// 2 otherwise, Nyquist included; C_i the circumference of the row) and adds it
// to float64 accumulators in the lane's registers, the first member starting
// the chain.  After the last member the four spectra are stored once: plain
// stores, no atomics, so two runs are bit-equal.
//
// A row is INVALID iff the truth row or any member row holds a non-finite
// value: the test rides on the pass-0 loads (one comparison per loaded value,
// one wave ballot per transformed row).  An invalid row stores +0.0 in all four
// terms and counts as invalid.
//
// Sign: a forecast that is the truth displaced EASTWARD by d degrees has
// atan2(quadrature, cospectrum) = -2 pi k d / 360 (mod 2 pi).
//
// Simple and untuned: the waves per workgroup are the most of 4, 2, 1 whose
// slabs fit the LDS, whatever that does to the occupancy; the truth's
// recombination is repeated per member instead of held in registers; nothing
// is prefetched across rows or members.

#include "common.hpp"

#include "fft_lds.hpp"

#include "event_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

#include <limits>
#include <string>

#ifndef WB2_CROSS_MAX_BLOCKS
#define WB2_CROSS_MAX_BLOCKS 2048  // workgroups; waves stride over the rest
#endif

namespace wb2 {

// spectrum.hip: the twiddle tables a plan owns (null: the plan has none)
void* spectrum_plan_tables(void* plan, int* dtype, int* n_lon);

namespace cross {

using namespace fftcore;
using fused::lds_pass;
using fused::lds_read;

constexpr int kCrossMaxMember = 128;
constexpr long long kCrossLds = 160 * 1024;

// The passes of a row of N2 complex points, as K4f has them.
template <int N2>
struct Passes {
  using PL = Plan<N2>;
  static constexpr int R0 = PL::R0, R1 = PL::R1, R2 = PL::R2;
  using P0 = Pass<N2, R0, 1, 1, 0, PL::PAD0>;
  using P1 = Pass<N2, R1, R0, R0, PL::PAD0, PL::PAD1>;
  using P2 = Pass<N2, R2, R0 * R1, R0 * R1, PL::PAD1, 0>;
};

// bytes of LDS of a workgroup of `waves` waves: the twq table, then two slabs
// per wave
template <int N2, typename S>
constexpr long long lds_bytes(int waves) {
  return (long long)sizeof(cx<S>) *
         ((N2 / 2 + 2) + (long long)waves * 2 * slab_slots<N2>());
}

// the most of 4, 2 and 1 waves whose slabs and the twq table fit 160 KiB
template <int N2, typename S>
constexpr int waves_per_group() {
  return lds_bytes<N2, S>(4) <= kCrossLds ? 4
         : lds_bytes<N2, S>(2) <= kCrossLds ? 2 : 1;
}

// Where the member sums of a row live.  6 float64 per bin pair and lane beside
// K4f's transform (371 registers of the 512 for float64 rows of 3600) do not
// fit the register file of the long rows: with all of them in registers the
// compiler reported scratch for N/2 >= 900 (float64) and N/2 >= 1280
// (float32).  Those lengths keep the sums in the lane's own elements of `sums`
// instead -- member 0 stores, every later member adds to what the same lane
// stored: the same chain in the same order, the same bits, and for one member
// still one store per value.
template <int N2, typename S>
constexpr bool register_sums() {
  return sizeof(S) == 4 ? N2 <= 1024 : N2 <= 720;
}

struct CrossParams {
  const void* ens;
  const void* truth;
  const void* twz;              // [N2]      as K4f's
  const void* twq;              // [N2/2+1]
  const long long* ens_slab;    // [n_outer] or null: member 0's slab
  const long long* truth_slab;  // [n_outer] or null
  const double* circ;           // [n_row]
  double* sums;                 // [n_outer][n_row][4][N2 + 1]
  int* cnt;                     // [n_outer][n_row][2]
  long long member_stride, n_rows;  // n_rows = n_outer * n_row
  int n_member, n_row;
};

// One row -> its N2-point transform in the slab `z`.  True in a lane that
// loaded a non-finite value.
template <int N2, typename S, typename TW1, typename TW2>
__device__ __forceinline__ bool transform_row(const S* __restrict__ row,
                                              cx<S>* __restrict__ z, int lane,
                                              const cx<S>* g_twz, TW1& tw1,
                                              TW2& tw2) {
  typedef cx<S> C;
  using PS = Passes<N2>;
  constexpr bool RESIDENT_TW = sizeof(S) == 4;
  const S big = std::numeric_limits<S>::max();
  bool off = false;
  {  // ---- pass 0: memory -> butterflies -> contiguous runs in the slab
    C v[PS::P0::ROUNDS][PS::R0];
    const C* src = reinterpret_cast<const C*>(row);
    PS::P0::load(
        [&](int i) {
          const C c = __builtin_nontemporal_load(src + i);
          // (false for NaN and for +-inf)
          off |= !(abs_of(c.x) <= big) | !(abs_of(c.y) <= big);
          return c;
        },
        lane, v);
    PS::P0::butterflies(v);
    PS::P0::store(z, lane, v);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  if constexpr (!RESIDENT_TW) {
    const C* tz = g_twz;
    asm volatile("" : "+s"(tz));  // per row: not hoisted out of the loops
    PS::P1::load_twiddles(tz, lane, tw1);
  }
  lds_pass<typename PS::P1, PS::R1>(z, lane, tw1);
  if constexpr (PS::R2 > 1) {
    if constexpr (!RESIDENT_TW) {
      const C* tz = g_twz;
      asm volatile("" : "+s"(tz));
      PS::P2::load_twiddles(tz, lane, tw2);
    }
    lds_pass<typename PS::P2, PS::R2>(z, lane, tw2);
  }
  return off;
}

template <int N2, typename S>
__global__ void __launch_bounds__((64 * waves_per_group<N2, S>()))
    cross_spectrum_kernel(const CrossParams p) {
  typedef cx<S> C;
  using PS = Passes<N2>;
  constexpr int N = 2 * N2, NB = N2 + 1, NWAVE = waves_per_group<N2, S>();
  constexpr int NH = N2 / 2 + 1;  // bin pairs (k, N2 - k), k = 0..N2/2
  constexpr int NIT = (NH + kWave - 1) / kWave;
  constexpr bool RESIDENT_TW = sizeof(S) == 4;
  constexpr bool REG_ACC = register_sums<N2, S>();
  __shared__ __attribute__((aligned(16))) C s_twq[NH + 1];
  __shared__ __attribute__((aligned(16))) C s_t[NWAVE][slab_slots<N2>()];
  __shared__ __attribute__((aligned(16))) C s_f[NWAVE][slab_slots<N2>()];
  const C* g_twz = static_cast<const C*>(p.twz);
  const C* g_twq = static_cast<const C*>(p.twq);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  for (int i = threadIdx.x; i <= NH; i += blockDim.x)
    s_twq[i] = g_twq[i < NH ? i : NH - 1];
  // inter-pass twiddles, as in K4f: float32 keeps them in VGPRs for the whole
  // kernel, float64 fetches them again before the pass that uses them
  C tw1[PS::P1::ROUNDS][PS::P1::NTW], tw2[PS::P2::ROUNDS][PS::P2::NTW];
  if constexpr (RESIDENT_TW) {
    PS::P1::load_twiddles(g_twz, lane, tw1);
    if constexpr (PS::R2 > 1) PS::P2::load_twiddles(g_twz, lane, tw2);
  }
  __syncthreads();
  C* zt = s_t[wave];
  C* zf = s_f[wave];
  const S half_inv_n = (S)0.5 / (S)N;
  const int M = p.n_member;
  const long long slab = (long long)p.n_row * N;
  const long long stride = (long long)gridDim.x * NWAVE;
  for (long long r = (long long)blockIdx.x * NWAVE + wave; r < p.n_rows;
       r += stride) {
    const long long o = r / p.n_row;
    const int row = (int)(r - o * p.n_row);
    const double c = p.circ[row], c2 = 2.0 * c;
    const long long first = (long long)row * N;
    const S* trow = exceed_slab<S>(p.truth, p.truth_slab, o, slab, first);
    const S* frow = exceed_slab<S>(p.ens, p.ens_slab, o, slab, first);
    double* orow = p.sums + r * 4 * NB;
    bool off = transform_row<N2, S>(trow, zt, lane, g_twz, tw1, tw2);
    // bin k / bin N2 - k of power_forecast, cospectrum and quadrature
    constexpr int NACC = REG_ACC ? NIT : 1;
    double pf1[NACC], pf2[NACC], co1[NACC], co2[NACC], qu1[NACC], qu2[NACC];
    for (int m = 0; m < M; ++m) {
      off |= transform_row<N2, S>(frow + m * p.member_stride, zf, lane, g_twz,
                                  tw1, tw2);
      auto bin_pair = [&](int i) {
        const int k = lane + i * kWave;
        if ((i + 1) * kWave <= NH || k < NH) {
          const int km = (i == 0 && k == 0) ? 0 : N2 - k;
          const C w = lds_read(s_twq + k);
          C t1, t2, f1, f2;
          recombine_pair_complex(lds_read(zt + k), lds_read(zt + km), w,
                                 half_inv_n, t1, t2);
          recombine_pair_complex(lds_read(zf + k), lds_read(zf + km), w,
                                 half_inv_n, f1, f2);
          // every bin but 0 is doubled (Nyquist too), as K4f has it
          const double s1 = (i == 0 && k == 0) ? c : c2;
          const double vp1 = (double)(f1.x * f1.x + f1.y * f1.y) * s1;
          const double vp2 = (double)(f2.x * f2.x + f2.y * f2.y) * c2;
          const double vc1 = (double)(f1.x * t1.x + f1.y * t1.y) * s1;
          const double vc2 = (double)(f2.x * t2.x + f2.y * t2.y) * c2;
          const double vq1 = (double)(f1.y * t1.x - f1.x * t1.y) * s1;
          const double vq2 = (double)(f2.y * t2.x - f2.x * t2.y) * c2;
          const bool pair = 2 * k != N2;  // (k = N2 / 2 is its own mirror)
          double* o1 = orow + k;
          double* o2 = orow + N2 - k;
          if (m == 0) {  // the first term starts the chain
            // power_truth: stored now (an invalid row overwrites it below)
            o1[NB] = (double)(t1.x * t1.x + t1.y * t1.y) * s1;
            if (pair) o2[NB] = (double)(t2.x * t2.x + t2.y * t2.y) * c2;
            if constexpr (REG_ACC) {
              pf1[i] = vp1;
              pf2[i] = vp2;
              co1[i] = vc1;
              co2[i] = vc2;
              qu1[i] = vq1;
              qu2[i] = vq2;
            } else {
              o1[0] = vp1;
              o1[2 * NB] = vc1;
              o1[3 * NB] = vq1;
              if (pair) {
                o2[0] = vp2;
                o2[2 * NB] = vc2;
                o2[3 * NB] = vq2;
              }
            }
          } else if constexpr (REG_ACC) {
            pf1[i] = pf1[i] + vp1;
            pf2[i] = pf2[i] + vp2;
            co1[i] = co1[i] + vc1;
            co2[i] = co2[i] + vc2;
            qu1[i] = qu1[i] + vq1;
            qu2[i] = qu2[i] + vq2;
          } else {  // the lane's own elements: the same chain, in memory
            o1[0] = o1[0] + vp1;
            o1[2 * NB] = o1[2 * NB] + vc1;
            o1[3 * NB] = o1[3 * NB] + vq1;
            if (pair) {
              o2[0] = o2[0] + vp2;
              o2[2 * NB] = o2[2 * NB] + vc2;
              o2[3 * NB] = o2[3 * NB] + vq2;
            }
          }
        }
      };
      if constexpr (REG_ACC) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) bin_pair(i);
      } else {
        // a rolled loop: unrolled, the loads and sums of all NIT pairs are in
        // flight at once and cost these rows scratch as well
#pragma unroll 1
        for (int i = 0; i < NIT; ++i) bin_pair(i);
      }
      // the next member's pass 0 writes the slab these reads came from
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    const bool bad = __ballot(off) != 0ull;  // wave-uniform
    if (REG_ACC || bad) {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int k = lane + i * kWave;
        if (k < NH) {
          double* o1 = orow + k;
          double* o2 = orow + N2 - k;
          const bool pair = 2 * k != N2;
          double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          if constexpr (REG_ACC) {
            if (!bad) {
              v[0] = pf1[i];
              v[1] = co1[i];
              v[2] = qu1[i];
              v[3] = pf2[i];
              v[4] = co2[i];
              v[5] = qu2[i];
            }
          }
          o1[0] = v[0];
          o1[2 * NB] = v[1];
          o1[3 * NB] = v[2];
          if (bad) o1[NB] = 0.0;
          if (pair) {
            o2[0] = v[3];
            o2[2 * NB] = v[4];
            o2[3 * NB] = v[5];
            if (bad) o2[NB] = 0.0;
          }
        }
      }
    }
    if (lane == 0) {
      p.cnt[2 * r] = bad ? 0 : 1;
      p.cnt[2 * r + 1] = bad ? 1 : 0;
    }
  }
}

template <int N2, typename S>
int launch(const CrossParams& p, hipStream_t s) {
  constexpr int NWAVE = waves_per_group<N2, S>();
  static_assert(lds_bytes<N2, S>(NWAVE) <= kCrossLds, "the slabs fit the LDS");
  long long blocks = (p.n_rows + NWAVE - 1) / NWAVE;
  if (blocks > WB2_CROSS_MAX_BLOCKS) blocks = WB2_CROSS_MAX_BLOCKS;
  hipLaunchKernelGGL((cross_spectrum_kernel<N2, S>), dim3((unsigned)blocks),
                     dim3(64 * NWAVE), 0, s, p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

// (waves per workgroup, LDS bytes) of an instantiated (N2, dtype)
inline bool geometry_of(int dtype, int n2, int* waves, long long* lds) {
  switch (n2) {
#define WB2_CASE(N2)                                                        \
  case N2:                                                                  \
    *waves = dtype == WB2_F32 ? waves_per_group<N2, float>()                \
                              : waves_per_group<N2, double>();              \
    *lds = dtype == WB2_F32 ? lds_bytes<N2, float>(*waves)                  \
                            : lds_bytes<N2, double>(*waves);                \
    return true;
    WB2_FFT_PLAN_SIZES(WB2_CASE)
#undef WB2_CASE
  }
  return false;
}

inline bool instantiated(int n_col) {
  int waves;
  long long lds;
  return n_col >= 2 && n_col % 2 == 0 &&
         geometry_of(WB2_F32, n_col / 2, &waves, &lds);
}

// " 64 128 ...": the instantiated row lengths, for the message
inline std::string row_lengths() {
  std::string s;
#define WB2_LEN(N2) s += " " + std::to_string(2 * N2);
  WB2_FFT_PLAN_SIZES(WB2_LEN)
#undef WB2_LEN
  return s;
}

}  // namespace cross
}  // namespace wb2

extern "C" {

int wb2_cross_spectrum_geometry(int dtype, int32_t n_col, int32_t n_member,
                                int32_t* supported, int32_t* waves_per_group,
                                int64_t* lds_bytes, int32_t* max_grid_outer) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(n_member >= 1 && n_member <= cross::kCrossMaxMember,
              "n_member=%d: the cross-spectrum takes 1 to %d members",
              (int)n_member, cross::kCrossMaxMember);
  WB2_REQUIRE(supported && waves_per_group && lds_bytes && max_grid_outer,
              "null pointer argument");
  int waves = 0;
  long long lds = 0;
  const bool ok = n_col >= 2 && n_col % 2 == 0 &&
                  cross::geometry_of(dtype, n_col / 2, &waves, &lds);
  *supported = ok ? 1 : 0;
  *waves_per_group = ok ? waves : 0;
  *lds_bytes = ok ? lds : 0;
  *max_grid_outer = WB2_CROSS_MAX_BLOCKS;
  return 0;
}

int wb2_cross_spectrum_rows(void* plan, int dtype, const void* ens,
                            const int64_t* ens_slab, const void* truth,
                            const int64_t* truth_slab, int32_t n_member,
                            int64_t member_stride, int64_t n_outer,
                            int32_t n_row, int32_t n_col,
                            const double* circumference, double* sums,
                            int32_t* cnt, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(cross::instantiated(n_col),
              "n_col=%d is not instantiated: the cross-spectrum takes the row "
              "lengths%s", (int)n_col, cross::row_lengths().c_str());
  WB2_REQUIRE(n_member >= 1 && n_member <= cross::kCrossMaxMember,
              "n_member=%d: the cross-spectrum takes 1 to %d members",
              (int)n_member, cross::kCrossMaxMember);
  WB2_REQUIRE(member_stride >= 0, "member_stride=%lld is negative",
              (long long)member_stride);
  WB2_EMPTY_OK(n_outer);
  WB2_EMPTY_OK(n_row);
  // a complex point of pass 0 is one load: 8 bytes (float32), 16 (float64)
  const int align = dtype == WB2_F32 ? 8 : 16;
  WB2_REQUIRE(reinterpret_cast<uintptr_t>(ens) % align == 0 &&
                  reinterpret_cast<uintptr_t>(truth) % align == 0 &&
                  member_stride % 2 == 0,
              "the rows are not %d-byte aligned (pointers, or an odd "
              "member_stride=%lld)", align, (long long)member_stride);
  WB2_REQUIRE(plan && ens && truth && circumference && sums && cnt,
              "null pointer argument");
  WB2_REQUIRE(n_outer <= (1ll << 40) / n_row,
              "the grid does not fit: %lld outer indices of %d rows",
              (long long)n_outer, (int)n_row);
  int plan_dtype = 0, plan_n_lon = 0;
  void* tables = spectrum_plan_tables(plan, &plan_dtype, &plan_n_lon);
  WB2_REQUIRE(tables && plan_dtype == dtype && plan_n_lon == n_col,
              "the plan (dtype %d, n_lon=%d%s) does not serve dtype %d, "
              "n_col=%d", plan_dtype, plan_n_lon,
              tables ? "" : ", no twiddle tables", dtype, (int)n_col);
  cross::CrossParams p{};
  p.ens = ens;
  p.truth = truth;
  const int n2 = n_col / 2;
  p.twz = tables;
  p.twq = static_cast<char*>(tables) + (size_t)n2 * (size_t)align;
  p.ens_slab = reinterpret_cast<const long long*>(ens_slab);
  p.truth_slab = reinterpret_cast<const long long*>(truth_slab);
  p.circ = circumference;
  p.sums = sums;
  p.cnt = cnt;
  p.member_stride = member_stride;
  p.n_rows = (long long)n_outer * n_row;
  p.n_member = n_member;
  p.n_row = n_row;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (n2) {
#define WB2_CASE(N2)                                                  \
  case N2:                                                            \
    return dtype == WB2_F32 ? cross::launch<N2, float>(p, s)          \
                            : cross::launch<N2, double>(p, s);
    WB2_FFT_PLAN_SIZES(WB2_CASE)
#undef WB2_CASE
  }
  return fail("cross-spectrum: n_col=%d is not instantiated", (int)n_col);
}

}  // extern "C"
