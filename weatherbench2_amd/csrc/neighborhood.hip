// K19 of libwb2hip.so: neighbourhood verification, the sufficient statistics
// of the fractions skill score (Roberts & Lean 2008).  The reference has no
// counterpart.
//
//   wb2_event_codes  code[t][o][i][j] (uint16) = k | obs << 8 | invalid << 9
//                    of every point under threshold t: the per-point compare
//                    of event_common.hpp, stored where K18 counts it
//   wb2_fss_sums     sums[cell][window][i][c][6] (int64): over the valid
//                    centres j of class c in row i, with F = the window sum of
//                    k and O = n_member * the window sum of obs,
//                    (F-O)^2, F^2, O^2, F, O and the number of centres
//   wb2_fss_fold     table[cell][window][r][q] = sum_i w[window][g(q)][r][i] *
//                    (double)(sum_c mult[r][c] * sums[cell][window][i][c][q])
//
// A window of centre (i, j) and odd size n = 2 h + 1 is the rows max(0, i - h)
// .. min(n_row - 1, i + h) (clipped at the poles) and the columns (j - h .. j +
// h) mod n_col (longitude is cyclic).  An invalid point (truth or a member NaN)
// has k = obs = 0, stays in the windows and is left out as a centre.
//
// The box sum: a workgroup of 256 threads owns one cell and a run of
// kFssRows rows at full row width; thread t owns the ceil(n_col / 256)
// adjacent columns from t * that on.  Per window it keeps the vertical running
// sum of every column in LDS, k in the low and obs in the high half of one
// word (k <= 128 * 255, obs <= 255: neither half overflows or borrows), adds
// the entering row and subtracts the leaving one, re-read from the code plane
// (2 bytes per point: it stays in the caches).  An inclusive scan of the row
// of running sums (per thread, then over the workgroup) in LDS makes every
// horizontal window two reads; the cyclic wrap is an index and a multiple of
// the row total, in arithmetic mod 2^32 (a window sum is below 2^24).  The six
// sums of a thread's columns go to the LDS sums [window][class][6] through a
// wave reduction where the columns of a wave are one class and through 64-bit
// integer LDS adds otherwise; after a barrier they are stored with plain
// stores.  Integers only, no global atomics, no float: two runs are bit-equal.
// Up to kFssWin windows are served from the same walk.

#include <cstdint>

#include "common.hpp"
#include "event_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kFssThreads = 256;
constexpr int kFssWaves = kFssThreads / kWave;
constexpr int kFssMaxWindow = 255;
constexpr int kFssWin = 4;       // windows served from one walk
constexpr int kFssRows = 32;     // rows of one workgroup
constexpr int kFssSums = 6;
constexpr long long kFssLds = 160 * 1024;  // bytes of LDS of one workgroup

constexpr unsigned kCodeObs = 0x100u, kCodeInvalid = 0x200u;

// ---------------------------------------------------------------------------
// wb2_event_codes
// ---------------------------------------------------------------------------
constexpr char kCodeTakes[] = "the event codes take";

struct CodeParams : ExceedOperands {
  uint16_t* code;               // the first threshold of this launch
  long long code_thr_stride;    // codes of one threshold
  long long slab;
};

template <int VEC>
__device__ __forceinline__ void store_codes(uint16_t* p,
                                            const uint16_t (&c)[VEC]) {
  if constexpr (VEC == 1) {
    *p = c[0];
  } else {
    typedef uint16_t V __attribute__((ext_vector_type(VEC)));
    V x;
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[v] = c[v];
    *reinterpret_cast<V*>(p) = x;  // (read again by wb2_fss_sums: cached)
  }
}

// One thread per VEC adjacent points of one slab: exceed_points(), with the
// code stored.
template <typename T, int VEC, int NT>
__global__ void __launch_bounds__(kFssThreads)
    event_codes_kernel(const CodeParams p) {
  const long long o = outer_index();
  const long long e =
      ((long long)blockIdx.x * kFssThreads + threadIdx.x) * VEC;
  // (VEC divides the slab on the wide path: a lane never leaves it)
  if (o >= p.n_outer || e >= p.slab) return;
  int k[NT][VEC];
  bool obs[NT][VEC], bad[VEC];
  const T* xe = exceed_slab<T>(p.ens, p.ens_slab, o, p.slab, e);
  T tv[VEC], hv[NT][VEC];
  // (the truth is requested before the thresholds' slabs are resolved)
  load_v<T, VEC>(exceed_slab<T>(p.truth, p.truth_slab, o, p.slab, e), tv);
#pragma unroll
  for (int t = 0; t < NT; ++t)
    load_v<T, VEC>(exceed_slab<T>(p.thr[t], p.thr_slab[t], o, p.slab, e),
                   hv[t]);
  exceed_points<T, VEC, NT>(xe, p.member_stride, p.n_member, tv, hv, k, obs,
                            bad);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    uint16_t c[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      c[v] = (uint16_t)(bad[v] ? kCodeInvalid
                               : (unsigned)k[t][v] |
                                     (obs[t][v] ? kCodeObs : 0u));
    store_codes<VEC>(p.code + t * p.code_thr_stride + o * p.slab + e, c);
  }
}

// ---------------------------------------------------------------------------
// wb2_fss_sums
// ---------------------------------------------------------------------------
struct FssParams {
  const uint16_t* code;    // [n_cell][n_row][n_col]
  const int* col_class;    // [n_col]
  long long* sums;         // the first window of this launch
  long long cell_stride;   // sums of one cell (all windows of the call)
  long long n_cell;
  int half[kFssWin];       // h of the windows of this launch
  int n_member, n_row, n_col, n_class;
};

// k in the low half, obs in the high half; an invalid point has neither
__device__ __forceinline__ unsigned pack_code(unsigned c) {
  return (c & 0xffu) | ((c & kCodeObs) << 8);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(
    unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

inline long long fss_lds_bytes(int nw, int n_col, int n_class) {
  // sums (8 B), scanned (k, obs) pairs (8 B), running sums (4 B), wave totals
  return (long long)nw * ((long long)n_class * kFssSums * 8 +
                          (long long)n_col * 12) +
         (long long)kFssWin * kFssWaves * 2 * 4;
}

template <int NW>
__global__ void __launch_bounds__(kFssThreads)
    fss_sums_kernel(const FssParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fss_lds[];
  const long long cell = outer_index();
  if (cell >= p.n_cell) return;  // (the whole workgroup)
  const int n_col = p.n_col, n_row = p.n_row, n_class = p.n_class;
  const unsigned M = (unsigned)p.n_member;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n_acc = NW * n_class * kFssSums;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(fss_lds);
  uint2* scan = reinterpret_cast<uint2*>(acc + n_acc);       // [NW][n_col]
  unsigned* run = reinterpret_cast<unsigned*>(scan + (long long)NW * n_col);
  unsigned* wtot = run + (long long)NW * n_col;              // [NW][waves][2]

  const int chunk = (n_col + kFssThreads - 1) / kFssThreads;
  const int j0 = tid * chunk < n_col ? tid * chunk : n_col;
  const int j1 = j0 + chunk < n_col ? j0 + chunk : n_col;
  const int row0 = (int)blockIdx.x * kFssRows;
  const int row1 = row0 + kFssRows < n_row ? row0 + kFssRows : n_row;
  const uint16_t* __restrict__ plane = p.code + cell * n_row * n_col;
  const int* __restrict__ cls = p.col_class;
  for (int a = tid; a < n_acc; a += kFssThreads) acc[a] = 0;

  // Are the columns of this wave one class?  (Lane 0 has columns if any lane
  // of the wave has; a lane without columns agrees with every class.)
  int mine = -1;
  bool single = true;
  for (int j = j0; j < j1; ++j) {
    const int c = cls[j];
    single = single && (mine < 0 || c == mine);
    if (mine < 0) mine = c;
  }
  const int wave_class = __shfl(mine, 0, kWave);
  const bool uniform = __all(single && (mine < 0 || mine == wave_class));

  for (int i = row0; i < row1; ++i) {
    // 1. the vertical running sums of the own columns, and their totals
    unsigned tk[NW], to[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) tk[w] = to[w] = 0;
    if (i == row0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const int h = p.half[w];
        unsigned* vrun = run + (long long)w * n_col;
        const int lo = i - h > 0 ? i - h : 0;
        const int hi = i + h < n_row - 1 ? i + h : n_row - 1;
        for (int j = j0; j < j1; ++j) {
          unsigned v = 0;
#pragma unroll 4
          for (int r = lo; r <= hi; ++r)
            v += pack_code(plane[(long long)r * n_col + j]);
          vrun[j] = v;
          tk[w] += v & 0xffffu;
          to[w] += v >> 16;
        }
      }
    } else {
      // (a row outside the grid neither enters nor leaves: it is read as the
      // centre row and masked, so that the loads of a column's windows are
      // requested together)
      const uint16_t* in[NW];
      const uint16_t* out[NW];
      unsigned min_[NW], mout[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const int h = p.half[w];
        const bool enter = i + h <= n_row - 1, leave = i - h - 1 >= 0;
        in[w] = plane + (long long)(enter ? i + h : i) * n_col;
        out[w] = plane + (long long)(leave ? i - h - 1 : i) * n_col;
        min_[w] = enter ? 0xffffffffu : 0u;
        mout[w] = leave ? 0xffffffffu : 0u;
      }
#pragma unroll 2
      for (int j = j0; j < j1; ++j) {
        unsigned cin[NW], cout[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          cin[w] = in[w][j];
          cout[w] = out[w][j];
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          unsigned* vrun = run + (long long)w * n_col;
          const unsigned v = vrun[j] + (pack_code(cin[w]) & min_[w]) -
                             (pack_code(cout[w]) & mout[w]);
          vrun[j] = v;
          tk[w] += v & 0xffffu;
          to[w] += v >> 16;
        }
      }
    }
    // 2. the scan of the thread totals: over the wave, then over the waves
    unsigned ik[NW], io[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      ik[w] = tk[w];
      io[w] = to[w];
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const unsigned a = __shfl_up(ik[w], off, kWave);
        const unsigned b = __shfl_up(io[w], off, kWave);
        if (lane >= off) {
          ik[w] += a;
          io[w] += b;
        }
      }
      if (lane == kWave - 1) {
        wtot[(w * kFssWaves + wave) * 2] = ik[w];
        wtot[(w * kFssWaves + wave) * 2 + 1] = io[w];
      }
    }
    __syncthreads();
    // 3. the inclusive scan of the row, as (k, obs) pairs
    unsigned totk[NW], toto[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      unsigned pk = ik[w] - tk[w], po = io[w] - to[w];
      totk[w] = toto[w] = 0;
#pragma unroll
      for (int v = 0; v < kFssWaves; ++v) {
        const unsigned a = wtot[(w * kFssWaves + v) * 2];
        const unsigned b = wtot[(w * kFssWaves + v) * 2 + 1];
        if (v < wave) {
          pk += a;
          po += b;
        }
        totk[w] += a;
        toto[w] += b;
      }
      const unsigned* vrun = run + (long long)w * n_col;
      uint2* vscan = scan + (long long)w * n_col;
      for (int j = j0; j < j1; ++j) {
        const unsigned v = vrun[j];
        pk += v & 0xffffu;
        po += v >> 16;
        vscan[j] = make_uint2(pk, po);
      }
    }
    __syncthreads();
    // 4. the windows of the own valid centres
    unsigned long long q[NW][kFssSums];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int s = 0; s < kFssSums; ++s) q[w][s] = 0;
    int cur = -1;
    // the invalid centres among the own columns, requested together (a thread
    // owns at most 64 columns: the LDS budget admits no row beyond 13 638)
    const uint16_t* centre = plane + (long long)i * n_col;
    unsigned long long invalid = 0;
#pragma unroll 4
    for (int j = j0; j < j1; ++j)
      invalid |= (unsigned long long)((centre[j] >> 9) & 1u) << (j - j0);
    for (int j = j0; j < j1; ++j) {
      if (!uniform) {
        const int c = cls[j];
        if (c != cur) {
          if (cur >= 0) {
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
              for (int s = 0; s < kFssSums; ++s) {
                __hip_atomic_fetch_add(
                    &acc[(w * n_class + cur) * kFssSums + s], q[w][s],
                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                q[w][s] = 0;
              }
          }
          cur = c;
        }
      }
      if ((invalid >> (j - j0)) & 1) continue;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const int h = p.half[w];
        const uint2* vscan = scan + (long long)w * n_col;
        const int a = j + h, b = j - h - 1;
        const uint2 pa = vscan[a >= n_col ? a - n_col : a];
        const uint2 pb = vscan[b < 0 ? b + n_col : b];
        // P(a) = P[a - n_col] + total past the end, P(b) = P[b + n_col] -
        // total before the start (P(-1) = 0 among them), all mod 2^32
        const unsigned turns = (a >= n_col ? 1u : 0u) + (b < 0 ? 1u : 0u);
        const unsigned F = pa.x - pb.x + turns * totk[w];
        const unsigned O = (pa.y - pb.y + turns * toto[w]) * M;
        const long long d = (long long)F - (long long)O;
        q[w][0] += (unsigned long long)(d * d);
        q[w][1] += (unsigned long long)F * F;
        q[w][2] += (unsigned long long)O * O;
        q[w][3] += F;
        q[w][4] += O;
        q[w][5] += 1;
      }
    }
    if (uniform) {
      if (wave_class >= 0) {
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
          for (int s = 0; s < kFssSums; ++s) {
            const unsigned long long v = wave_sum_u64(q[w][s]);
            if (lane == 0)
              __hip_atomic_fetch_add(
                  &acc[(w * n_class + wave_class) * kFssSums + s], v,
                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
      }
    } else if (cur >= 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int s = 0; s < kFssSums; ++s)
          __hip_atomic_fetch_add(&acc[(w * n_class + cur) * kFssSums + s],
                                 q[w][s], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    // 5. the sums of the row leave, and are zero for the next row (whose adds
    // come two barriers later)
    const int row_sums = n_class * kFssSums;
    long long* dst = p.sums + cell * p.cell_stride + (long long)i * row_sums;
    for (int a = tid; a < n_acc; a += kFssThreads) {
      const int w = a / row_sums;
      dst[(long long)w * n_row * row_sums + (a - w * row_sums)] =
          (long long)acc[a];
      acc[a] = 0;
    }
  }
}

struct FssGeometry {
  int windows_per_launch;
  long long lds_bytes;
};

// The most windows per launch that fit the budget (they share the walk).
// False: not even one window fits.
inline bool fss_geometry(int n_col, int n_class, int n_window,
                         FssGeometry* g) {
  const int nw_max = n_window < kFssWin ? n_window : kFssWin;
  for (int nw = nw_max; nw >= 1; --nw)
    if (fss_lds_bytes(nw, n_col, n_class) <= kFssLds) {
      *g = {nw, fss_lds_bytes(nw, n_col, n_class)};
      return true;
    }
  return false;
}

#define WB2_REQUIRE_FSS_SHAPE(n_col, n_class, n_window, g)                     \
  do {                                                                         \
    WB2_REQUIRE(n_class >= 1 && n_class <= kExceedMaxClass,                    \
                "n_class=%d: the fractions sums take 1 to %d column classes",  \
                (int)n_class, kExceedMaxClass);                                \
    WB2_REQUIRE(n_window >= 1, "n_window=%d", (int)n_window);                  \
    WB2_REQUIRE(n_col >= 0, "n_col=%d is negative", (int)n_col);               \
    WB2_REQUIRE(fss_geometry(n_col, n_class, n_window, &g),                    \
                "a row of %d columns and %d classes does not fit the LDS "     \
                "budget of %lld bytes", (int)n_col, (int)n_class, kFssLds);    \
  } while (0)

template <typename F>
hipError_t allow_lds(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kFssLds);
}

// ---------------------------------------------------------------------------
// wb2_fss_fold
// ---------------------------------------------------------------------------
struct FssFoldParams {
  const long long* sums;  // [n_cell][n_window][n_row][n_class][6]
  const double* w;        // [n_window][3][n_region][n_row]
  const int* mult;        // [n_region][n_class]
  double* table;          // [n_cell][n_window][n_region][6]
  long long n_unit;       // n_cell * n_window * n_region
  int n_window, n_row, n_class, n_region;
};

__device__ __forceinline__ double lane_value(double v, int lane) {
  // (lane is the same in every lane: a read of one lane, no LDS)
  return __hiloint2double(
      __builtin_amdgcn_readlane(__double2hiint(v), lane),
      __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// One WAVE per (cell, window, region) and all six sums of it: lane l takes
// row i0 + l of a block of 64 rows -- its 48 contiguous bytes of every class,
// the integer sums over the classes and the six products g * (double)s -- and
// the wave then adds the products of the block to the six accumulators lane
// by lane, that is in increasing row order: acc = acc + g * s as one thread
// would.  The integer work and the loads are spread over the lanes; the float
// sum keeps its order.
__global__ void __launch_bounds__(kFssThreads)
    fss_fold_kernel(const FssFoldParams p) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long unit =
      (long long)blockIdx.x * kFssWaves + threadIdx.x / kWave;
  if (unit >= p.n_unit) return;  // (the whole wave; no barrier below)
  const int r = (int)(unit % p.n_region);
  const long long cw = unit / p.n_region;  // cell * n_window + window
  const int win = (int)(cw % p.n_window);
  const long long* __restrict__ sums =
      p.sums + cw * p.n_row * p.n_class * kFssSums;
  const int* __restrict__ mult = p.mult + (long long)r * p.n_class;
  const double* __restrict__ w =
      p.w + ((long long)win * 3 * p.n_region + r) * p.n_row;
  const long long group_stride = (long long)p.n_region * p.n_row;
  double acc[kFssSums];
#pragma unroll
  for (int q = 0; q < kFssSums; ++q) acc[q] = 0.0;
  for (int i0 = 0; i0 < p.n_row; i0 += kWave) {
    const int i = i0 + lane;
    double prod[kFssSums];
#pragma unroll
    for (int q = 0; q < kFssSums; ++q) prod[q] = 0.0;
    if (i < p.n_row) {
      long long s[kFssSums] = {};
      const long long* row = sums + (long long)i * p.n_class * kFssSums;
#pragma unroll 2
      for (int c = 0; c < p.n_class; ++c) {
        const long long m = mult[c];
#pragma unroll
        for (int q = 0; q < kFssSums; ++q) s[q] += m * row[c * kFssSums + q];
      }
      const double g2 = w[i], g1 = w[group_stride + i],
                   g0 = w[2 * group_stride + i];
#pragma unroll
      for (int q = 0; q < kFssSums; ++q)
        prod[q] = (q < 3 ? g2 : q < 5 ? g1 : g0) * (double)s[q];
    }
    const int n = p.n_row - i0 < kWave ? p.n_row - i0 : kWave;
    for (int l = 0; l < n; ++l)
#pragma unroll
      for (int q = 0; q < kFssSums; ++q) acc[q] += lane_value(prod[q], l);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kFssSums; ++q) p.table[unit * kFssSums + q] = acc[q];
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_event_codes(int dtype, const void* ens, const int64_t* ens_slab,
                    const void* truth, const int64_t* truth_slab,
                    const void* const* threshold, const int64_t* thr_slab,
                    int32_t n_threshold, int32_t n_member,
                    int64_t member_stride, int64_t n_outer, int32_t n_row,
                    int32_t n_col, uint16_t* code, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  if (const int rc = exceed_shape(kCodeTakes, dtype, n_member, n_threshold))
    return rc;
  CodeParams p{};
  const int go = exceed_operands(ens, ens_slab, truth, truth_slab, threshold,
                                 n_threshold, n_member, member_stride, n_outer,
                                 n_row, n_col, &p);
  if (go <= 0) return go;
  WB2_REQUIRE(code, "null pointer argument");
  const bool wide = aligned16(code) &&
                    exceed_wide(dtype, ens, truth, threshold, n_threshold,
                                n_col, member_stride);
  p.slab = (long long)n_row * n_col;
  p.code_thr_stride = (long long)n_outer * p.slab;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_outer,
                         point_tiles(p.slab, wide ? wide_lanes(dtype) : 1,
                                     kFssThreads), &grid),
              "the grid does not fit: %lld outer indices of %lld points",
              (long long)n_outer, p.slab);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return exceed_batches(
      &p, threshold, thr_slab, n_threshold, kExceedThr, [&](int t0, int nt) {
        p.code = code + t0 * p.code_thr_stride;
        for_exceed(dtype, wide, nt, [&](auto T0, auto V, auto NT) {
          hipLaunchKernelGGL(
              (event_codes_kernel<decltype(T0), decltype(V)::value,
                                  decltype(NT)::value>),
              grid, dim3(kFssThreads), 0, s, p);
        });
      });
}

int wb2_fss_sums_geometry(int32_t n_col, int32_t n_class, int32_t n_window,
                          int32_t* rows_per_group,
                          int32_t* windows_per_launch, int64_t* lds_bytes,
                          int32_t* max_grid_outer) {
  using namespace wb2;
  FssGeometry g;
  WB2_REQUIRE_FSS_SHAPE(n_col, n_class, n_window, g);
  WB2_REQUIRE(rows_per_group && windows_per_launch && lds_bytes &&
              max_grid_outer, "null pointer argument");
  *rows_per_group = kFssRows;
  *windows_per_launch = g.windows_per_launch;
  *lds_bytes = g.lds_bytes;
  *max_grid_outer = (int32_t)kGridOuter;
  return 0;
}

int wb2_fss_sums(const uint16_t* code, int64_t n_cell, int32_t n_row,
                 int32_t n_col, int32_t n_member, const int32_t* window,
                 int32_t n_window, const int32_t* col_class, int32_t n_class,
                 int64_t* sums, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(n_member >= 1 && n_member <= kExceedMaxMember,
              "n_member=%d: the fractions sums take 1 to %d members",
              (int)n_member, kExceedMaxMember);
  FssGeometry g;
  WB2_REQUIRE_FSS_SHAPE(n_col, n_class, n_window, g);
  WB2_EMPTY_OK(n_cell);
  WB2_EMPTY_OK(n_row);
  WB2_EMPTY_OK(n_col);
  WB2_REQUIRE(code && window && col_class && sums, "null pointer argument");
  for (int w = 0; w < n_window; ++w)
    WB2_REQUIRE(window[w] >= 1 && window[w] <= kFssMaxWindow &&
                    window[w] % 2 == 1 && window[w] <= n_col,
                "window=%d: a window is odd, 1 to %d and at most n_col=%d",
                (int)window[w], kFssMaxWindow, (int)n_col);
  const long long groups = ((long long)n_row + kFssRows - 1) / kFssRows;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_cell, groups, &grid),
              "the grid does not fit: %lld cells of %lld row groups",
              (long long)n_cell, groups);
  if (g.lds_bytes > 64 * 1024) {
    // (once per PROCESS, as in quantile.hip: the attribute belongs to the
    // function of the device that is current at the first such call, which is
    // every call's device in a one-GPU process; a process that drives several
    // GPUs would have to set it once per device)
    static const hipError_t allowed = [] {
      hipError_t e = allow_lds(fss_sums_kernel<1>);
      if (e == hipSuccess) e = allow_lds(fss_sums_kernel<2>);
      if (e == hipSuccess) e = allow_lds(fss_sums_kernel<3>);
      if (e == hipSuccess) e = allow_lds(fss_sums_kernel<4>);
      return e;
    }();
    WB2_HIP_OK(allowed);
  }
  FssParams p{};
  p.code = code;
  p.col_class = col_class;
  p.cell_stride = (long long)n_window * n_row * n_class * kFssSums;
  p.n_cell = n_cell;
  p.n_member = n_member;
  p.n_row = n_row;
  p.n_col = n_col;
  p.n_class = n_class;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // more windows than one walk serves: further launches
  for (int w0 = 0; w0 < n_window; w0 += g.windows_per_launch) {
    const int nw = n_window - w0 < g.windows_per_launch
                       ? n_window - w0 : g.windows_per_launch;
    for (int w = 0; w < kFssWin; ++w)
      p.half[w] = w < nw ? window[w0 + w] / 2 : 0;
    p.sums = reinterpret_cast<long long*>(sums) +
             (long long)w0 * n_row * n_class * kFssSums;
    const size_t lds = (size_t)fss_lds_bytes(nw, n_col, n_class);
#define WB2_L(NW)                                                     \
  hipLaunchKernelGGL((fss_sums_kernel<NW>), grid, dim3(kFssThreads),  \
                     lds, s, p)
    switch (nw) {
      case 1: WB2_L(1); break;
      case 2: WB2_L(2); break;
      case 3: WB2_L(3); break;
      default: WB2_L(4); break;
    }
#undef WB2_L
    WB2_HIP_OK(hipGetLastError());
  }
  return 0;
}

int wb2_fss_fold(const int64_t* sums, int64_t n_cell, int32_t n_window,
                 int32_t n_row, int32_t n_class, const double* w,
                 const int32_t* mult, int32_t n_region, double* table,
                 void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(n_row >= 0 && n_class >= 1,
              "bad sizes: %d rows, n_class=%d", (int)n_row, (int)n_class);
  WB2_EMPTY_OK(n_cell);
  WB2_EMPTY_OK(n_window);
  WB2_EMPTY_OK(n_region);
  WB2_REQUIRE(table && (n_row == 0 || (sums && w && mult)),
              "null pointer argument");
  FssFoldParams p{};
  p.sums = reinterpret_cast<const long long*>(sums);
  p.w = w;
  p.mult = mult;
  p.table = table;
  p.n_unit = (long long)n_cell * n_window * n_region;
  p.n_window = n_window;
  p.n_row = n_row;
  p.n_class = n_class;
  p.n_region = n_region;
  const long long blocks = (p.n_unit + kFssWaves - 1) / kFssWaves;
  WB2_REQUIRE(blocks < (1ll << 31), "the grid does not fit: %lld waves",
              p.n_unit);
  hipLaunchKernelGGL(fss_fold_kernel, dim3((unsigned)blocks),
                     dim3(kFssThreads), 0, static_cast<hipStream_t>(stream),
                     p);
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
