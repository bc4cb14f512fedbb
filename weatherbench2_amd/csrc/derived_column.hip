// K9 of libwb2hip.so: derived variables that walk the `level` axis of a grid
// column (weatherbench2/derived_variables.py).
//
//   wb2_derived_column      TotalColumnWater :365-385, IntegratedWaterTransport
//                           :388-430, LapseRate :341-362, the vertical integral
//                           of VerticalVelocity :179-209, EddyKineticEnergy
//                           :212-228
//   wb2_derived_zonal_mean  the NaN-skipping zonal means EddyKineticEnergy
//                           subtracts
//
// A chunk is (..., level, latitude, longitude): consecutive levels of a column
// lie a whole slab apart.  A thread owns VEC adjacent points of the contiguous
// inner block and walks the levels; level l of column c of an input starts
// `table[c][l] * n_point` elements after its base, so contiguous tensors,
// strided views of whole slabs and gathers are read where they lie.  A launch
// has only a few workgroups per CU, so the bytes in flight come from
// kColumnAhead levels requested per thread before any is consumed.
//
// Arithmetic in the dtype NumPy would use (-ffp-contract=off): np.trapezoid
// forms y[k+1] + y[k] in the field's dtype T, multiplies by the spacing in the
// promoted dtype O and halves; the sum over levels is kept in float64 and
// rounded to O once.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

constexpr int kColumnThreads = 256;
constexpr int kColumnAhead = 4;  // levels loaded before any is combined

struct ColumnParams {
  // INTEGRAL: 0 = the field.  TRANSPORT: 0 = water species, 1 = u, 2 = v.
  // GRADIENT_RATIO: 0 = numerator field, 1 = denominator field.
  // EDDY: 0 = u, 1 = v, 2 / 3 = their zonal means [n_column][n_level][n_mean].
  // CUMULATIVE: none (in place on `out`, addressed through slab[0]).
  const void* in[4];
  const long long* slab[3];  // [n_column][n_level] each
  const double* spacing;     // [n_level - 1]: x[l + 1] - x[l]
  const double* coef;        // [4][n_level]: a, b, c, den of d/d(level)
  void* out;
  long long n_column, n_point, mean_div;
  int n_level, l0, l1, uniform, n_mean;
  double scale;
};

// INTEGRAL / TRANSPORT / EDDY: out[c][point] of dtype O
template <typename T, typename O, int VEC, int MODE>
__global__ void __launch_bounds__(kColumnThreads)
    column_integral_kernel(const ColumnParams p) {
  const long long q =
      ((long long)blockIdx.x * kColumnThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long c = outer_index();
  if (c >= p.n_column) return;
  constexpr int NIN = MODE == WB2_COLUMN_INTEGRAL ? 1
                      : MODE == WB2_COLUMN_TRANSPORT ? 3 : 2;
  constexpr int NACC = MODE == WB2_COLUMN_TRANSPORT ? 2 : 1;
  constexpr int U = kColumnAhead;
  const T* in[NIN];
  const long long* slab[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    in[i] = static_cast<const T*>(p.in[i]) + q;
    slab[i] = p.slab[i] + c * p.n_level;
  }
  int mean_at[VEC];
  if constexpr (MODE == WB2_COLUMN_EDDY) {
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      mean_at[e] = (int)(((q + e) / p.mean_div) % p.n_mean);
  }
  double acc[NACC][VEC];
  T prev[NACC][VEC];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[a][e] = 0.0;
      prev[a][e] = T(0);
    }
  // (fewer than two selected levels: np.trapezoid sums nothing, 0.0 even where
  // the field is NaN; nothing is read)
  const int l0 = p.l0, l1 = p.l1 - p.l0 < 2 ? p.l0 : p.l1;
  for (int lb = l0; lb < l1; lb += U) {
    T cur[U][NIN][VEC];
    T bar[U][2][VEC];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      // (levels past the end are read from the last one and dropped)
      const int l = min(lb + k, l1 - 1);
#pragma unroll
      for (int i = 0; i < NIN; ++i)
        load_v<T, VEC>(in[i] + slab[i][l] * p.n_point, cur[k][i]);
      if constexpr (MODE == WB2_COLUMN_EDDY) {
        const long long row = (c * p.n_level + l) * p.n_mean;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          bar[k][0][e] = static_cast<const T*>(p.in[2])[row + mean_at[e]];
          bar[k][1][e] = static_cast<const T*>(p.in[3])[row + mean_at[e]];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int l = lb + k;
      if (l >= l1) break;
      const O d = l > l0 ? (O)p.spacing[l - 1] : O(0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        T f[NACC];
        if constexpr (MODE == WB2_COLUMN_INTEGRAL) {
          f[0] = cur[k][0][e];
        } else if constexpr (MODE == WB2_COLUMN_TRANSPORT) {
          f[0] = cur[k][0][e] * cur[k][1][e];
          f[1] = cur[k][0][e] * cur[k][2][e];
        } else {
          const T du = cur[k][0][e] - bar[k][0][e];
          const T dv = cur[k][1][e] - bar[k][1][e];
          const T uu = du * du;
          const T vv = dv * dv;
          f[0] = uu + vv;
        }
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
          if (l > l0) {
            const T s = f[a] + prev[a][e];
            const O term = (d * (O)s) / O(2);
            acc[a][e] += (double)term;
          }
          prev[a][e] = f[a];
        }
      }
    }
  }
  O r[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    if constexpr (MODE == WB2_COLUMN_TRANSPORT) {
      const O iu = (O)acc[0][e], iv = (O)acc[1][e];
      const O uu = iu * iu;
      const O vv = iv * iv;
      r[e] = (O)p.scale * sqrt_rn(uu + vv);
    } else {
      r[e] = (O)p.scale * (O)acc[0][e];
    }
  }
  store_v<O, VEC>(static_cast<O*>(p.out) + c * p.n_point + q, r);
}

// GRADIENT_RATIO: out[c][l][point] of dtype T, a three-level window of both
// fields in registers
template <typename T, int VEC>
__global__ void __launch_bounds__(kColumnThreads)
    column_gradient_ratio_kernel(const ColumnParams p) {
  const long long q =
      ((long long)blockIdx.x * kColumnThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long c = outer_index();
  if (c >= p.n_column) return;
  constexpr int U = kColumnAhead;
  const int n_level = p.n_level;
  const T* a = static_cast<const T*>(p.in[0]) + q;
  const T* b = static_cast<const T*>(p.in[1]) + q;
  const long long* sa = p.slab[0] + c * n_level;
  const long long* sb = p.slab[1] + c * n_level;
  T* out = static_cast<T*>(p.out) + c * n_level * p.n_point + q;
  const T scale = (T)p.scale;
  // levels l - 1 ... l + U of both fields: the window rolls down the column
  T wa[U + 2][VEC], wb[U + 2][VEC];
  load_v<T, VEC>(a + sa[0] * p.n_point, wa[1]);
  load_v<T, VEC>(b + sb[0] * p.n_point, wb[1]);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    wa[0][e] = wa[1][e];
    wb[0][e] = wb[1][e];
  }
  for (int lb = 0; lb < n_level; lb += U) {
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int l = min(lb + k + 1, n_level - 1);
      load_v<T, VEC>(a + sa[l] * p.n_point, wa[k + 2]);
      load_v<T, VEC>(b + sb[l] * p.n_point, wb[k + 2]);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int l = lb + k;
      if (l >= n_level) break;
      const bool diff = p.uniform || l == 0 || l == n_level - 1;
      const double ca = diff ? 0.0 : p.coef[l];
      const double cb = diff ? 0.0 : p.coef[n_level + l];
      const double cc = diff ? 0.0 : p.coef[2 * n_level + l];
      const double den = p.coef[3 * n_level + l];
      T r[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const T ga = gradient_at<T>(wa[k][e], wa[k + 1][e], wa[k + 2][e], diff,
                                    ca, cb, cc, den);
        const T gb = gradient_at<T>(wb[k][e], wb[k + 1][e], wb[k + 2][e], diff,
                                    ca, cb, cc, den);
        const T below = scale * gb;
        r[e] = ga / below;
      }
      store_v<T, VEC>(out + (long long)l * p.n_point, r);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      wa[0][e] = wa[U][e];
      wa[1][e] = wa[U + 1][e];
      wb[0][e] = wb[U][e];
      wb[1][e] = wb[U + 1][e];
    }
  }
}

// CUMULATIVE: scipy's cumulative_trapezoid(-field, initial=0) down the levels,
// in place on a float64 field.  A thread reads a level of its own points
// before it writes it, and no other thread touches them.
template <int VEC>
__global__ void __launch_bounds__(kColumnThreads)
    column_cumulative_kernel(const ColumnParams p) {
  const long long q =
      ((long long)blockIdx.x * kColumnThreads + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long c = outer_index();
  if (c >= p.n_column) return;
  constexpr int U = kColumnAhead;
  const int n_level = p.n_level;
  double* field = static_cast<double*>(p.out) + q;
  const long long* slab = p.slab[0] + c * n_level;
  double acc[VEC], prev[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = prev[e] = 0.0;
  for (int lb = 0; lb < n_level; lb += U) {
    double cur[U][VEC];
#pragma unroll
    for (int k = 0; k < U; ++k)
      load_v<double, VEC>(field + slab[min(lb + k, n_level - 1)] * p.n_point,
                          cur[k]);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int l = lb + k;
      if (l >= n_level) break;
      const double d = l > 0 ? p.spacing[l - 1] : 0.0;
      double r[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double y = -cur[k][e];
        if (l > 0) {
          const double s = y + prev[e];
          acc[e] += (d * s) / 2.0;
        }
        prev[e] = y;
        r[e] = acc[e];  // (0.0 at the first level whatever the field holds)
      }
      store_v<double, VEC>(field + slab[l] * p.n_point, r);
    }
  }
}

// NaN-skipping mean over longitude of every (slab, latitude): float64 sum and
// count, rounded to T (0 / 0 = NaN where a circle has no finite point).
// LAT_ROWS: rows are latitudes, one wave sums a row; otherwise columns are
// latitudes, one thread walks down a column.
template <typename T, bool LAT_ROWS>
__global__ void __launch_bounds__(256) zonal_mean_kernel(
    const T* in, const long long* slab, long long n_slab, int n_row, int n_col,
    T* out) {
  if constexpr (LAT_ROWS) {
    const long long row =
        ((long long)blockIdx.x * 256 + threadIdx.x) / kWave;  // (slab, lat)
    if (row >= n_slab * n_row) return;
    const long long o = row / n_row;
    const T* x = in + ((slab ? slab[o] : o) * n_row + row % n_row) * n_col;
    double sum = 0.0, count = 0.0;
    for (int j = threadIdx.x % kWave; j < n_col; j += kWave) {
      const T v = x[j];
      if (!is_nan(v)) {
        sum += (double)v;
        count += 1.0;
      }
    }
    sum = wave_allsum(sum);
    count = wave_allsum(count);
    if (threadIdx.x % kWave == 0) out[row] = (T)(sum / count);
  } else {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= n_slab * n_col) return;
    const long long o = at / n_col;
    const T* x = in + (slab ? slab[o] : o) * n_row * n_col + at % n_col;
    double sum = 0.0, count = 0.0;
    for (int i = 0; i < n_row; ++i) {
      const T v = x[(long long)i * n_col];
      if (!is_nan(v)) {
        sum += (double)v;
        count += 1.0;
      }
    }
    out[at] = (T)(sum / count);
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_derived_column_geometry(int dtype, int wide, int32_t* tile_points,
                                int32_t* levels_ahead) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_points && levels_ahead, "null pointer argument");
  *tile_points = kColumnThreads * (wide ? wide_lanes(dtype) : 1);
  *levels_ahead = kColumnAhead;
  return 0;
}

int wb2_derived_column(int mode, int dtype, int out_dtype,
                       const void* const* inputs, const int64_t* const* slabs,
                       int64_t n_column, int32_t n_level, int64_t n_point,
                       int32_t level_begin, int32_t level_end,
                       const double* spacing, const double* level_coef,
                       int level_uniform, int64_t mean_div, int32_t n_mean,
                       double scale, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(out_dtype == WB2_F32 || out_dtype == WB2_F64,
              "unknown dtype %d", out_dtype);
  WB2_REQUIRE(mode >= WB2_COLUMN_INTEGRAL && mode <= WB2_COLUMN_EDDY,
              "unknown mode %d", mode);
  WB2_EMPTY_OK(n_column);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(n_level >= 1 && level_begin >= 0 && level_begin <= level_end &&
                  level_end <= n_level,
              "bad sizes: levels [%d, %d) of %d", (int)level_begin,
              (int)level_end, (int)n_level);
  const bool ratio = mode == WB2_COLUMN_GRADIENT_RATIO;
  const bool cumulative = mode == WB2_COLUMN_CUMULATIVE;
  const int n_in = cumulative ? 0
                   : mode == WB2_COLUMN_INTEGRAL ? 1
                   : mode == WB2_COLUMN_TRANSPORT ? 3 : 2;
  const int n_slab = cumulative ? 1 : n_in;
  WB2_REQUIRE(out && slabs && (cumulative || inputs), "null pointer argument");
  for (int k = 0; k < n_in; ++k)
    WB2_REQUIRE(inputs[k], "null pointer argument");
  for (int k = 0; k < n_slab; ++k)
    WB2_REQUIRE(slabs[k], "null pointer argument");
  WB2_REQUIRE(ratio ? level_coef != nullptr : (n_level < 2 || spacing),
              "null pointer argument");
  // np.gradient needs two points along the axis
  WB2_REQUIRE(!ratio || n_level >= 2, "bad sizes: %d levels", (int)n_level);
  if (mode == WB2_COLUMN_EDDY) {
    WB2_REQUIRE(inputs[2] && inputs[3], "null pointer argument");
    WB2_REQUIRE(mean_div >= 1 && n_mean >= 1, "bad sizes: mean table %lld, %d",
                (long long)mean_div, (int)n_mean);
  }
  WB2_REQUIRE(ratio ? out_dtype == dtype
              : cumulative ? (dtype == WB2_F64 && out_dtype == WB2_F64)
                           : out_dtype >= dtype,
              "out_dtype %d does not fit dtype %d", out_dtype, dtype);
  WB2_REQUIRE((n_point + kColumnThreads - 1) / kColumnThreads < (1ll << 31),
              "bad sizes");
  ColumnParams p{};
  const int w = wide_lanes(dtype);
  bool wide = n_point % w == 0 && aligned16(out);
  for (int k = 0; k < n_in; ++k) {
    p.in[k] = inputs[k];
    wide = wide && aligned16(inputs[k]);
  }
  for (int k = 0; k < n_slab; ++k)
    p.slab[k] = reinterpret_cast<const long long*>(slabs[k]);
  if (mode == WB2_COLUMN_EDDY) {
    p.in[2] = inputs[2];
    p.in[3] = inputs[3];
  }
  p.spacing = spacing;
  p.coef = level_coef;
  p.out = out;
  p.n_column = n_column;
  p.n_point = n_point;
  p.mean_div = mean_div;
  p.n_level = n_level;
  p.l0 = level_begin;
  p.l1 = level_end;
  p.uniform = level_uniform;
  p.n_mean = n_mean;
  p.scale = scale;
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_column,
                         point_tiles(n_point, wide ? w : 1, kColumnThreads),
                         &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kColumnThreads), 0, s, p);
  };
  // the three reducing modes: T the fields' dtype, O the promoted one
  auto integral = [&](auto m) {
    constexpr int M = decltype(m)::value;
    for_field(dtype, wide, [&](auto t, auto v) {
      using T = decltype(t);
      constexpr int V = decltype(v)::value;
      if constexpr (std::is_same<T, double>::value)
        launch(column_integral_kernel<double, double, V, M>);
      else if (out_dtype == WB2_F64)
        launch(column_integral_kernel<float, double, V, M>);
      else
        launch(column_integral_kernel<float, float, V, M>);
    });
  };
  if (mode == WB2_COLUMN_INTEGRAL) {
    integral(std::integral_constant<int, WB2_COLUMN_INTEGRAL>{});
  } else if (mode == WB2_COLUMN_TRANSPORT) {
    integral(std::integral_constant<int, WB2_COLUMN_TRANSPORT>{});
  } else if (mode == WB2_COLUMN_EDDY) {
    integral(std::integral_constant<int, WB2_COLUMN_EDDY>{});
  } else if (ratio) {
    for_field(dtype, wide, [&](auto t, auto v) {
      launch(column_gradient_ratio_kernel<decltype(t), decltype(v)::value>);
    });
  } else {
    if (wide) launch(column_cumulative_kernel<2>);
    else launch(column_cumulative_kernel<1>);
  }
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_derived_zonal_mean(int dtype, int lat_rows, const void* in,
                           const int64_t* slab, int64_t n_slab, int32_t n_row,
                           int32_t n_col, void* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_EMPTY_OK(n_slab);
  WB2_EMPTY_OK(n_row);
  WB2_EMPTY_OK(n_col);
  WB2_REQUIRE(in && out, "null pointer argument");
  const long long n_thread =
      lat_rows ? n_slab * n_row * (long long)kWave : n_slab * (long long)n_col;
  const long long blocks = (n_thread + 255) / 256;
  WB2_REQUIRE(blocks < (1ll << 31), "bad sizes");
  const long long* tab = reinterpret_cast<const long long*>(slab);
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, false, [&](auto t, auto) {
    using T = decltype(t);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                         static_cast<const T*>(in), tab, (long long)n_slab,
                         (int)n_row, (int)n_col, static_cast<T*>(out));
    };
    if (lat_rows) launch(zonal_mean_kernel<T, true>);
    else launch(zonal_mean_kernel<T, false>);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
