// K8 of libwb2hip.so: derived variables that are materialised as one more
// field of a chunk (weatherbench2/derived_variables.py).
//
//   wb2_derived_pointwise  WindSpeed :76-99, RelativeHumidity :433-468
//   wb2_derived_stencil    _d_dx / _d_dy / _divergence / _curl :102-129 and the
//                          geostrophic / ageostrophic winds :231-338
//
// Plain HBM streams.  Elementwise arithmetic in the dtype NumPy would use for
// the reference's expressions (-ffp-contract=off): WindSpeed is three
// correctly rounded operations in the input dtype; np.gradient forms the
// neighbour difference in the input dtype, divides (or weighs) in float64 and
// stores in the input dtype; everything a float64 coordinate enters is float64.
// All per-latitude and per-axis factors are float64 tables made on the host.

#include "common.hpp"
#include "derived_common.hpp"
#include "launch_common.hpp"
#include "trace.hpp"
#include "wb2hip.h"

namespace wb2 {
namespace {

__device__ __forceinline__ float exp_of(float x) { return expf(x); }
__device__ __forceinline__ double exp_of(double x) { return exp(x); }

struct PointParams {
  const void* a;
  const void* b;
  const long long* a_slab;
  const long long* b_slab;
  const void* scalar;  // RelativeHumidity: pressure of slab o, in the out dtype
  void* out;           // [n_slab][n_point]
  long long n_slab, n_point;
};

// grid: x = point blocks, y (z) = slab
template <typename T, int VEC>
__global__ void __launch_bounds__(256) wind_speed_kernel(const PointParams p) {
  const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_slab) return;
  const long long as = p.a_slab ? p.a_slab[o] : o;
  const long long bs = p.b_slab ? p.b_slab[o] : o;
  T u[VEC], v[VEC], r[VEC];
  load_v<T, VEC>(static_cast<const T*>(p.a) + as * p.n_point + q, u);
  load_v<T, VEC>(static_cast<const T*>(p.b) + bs * p.n_point + q, v);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const T uu = u[e] * u[e];
    const T vv = v[e] * v[e];
    r[e] = sqrt_rn(uu + vv);
  }
  store_v<T, VEC>(static_cast<T*>(p.out) + o * p.n_point + q, r);
}

// a = temperature (K), b = specific humidity, scalar[o] = pressure (hPa).
// T is the inputs' dtype, O the dtype of (input op pressure coordinate).
template <typename T, typename O, int VEC>
__global__ void __launch_bounds__(256)
    relative_humidity_kernel(const PointParams p) {
  const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (q >= p.n_point) return;
  const long long o = outer_index();
  if (o >= p.n_slab) return;
  const long long as = p.a_slab ? p.a_slab[o] : o;
  const long long bs = p.b_slab ? p.b_slab[o] : o;
  const O pressure = static_cast<const O*>(p.scalar)[o];
  T t[VEC], h[VEC];
  O r[VEC];
  load_v<T, VEC>(static_cast<const T*>(p.a) + as * p.n_point + q, t);
  load_v<T, VEC>(static_cast<const T*>(p.b) + bs * p.n_point + q, h);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    // Bolton (1980) saturation vapour pressure, as derived_variables.py:465-468
    const T svp = T(6.112) * exp_of(T(17.67) * (t[e] - T(273.15)) /
                                    (t[e] - T(29.65)));
    const T mixing = h[e] / (T(1) - h[e]);
    const O saturation = (O)(T(0.622) * svp) / (pressure - (O)svp);
    r[e] = (O)mixing / saturation;
  }
  store_v<O, VEC>(static_cast<O*>(p.out) + o * p.n_point + q, r);
}

// ---------------------------------------------------------------------------
// horizontal stencil
// ---------------------------------------------------------------------------
constexpr int kStencilThreads = 64;  // one wave: 64 * VEC columns
constexpr int kStencilRows = 16;     // rows a workgroup walks down (2 halo rows)
constexpr int kStencilAhead = 4;     // rows loaded before any is combined

struct StencilParams {
  // 0: the field differentiated along longitude, 1: along latitude,
  // 2, 3: u and v read pointwise (ageostrophic modes)
  const void* in[4];
  const long long* slab[4];
  const double* row_coef;  // [4][n_row]: a, b, c, den of d/d(row)
  const double* col_coef;  // [4][n_col]
  const double* lat_cos;   // [n_lat]
  const double* lat_cor;   // [n_lat], geostrophic modes
  double* out;             // [n_slab][n_row][n_col]
  long long n_slab;
  int n_row, n_col, row_uniform, col_uniform, mode;
  double m_per_deg;
};

// grid: x = column tiles of 64 * VEC, y = row chunks of kStencilRows, z = slabs
template <typename T, int VEC, bool LAT_ROWS>
__global__ void __launch_bounds__(kStencilThreads)
    stencil_kernel(const StencilParams p) {
  const int c0 = (blockIdx.x * kStencilThreads + threadIdx.x) * VEC;
  if (c0 >= p.n_col) return;
  const int r_begin = blockIdx.y * kStencilRows;
  const int r_end = min(r_begin + kStencilRows, p.n_row);
  const int n_row = p.n_row, n_col = p.n_col;
  const long long n_point = (long long)n_row * n_col;
  // which input rolls down the rows, which one needs its column neighbours
  constexpr int kRowIn = LAT_ROWS ? 1 : 0;
  constexpr int kColIn = LAT_ROWS ? 0 : 1;
  const bool ageo = p.mode >= WB2_STENCIL_AGEO_U;
  const bool geo = p.mode >= WB2_STENCIL_GEO_U;

  // per-column tables, once per workgroup
  double ca[VEC], cb[VEC], cc[VEC], cden[VEC], col_cos[VEC], col_cor[VEC];
  bool col_diff[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int c = c0 + e;
    col_diff[e] = p.col_uniform || c == 0 || c == n_col - 1;
    ca[e] = col_diff[e] ? 0.0 : p.col_coef[c];
    cb[e] = col_diff[e] ? 0.0 : p.col_coef[n_col + c];
    cc[e] = col_diff[e] ? 0.0 : p.col_coef[2 * n_col + c];
    cden[e] = p.col_coef[3 * n_col + c];
    col_cos[e] = LAT_ROWS ? 0.0 : p.lat_cos[c];
    col_cor[e] = (!LAT_ROWS && geo) ? p.lat_cor[c] : 0.0;
  }
  const int c_left = max(c0 - 1, 0);
  const int c_right = min(c0 + VEC, n_col - 1);

  for (long long o = blockIdx.z; o < p.n_slab; o += gridDim.z) {
    const T* in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long s = p.slab[k] ? p.slab[k][o] : o;
      in[k] = p.in[k] ? static_cast<const T*>(p.in[k]) + s * n_point : nullptr;
    }
    const T* rin = in[kRowIn];
    const T* cin = in[kColIn];
    const bool same = rin == cin;
    double* out = p.out + o * n_point;

    // rows r - 1 ... r + kStencilAhead of the row-differentiated input: the
    // window rolls down the chunk, kStencilAhead rows are requested at once
    constexpr int U = kStencilAhead;
    T win[U + 2][VEC];
    load_cached<T, VEC>(rin + (long long)max(r_begin - 1, 0) * n_col + c0,
                        win[0]);
    load_cached<T, VEC>(rin + (long long)r_begin * n_col + c0, win[1]);
    for (int r0 = r_begin; r0 < r_end; r0 += U) {
      T mid[U][VEC], u[U][VEC], v[U][VEC], left[U], right[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        // (rows past the chunk's end are read from the last row and dropped)
        const long long below = (long long)min(r0 + k + 1, n_row - 1) * n_col;
        const long long row = (long long)min(r0 + k, n_row - 1) * n_col;
        load_cached<T, VEC>(rin + below + c0, win[k + 2]);
        if (!same) load_cached<T, VEC>(cin + row + c0, mid[k]);
        left[k] = cin[row + c_left];
        right[k] = cin[row + c_right];
        if (ageo) {
          load_v<T, VEC>(in[2] + row + c0, u[k]);
          load_v<T, VEC>(in[3] + row + c0, v[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = r0 + k;
        if (r >= r_end) break;
        if (same) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) mid[k][e] = win[k + 1][e];
        }
        if (!ageo) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) u[k][e] = v[k][e] = T(0);
        }
        const bool row_diff = p.row_uniform || r == 0 || r == n_row - 1;
        const double ra = row_diff ? 0.0 : p.row_coef[r];
        const double rb = row_diff ? 0.0 : p.row_coef[n_row + r];
        const double rc = row_diff ? 0.0 : p.row_coef[2 * n_row + r];
        const double rden = p.row_coef[3 * n_row + r];
        const double row_cos = LAT_ROWS ? p.lat_cos[r] : 0.0;
        const double row_cor = (LAT_ROWS && geo) ? p.lat_cor[r] : 0.0;
        double res[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const T g_row = gradient_at<T>(win[k][e], win[k + 1][e],
                                         win[k + 2][e], row_diff, ra, rb, rc,
                                         rden);
          const T lo = e == 0 ? left[k] : mid[k][e - 1];
          const T hi = e == VEC - 1 ? right[k] : mid[k][e + 1];
          const T g_col = gradient_at<T>(lo, mid[k][e], hi, col_diff[e], ca[e],
                                         cb[e], cc[e], cden[e]);
          const T g_lon = LAT_ROWS ? g_col : g_row;
          const T g_lat = LAT_ROWS ? g_row : g_col;
          const double cs = LAT_ROWS ? row_cos : col_cos[e];
          const double cor = LAT_ROWS ? row_cor : col_cor[e];
          // _d_dx: / cos(lat) / metres per degree, 0.0 at the poles (:102-117)
          const double quotient = ((double)g_lon / cs) / p.m_per_deg;
          const double dx = cs > 1e-6 ? quotient : 0.0;
          // _d_dy: the input dtype divided by a Python float stays (:120-121)
          const T dy = g_lat / (T)p.m_per_deg;
          double val;
          if (p.mode == WB2_STENCIL_DIVERGENCE) {
            val = dx + (double)dy;
          } else if (p.mode == WB2_STENCIL_VORTICITY) {
            val = dx - (double)dy;
          } else {
            // geostrophic wind: +-inf / NaN on the equator on purpose
            // (:238-240)
            const double ug = (double)(-dy) / cor;
            const double vg = dx / cor;
            const double du = ageo ? (double)u[k][e] - ug : ug;
            const double dv = ageo ? (double)v[k][e] - vg : vg;
            if (p.mode == WB2_STENCIL_GEO_U || p.mode == WB2_STENCIL_AGEO_U)
              val = du;
            else if (p.mode == WB2_STENCIL_GEO_V ||
                     p.mode == WB2_STENCIL_AGEO_V)
              val = dv;
            else
              val = sqrt_rn(du * du + dv * dv);
          }
          res[e] = val;
        }
        store_v<double, VEC>(out + (long long)r * n_col + c0, res);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        win[0][e] = win[U][e];
        win[1][e] = win[U + 1][e];
      }
    }
  }
}

}  // namespace
}  // namespace wb2

extern "C" {

int wb2_derived_pointwise(int mode, int dtype, int out_dtype, const void* a,
                          const int64_t* a_slab, const void* b,
                          const int64_t* b_slab, const void* slab_scalar,
                          int64_t n_slab, int64_t n_point, void* out,
                          void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(out_dtype == WB2_F32 || out_dtype == WB2_F64,
              "unknown dtype %d", out_dtype);
  WB2_REQUIRE(mode == WB2_POINT_WIND_SPEED || mode == WB2_POINT_RELATIVE_HUMIDITY,
              "unknown mode %d", mode);
  WB2_EMPTY_OK(n_slab);
  WB2_EMPTY_OK(n_point);
  WB2_REQUIRE(a && b && out, "null pointer argument");
  const bool rh = mode == WB2_POINT_RELATIVE_HUMIDITY;
  WB2_REQUIRE(!rh || slab_scalar, "null pointer argument");
  WB2_REQUIRE(rh ? out_dtype >= dtype : out_dtype == dtype,
              "out_dtype %d does not fit dtype %d", out_dtype, dtype);
  WB2_REQUIRE((n_point + 255) / 256 < (1ll << 31), "bad sizes");
  PointParams p{};
  p.a = a;
  p.b = b;
  p.a_slab = reinterpret_cast<const long long*>(a_slab);
  p.b_slab = reinterpret_cast<const long long*>(b_slab);
  p.scalar = slab_scalar;
  p.out = out;
  p.n_slab = n_slab;
  p.n_point = n_point;
  const int w = wide_lanes(dtype);
  const bool wide = n_point % w == 0 && all_aligned16(a, b, out);
  dim3 grid;
  WB2_REQUIRE(outer_grid(n_slab, point_tiles(n_point, wide ? w : 1, 256),
                         &grid),
              "bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p);
    };
    if (!rh)
      launch(wind_speed_kernel<T, V>);
    else if constexpr (std::is_same<T, double>::value)
      launch(relative_humidity_kernel<double, double, V>);
    else if (out_dtype == WB2_F64)
      launch(relative_humidity_kernel<float, double, V>);
    else
      launch(relative_humidity_kernel<float, float, V>);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

int wb2_derived_stencil_geometry(int dtype, int wide, int32_t* tile_cols,
                                 int32_t* chunk_rows) {
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(tile_cols && chunk_rows, "null pointer argument");
  *tile_cols = kStencilThreads * (wide ? wide_lanes(dtype) : 1);
  *chunk_rows = kStencilRows;
  return 0;
}

int wb2_derived_stencil(int mode, int dtype, int lat_rows,
                        const void* const* inputs,
                        const int64_t* const* slabs, int64_t n_slab,
                        int32_t n_row, int32_t n_col, const double* row_coef,
                        int row_uniform, const double* col_coef,
                        int col_uniform, const double* lat_cos,
                        const double* lat_coriolis, double m_per_deg,
                        double* out, void* stream) {
  WB2_TRACE();
  using namespace wb2;
  WB2_REQUIRE(dtype == WB2_F32 || dtype == WB2_F64, "unknown dtype %d", dtype);
  WB2_REQUIRE(mode >= WB2_STENCIL_DIVERGENCE && mode <= WB2_STENCIL_AGEO_SPEED,
              "unknown mode %d", mode);
  WB2_EMPTY_OK(n_slab);
  WB2_REQUIRE(inputs && inputs[0] && inputs[1] && row_coef && col_coef &&
                  lat_cos && out, "null pointer argument");
  WB2_REQUIRE(mode < WB2_STENCIL_GEO_U || lat_coriolis,
              "null pointer argument");
  WB2_REQUIRE(mode < WB2_STENCIL_AGEO_U || (inputs[2] && inputs[3]),
              "null pointer argument");
  // np.gradient needs two points along an axis
  WB2_REQUIRE(n_row >= 2 && n_col >= 2, "bad sizes: %d x %d", (int)n_row,
              (int)n_col);
  StencilParams p{};
  const int n_in = mode >= WB2_STENCIL_AGEO_U ? 4 : 2;
  const int w = wide_lanes(dtype);
  bool wide = n_col % w == 0 && aligned16(out);
  for (int k = 0; k < n_in; ++k) {
    p.in[k] = inputs[k];
    p.slab[k] = slabs ? reinterpret_cast<const long long*>(slabs[k]) : nullptr;
    wide = wide && aligned16(inputs[k]);
  }
  p.row_coef = row_coef;
  p.col_coef = col_coef;
  p.lat_cos = lat_cos;
  p.lat_cor = lat_coriolis;
  p.out = out;
  p.n_slab = n_slab;
  p.n_row = n_row;
  p.n_col = n_col;
  p.row_uniform = row_uniform;
  p.col_uniform = col_uniform;
  p.mode = mode;
  p.m_per_deg = m_per_deg;
  const int tile = kStencilThreads * (wide ? w : 1);
  const dim3 grid((unsigned)((n_col + tile - 1) / tile),
                  (unsigned)((n_row + kStencilRows - 1) / kStencilRows),
                  (unsigned)(n_slab < 65535 ? n_slab : 65535));
  WB2_REQUIRE(grid.y <= 65535, "bad sizes: %d rows", (int)n_row);
  hipStream_t s = static_cast<hipStream_t>(stream);
  for_field(dtype, wide, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int V = decltype(v)::value;
    if (lat_rows)
      hipLaunchKernelGGL((stencil_kernel<T, V, true>), grid,
                         dim3(kStencilThreads), 0, s, p);
    else
      hipLaunchKernelGGL((stencil_kernel<T, V, false>), grid,
                         dim3(kStencilThreads), 0, s, p);
  });
  WB2_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
