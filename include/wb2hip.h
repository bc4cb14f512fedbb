/*
 * wb2hip.h -- C ABI of libwb2hip.so: MI355X (gfx950) kernels for the
 * WeatherBench2 per-chunk metric-evaluation hot path.
 *
 * The reference (google-research/weatherbench2) is pure Python; it has no FFI.
 * Its boundary for this path is the duck-typed operator protocol
 *   Metric.compute_chunk(forecast, truth, region, skipna)   weatherbench2/metrics.py:88-115
 *   Region.apply(dataset, weights)                          weatherbench2/regions.py:40-54
 *   DerivedVariable.compute(dataset)                        weatherbench2/derived_variables.py:54-56
 * called from evaluation._metric_and_region_loop            weatherbench2/evaluation.py:388-438.
 * The entry points below are what a ctypes binding of that protocol calls (see
 * INTEGRATION.md); each one names the reference arithmetic it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; wb2_last_error() gives
 *    the (thread-local) message.  Nothing throws, nothing takes ownership of a
 *    caller buffer, nothing allocates device memory.
 *  - every pointer marked DEV is a device (HBM) pointer; `stream` is a
 *    hipStream_t passed as void* (NULL = the default stream).  All work is
 *    enqueued asynchronously on `stream`.
 *  - a call over zero units (n_outer, n_point, n_time ... == 0: an empty chunk)
 *    is a legal no-op and returns 0 whatever the data pointers are -- empty
 *    buffers have no address; a negative count is an error.
 *  - a "slab" is one 2-D (n_row, n_col) field, n_col contiguous.  For the
 *    (…, latitude, longitude) layout of 0.25-degree ERA5 rows are latitudes; for
 *    the (…, longitude, latitude) layout of the low-resolution/mocked datasets
 *    rows are longitudes.  `n_outer` counts the slabs = product of all
 *    non-spatial dims (time, lead, level, …).
 *  - regions are decomposed on the host into `bands` of rows and `segs` of
 *    columns with identical membership; the streaming kernel emits partial sums
 *    per (outer, row-chunk, col-tile, weight-field, seg) and the combine kernel
 *    folds them into every region at once.  See DESIGN.md.
 */
#ifndef WB2HIP_H_
#define WB2HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WB2_VERSION 1

/* element types of the data slabs */
#define WB2_F32 0
#define WB2_F64 1

/* streaming-reduction modes (which reference metrics one pass feeds) */
#define WB2_MODE_DET 0      /* forecast,truth        -> MSE/RMSE/MAE/Bias      metrics.py:236-359 */
#define WB2_MODE_DET_ACC 1  /* forecast,truth,clim   -> the above + ACC        metrics.py:377-414 */
#define WB2_MODE_WIND 2     /* fu,tu,fv,tv           -> WindVectorMSE/RMSE     metrics.py:175-233 */

#define WB2_MODE_ENS 3      /* members,truth         -> CRPS & ensemble moments  metrics.py:532-846,1161-1363
                             * (partials come from wb2_ens_partials)              */

#define WB2_MODE_GAUSS 4    /* mean,std,truth        -> GaussianCRPS, GaussianVariance  metrics.py:849-937 */
#define WB2_MODE_GAUSS_THR 5 /* mean,std,truth,thr   -> Gaussian Brier / ignorance / RPS part  metrics.py:975-1158 */
#define WB2_MODE_SEEPS 7     /* forecast,truth,wet-threshold + aux p1 field + scalar dry threshold
                             * -> SEEPS  metrics.py:417-524 (always NaN-skipping)             */
#define WB2_MODE_ENS_THR 6  /* members,truth,thr     -> ensemble Brier / debiased Brier / ignorance /
                             *                          RPS part  metrics.py:1524-1891
                             * (partials come from wb2_ens_threshold_partials)              */

/* number of metrics written by wb2_det_combine, in this order */
#define WB2_NMETRIC 5
#define WB2_METRIC_MSE 0
#define WB2_METRIC_RMSE 1
#define WB2_METRIC_MAE 2
#define WB2_METRIC_BIAS 3
#define WB2_METRIC_ACC 4
/* Modes >= WB2_MODE_GAUSS are "generic": their slots are [q_0..q_{KQ-1}] plus,
 * with skipna, the matching notnull weights [n_0..n_{KQ-1}], and
 * wb2_det_combine writes the KQ spatial means into metrics rows 0..KQ-1
 * (`metrics` must then hold KQ rows, not WB2_NMETRIC). */
#define WB2_GAUSS_CRPS 0
#define WB2_GAUSS_VARIANCE 1
#define WB2_GAUSS_THR_BRIER 0
#define WB2_GAUSS_THR_IGNORANCE 1
#define WB2_GAUSS_THR_RPS_PART 2
#define WB2_ENS_THR_BRIER 0
#define WB2_ENS_THR_DEBIASED_BRIER 1
#define WB2_ENS_THR_IGNORANCE 2
#define WB2_ENS_THR_RPS_PART 3

/* metrics written by wb2_ens_combine, in this order */
#define WB2_NMETRIC_ENS 8
#define WB2_ENS_CRPS 0          /* CRPS                                metrics.py:610-675  */
#define WB2_ENS_CRPS_SPREAD 1   /* CRPSSpread                          metrics.py:678-694  */
#define WB2_ENS_CRPS_SKILL 2    /* CRPSSkill                           metrics.py:697-715  */
#define WB2_ENS_MEAN_MSE 3      /* EnsembleMeanMSE                     metrics.py:1310-1333 */
#define WB2_ENS_MEAN_RMSE 4     /* EnsembleMeanRMSESqrtBeforeTimeAvg   metrics.py:1269-1307 */
#define WB2_ENS_VARIANCE 5      /* EnsembleVariance                    metrics.py:1213-1241 */
#define WB2_ENS_STDDEV 6        /* EnsembleStddevSqrtBeforeTimeAvg     metrics.py:1161-1210 */
#define WB2_ENS_DEBIASED_MSE 7  /* DebiasedEnsembleMeanMSE             metrics.py:1336-1363 */

int wb2_version(void);
const char* wb2_last_error(void);

/* Number of accumulated sums ("slots") per cell for a mode.
 *   DET      : S(w d) S(w|d|) S(w d^2)                                  [+ S(w notnull d)]
 *   DET_ACC  : the above + S(w fa ta) S(w fa^2) S(w ta^2)               [+ 3 more notnull sums]
 *   WIND     : S(w (du^2+dv^2))                                         [+ 1]
 *   GAUSS    : S(w crps) S(w std^2)                                     [+ 2]
 *   GAUSS_THR: S(w brier) S(w ignorance) S(w rps_part)                  [+ 3]
 *   ENS_THR  : S(w brier) S(w debiased) S(w ignorance) S(w rps_part)    [+ 4]
 *   SEEPS    : S(w seeps)                                               [+ 1]
 * The bracketed sums-of-weights exist only when skipna != 0 (xarray computes
 * them always, but without NaNs they are data independent: metrics.py:161-163). */
int wb2_num_slots(int mode, int skipna);

/* Columns one wavefront covers (64 lanes x 16-byte vectors whenever n_col holds
 * one vector: rows of any length and element-aligned base pointers take the wide
 * loads -- `aligned16` does not change the width);
 * n_ctile = ceil(n_col / wb2_tile_cols(...)). */
int wb2_tile_cols(int dtype, int n_col, int aligned16);
/* The same for a given instantiation: an instantiation may cover fewer columns
 * per wavefront than the dtype's default (the build-time knob
 * WB2_F32_VEC_HEAVY cuts WB2_MODE_DET_ACC with skipna or a 2-D weight field to
 * 8-byte vectors; the shipped value keeps 16-byte vectors for all of them).
 * wb2_tile_cols(d, n, a) == wb2_tile_cols_ex(WB2_MODE_DET,
 * d, 0, 0, n, a).  Callers of wb2_stream_partials[_ex] size n_ctile / seg_eoff
 * with THIS function. */
int wb2_tile_cols_ex(int mode, int dtype, int skipna, int has_wfield, int n_col,
                     int aligned16);

/*
 * K1: fused weighted streaming reduction.  Replaces the elementwise temporaries
 * and the two einsums of _spatial_average (metrics.py:141-163) for every metric
 * of `mode` and every region, reading each input exactly once.
 *
 *  in[i]       DEV  input i (mode order above); slab o of input i starts at
 *                   element  (slab[i] ? slab[i][o] : o) * n_row * n_col
 *  slab[i]     DEV  int64[n_outer] or NULL (identity); lets truth / climatology
 *                   be gathered by valid time without a copy (metrics.py:398-404,
 *                   evaluation.py:474-475)
 *  w_row       DEV  double[n_row]  > 0   (latitude weights when rows = lat, else 1)
 *  w_col       DEV  double[n_col]  > 0   (latitude weights when cols = lat) or NULL
 *                   when every column weight is 1 (rows = lat)
 *  wfield      DEV  double[n_row*n_col] or NULL: a 2-D weight factor such as the
 *                   land-sea mask (regions.py:112-138); points with wfield == 0
 *                   are excluded (metrics.py:159-160).  PRECONDITION: every
 *                   value is finite and >= 0 -- the kernel multiplies the
 *                   weight through unconditionally and only clears the DATA of
 *                   excluded points, so a NaN cell would make every sum of its
 *                   tile NaN and a negative cell would be counted.  The Python
 *                   host checks this (plan.build_plan); other callers must.
 *  chunk_row0/chunk_nrow  DEV int32[n_chunk]: row range of each chunk (a chunk
 *                   never straddles a band boundary; nrow == 0 chunks are padding)
 *  seg_col0    DEV  int32[n_seg+1]: column range of each seg
 *  seg_eoff    DEV  int32[n_seg+1]: prefix sum of the number of column tiles each
 *                   seg intersects, tiles(s) = (seg_col0[s+1]-1)/T - seg_col0[s]/T + 1
 *                   with T = wb2_tile_cols(...).  A (seg, tile) pair is one
 *                   "entry" e = seg_eoff[s] + tile - seg_col0[s]/T; n_ts =
 *                   seg_eoff[n_seg] entries exist per (outer, chunk, weight field).
 *  partials    DEV  double[n_outer][n_chunk][nwf][n_ts][K] (out),
 *                   nwf = wfield ? 2 : 1, K = wb2_num_slots(mode, skipna).
 *                   Entries of padding chunks are not written.
 *  n_ctile          must equal ceil(n_col / wb2_tile_cols_ex(mode, dtype, skipna,
 *                   wfield != NULL, n_col, a16))
 *                   with a16 = all of in[] (and wfield) are 16-byte aligned; it
 *                   is passed explicitly so that the caller's allocation of
 *                   `partials` and the launch can never disagree.
 */
int wb2_stream_partials(int mode, int dtype, int skipna,
                        const void* const* in, const int64_t* const* slab,
                        int64_t n_outer, int32_t n_row, int32_t n_col,
                        const double* w_row, const double* w_col,
                        const double* wfield,
                        const int32_t* chunk_row0, const int32_t* chunk_nrow,
                        int32_t n_chunk, int32_t n_ctile,
                        const int32_t* seg_col0, const int32_t* seg_eoff,
                        int32_t n_seg, int32_t n_ts,
                        double* partials, void* stream);

/* As wb2_stream_partials, plus the mode-specific extras:
 *  aux     DEV double[n_row*n_col] or NULL  (WB2_MODE_SEEPS: the climatological
 *          dry fraction p1, NaN where it is masked out, metrics.py:504-506)
 *  scalar  (WB2_MODE_SEEPS: the dry threshold in data units, metrics.py:449)
 *  wfield_dtype  WB2_F64, or WB2_F32: the 2-D weight field stored as float32 --
 *          for a field whose values ARE float32 numbers (an ERA5 land-sea mask,
 *          a thresholded mask): the same results bit for bit, half the field
 *          bytes per point.  float32 inputs of the modes DET / DET_ACC / WIND
 *          only; anything else with WB2_F32 is an error. */
int wb2_stream_partials_ex(int mode, int dtype, int skipna,
                           const void* const* in, const int64_t* const* slab,
                           int64_t n_outer, int32_t n_row, int32_t n_col,
                           const double* w_row, const double* w_col,
                           const void* wfield, int wfield_dtype,
                           const double* aux,
                           double scalar, const int32_t* chunk_row0,
                           const int32_t* chunk_nrow, int32_t n_chunk,
                           int32_t n_ctile, const int32_t* seg_col0,
                           const int32_t* seg_eoff, int32_t n_seg,
                           int32_t n_ts, double* partials, void* stream);

/* As wb2_stream_partials_ex for slabs that do not share an allocation: input i
 * of outer slab o is the n_row x n_col slab at BYTE ADDRESS slab_addr[i][o].
 * This is how ONE launch serves every variable of a chunk (a Dataset's
 * variables are separate arrays; the reference walks them one after the other,
 * metrics.py:264, 284, 329, 358, 405-410 under xarray's Dataset arithmetic) and
 * several consecutive chunks of the Beam pipeline
 * (evaluation.py:583-599, 693-705: `input_chunks=init_time=1,lead_time=1`,
 * `split_vars=False`).  The fold is per slab, so results are bit-identical to
 * those of separate launches with the same chunk tables.
 *
 *  slab_addr[i] DEV int64[n_outer]: addresses of device memory, each a multiple
 *                   of the element size; required for every input of `mode`
 *  aligned16        nonzero iff every address (and wfield) is 16-byte aligned:
 *                   the caller built the tables and knows; selects the same
 *                   instantiation as aligned in[] would (n_ctile as above)
 */
int wb2_stream_partials_addr(int mode, int dtype, int skipna,
                             const int64_t* const* slab_addr, int aligned16,
                             int64_t n_outer, int32_t n_row, int32_t n_col,
                             const double* w_row, const double* w_col,
                             const void* wfield, int wfield_dtype,
                             const double* aux,
                             double scalar, const int32_t* chunk_row0,
                             const int32_t* chunk_nrow, int32_t n_chunk,
                             int32_t n_ctile, const int32_t* seg_col0,
                             const int32_t* seg_eoff, int32_t n_seg,
                             int32_t n_ts, double* partials, void* stream);

/* K1 with the wind-vector pairs of the launch answered from the SAME read as
 * their per-variable metrics.  The reference forms diff = forecast - truth once
 * and MSE.compute_chunk derives both the per-variable and the wind-vector
 * numbers from it (metrics.py:283-301 calling :194-201; scripts/evaluate.py:
 * 279-311, 420-425); a separate WB2_MODE_WIND launch reads u and v again.
 *
 *  mode        WB2_MODE_DET or WB2_MODE_DET_ACC
 *  in / slab   as wb2_stream_partials_ex; in == NULL: `slab` holds byte
 *              addresses as in wb2_stream_partials_addr (`aligned16` likewise;
 *              ignored otherwise)
 *  n_pair      the LAST 2 * n_pair of the n_outer slabs are the u slabs, then
 *              the v slabs, of n_pair pairs: pair k = slabs n_outer - 2 n_pair
 *              + k and n_outer - n_pair + k
 *  partials    as wb2_stream_partials for all n_outer slabs (the slabs outside
 *              the pairs go through the per-variable kernel)
 *  wind_partials DEV double[n_pair][n_chunk][nwf][n_ts][KW], KW =
 *              wb2_num_slots(WB2_MODE_WIND, skipna): what a WB2_MODE_WIND launch
 *              over (u, truth u, v, truth v) of the pairs writes, bit for bit
 *              (fold with wb2_det_combine(WB2_MODE_WIND, ...)).
 * Every slot -- per-variable and wind -- holds the bits of the separate
 * launches: same loads, same float32 du^2 + dv^2, same order of additions.
 * wb2_pairs_supported() says whether the launch geometry has a pair kernel
 * (rows too narrow for the wide loads have none: launch WB2_MODE_WIND then). */
int wb2_pairs_supported(int mode, int dtype, int skipna, int has_wfield,
                        int n_col, int aligned16);
int wb2_stream_partials_pairs(int mode, int dtype, int skipna,
                              const void* const* in,
                              const int64_t* const* slab, int aligned16,
                              int64_t n_outer, int64_t n_pair, int32_t n_row,
                              int32_t n_col, const double* w_row,
                              const double* w_col, const void* wfield,
                              int wfield_dtype, const int32_t* chunk_row0,
                              const int32_t* chunk_nrow, int32_t n_chunk,
                              int32_t n_ctile, const int32_t* seg_col0,
                              const int32_t* seg_eoff, int32_t n_seg,
                              int32_t n_ts, double* partials,
                              double* wind_partials, void* stream);

/*
 * K2: fold the partials into per-region sums and finalise the metrics.
 * Replaces the region loop + concat of evaluation.py:416-430 and the ratio /
 * sqrt epilogues of metrics.py:172, 233, 407-414.
 *
 *  band_chunk0 DEV int32[n_band+1]: chunks of band b are
 *                  [band_chunk0[b], band_chunk0[b+1])
 *  seg_eoff    DEV int32[n_seg+1]: as above (entries of seg s are
 *                  [seg_eoff[s], seg_eoff[s+1]))
 *  coef_band   DEV double[n_region][n_band]: multiplicity of the band's rows in
 *                  the region (0 = excluded; SliceRegion lists may repeat rows)
 *  coef_seg    DEV double[n_region][n_seg]:  same for columns
 *  region_wf   DEV int32[n_region]: 0 = uniform weights, 1 = `wfield`
 *  region_wsum DEV double[n_region]: sum of the region's weights (used as the
 *                  denominator when skipna == 0)
 *  sums        DEV double[n_outer][n_region][K]           (out, may be NULL)
 *  metrics     DEV double[WB2_NMETRIC][n_region][n_outer] (out, may be NULL).
 *                  For WB2_MODE_WIND only MSE and RMSE are meaningful.
 */
int wb2_det_combine(int mode, int skipna, const double* partials,
                    int64_t n_outer, int32_t n_chunk, int32_t nwf,
                    int32_t n_seg, const int32_t* seg_eoff, int32_t n_ts,
                    const int32_t* band_chunk0, int32_t n_band,
                    const double* coef_band, const double* coef_seg,
                    const int32_t* region_wf, const double* region_wsum,
                    int32_t n_region, double* sums, double* metrics,
                    void* stream);

/*
 * K3: fused ensemble pass.  Replaces the member mean / var(ddof=1) / abs-mean
 * sweeps (metrics.py:562-565, 824), the argsort ranks (:827-846) and the
 * rank-weighted sum (:804-813) with ONE read of the members: a lane keeps the M
 * values of its grid point in registers and sorts them with a sorting network.
 *
 *  ens         DEV  member m, slab s starts at element
 *                   m * member_stride + s * n_row * n_col  (member-major, e.g.
 *                   dims (realization, ..., lat, lon) as in schema.py:113-114)
 *  ens_slab / truth_slab  DEV int64[n_outer] or NULL (identity)
 *  n_member         1 <= M <= 128 (float32) / 64 (float64).  M == 1 yields
 *                   var = NaN; callers apply the reference's M == 1 special
 *                   cases (metrics.py:1196-1204) themselves.
 *  partials    DEV  double[n_outer][n_chunk][nwf][n_ts][K], K = wb2_ens_num_slots,
 *                   with the column tile width wb2_ens_tile_cols() (= 64)
 * Everything else as for wb2_stream_partials.
 */
int wb2_ens_num_slots(int skipna);
int wb2_ens_tile_cols(int32_t n_col);
int wb2_ens_partials(int dtype, int skipna, const void* ens,
                     const int64_t* ens_slab, const void* truth,
                     const int64_t* truth_slab, int32_t n_member,
                     int64_t member_stride, int64_t n_outer, int32_t n_row,
                     int32_t n_col, const double* w_row, const double* w_col,
                     const double* wfield, const int32_t* chunk_row0,
                     const int32_t* chunk_nrow, int32_t n_chunk,
                     int32_t n_ctile, const int32_t* seg_col0,
                     const int32_t* seg_eoff, int32_t n_seg, int32_t n_ts,
                     double* partials, void* stream);

/*
 * Ensemble threshold metrics: one read of the members (+ truth + threshold)
 * gives, per grid point, the exceedance counts behind EnsembleBrierScore,
 * DebiasedEnsembleBrierScore, EnsembleIgnoranceScore and the EnsembleRPS part
 * (metrics.py:1524-1560, 1720-1738, 1791-1802); any M >= 1, no sorting.
 * Slots/partials as for WB2_MODE_ENS_THR; fold with
 * wb2_det_combine(WB2_MODE_ENS_THR, ...).  `threshold` is [n_slab][n_row][n_col]
 * in the data dtype, resolved through thr_slab like truth.
 */
int wb2_ens_threshold_partials(
    int dtype, int skipna, const void* ens, const int64_t* ens_slab,
    const void* truth, const int64_t* truth_slab, const void* threshold,
    const int64_t* thr_slab, int32_t n_member, int64_t member_stride,
    int64_t n_outer, int32_t n_row, int32_t n_col, const double* w_row,
    const double* w_col, const double* wfield, const int32_t* chunk_row0,
    const int32_t* chunk_nrow, int32_t n_chunk, int32_t n_ctile,
    const int32_t* seg_col0, const int32_t* seg_eoff, int32_t n_seg,
    int32_t n_ts, double* partials, void* stream);

/*
 * Means / raw moments along one axis of a [n_lead][n_red][n_tail] view: the
 * compute core of scripts/compute_ensemble_mean.py:111-141 (xbeam.Mean over
 * realization), scripts/compute_averages.py:125-167 (v * lat_weights, mean over
 * averaging dims) and scripts/compute_statistical_moments.py:52-80 (means of
 * notnull(x), x, x**2).  For every (lead, tail):
 *   sum   = sum_r w_red[r] * x[l][r][t]          over the valid r
 *   sumsq = sum_r w_red[r] * (x * x)             (x * x in the input dtype;
 *                                                 NULL = not wanted)
 *   count = number of valid r                    (valid: !isnan(x), or every r
 *                                                 when skipna == 0)
 * in fp64.  w_red == NULL means all ones; otherwise w_red holds n_red /
 * w_repeat weights, each applying to w_repeat consecutive r (w_repeat = 1440
 * for latitude weights over a merged (latitude, longitude) axis, 1 for one
 * weight per element).  Deterministic: the reduced axis is cut into n_split
 * slices (wb2_axis_moments_splits() proposes a count) whose partials are
 * combined in slice order; `workspace` holds 3 * n_split * n_lead * n_tail
 * doubles.
 */
int wb2_axis_moments_splits(int64_t n_lead, int64_t n_red, int64_t n_tail,
                            int64_t w_repeat);
int wb2_axis_moments(int dtype, const void* x, int64_t n_lead, int64_t n_red,
                     int64_t n_tail, const double* w_red, int64_t w_repeat,
                     int skipna, int n_split, double* workspace, double* sum,
                     double* sumsq, double* count, void* stream);

/*
 * Spatial* threshold metrics (SpatialEnsembleBrierScore,
 * SpatialDebiasedEnsembleBrierScore, SpatialEnsembleIgnoranceScore,
 * SpatialEnsembleRPS; metrics.py:1615-1638, 1697-1719, 1780-1802, 1870-1891):
 * the four per-point scores of wb2_ens_threshold_partials, unreduced, to
 * maps[4][n_outer][n_point] (fp64; Brier, debiased Brier, ignorance, RPS
 * part).  Slab addressing as in wb2_rank_histogram (n_point = n_row * n_col).
 */
int wb2_ens_threshold_maps(int dtype, int skipna, const void* ens,
                           const int64_t* ens_slab, const void* truth,
                           const int64_t* truth_slab, const void* threshold,
                           const int64_t* thr_slab, int32_t n_member,
                           int64_t member_stride, int64_t n_outer,
                           int64_t n_point, double* maps, void* stream);

/*
 * SpatialSEEPS (metrics.py:418-509): the per-point SEEPS score (NaN where the
 * forecast, truth or masked dry fraction is NaN) to out[n_outer][n_point]
 * (fp64).  in = {forecast, truth, wet threshold} in `dtype`, each resolved
 * through its slab table (NULL = identity); aux = p1[n_point] with NaN where
 * p1 is outside (min_p1, max_p1); scalar = dry threshold in data units.
 */
int wb2_seeps_map(int dtype, const void* const* in, const int64_t* const* slab,
                  int64_t n_outer, int64_t n_point, const double* aux,
                  double scalar, double* out, void* stream);

/* wb2_seeps_map for slabs given by ADDRESS: addr[i][o] (DEV int64[n_outer], i =
 * forecast, truth, wet threshold) is the byte address of input i's slab of
 * outer index o -- the (init_time=1, lead_time=1) chunks of a window are
 * allocations of their own; one launch scores the k chunks that carry one lead
 * label (map_suite.py) and wb2_time_accumulate_runs adds them in chunk order. */
int wb2_seeps_map_addr(int dtype, const int64_t* const* addr, int64_t n_outer,
                       int64_t n_point, const double* aux, double scalar,
                       double* out, void* stream);

/*
 * RankHistogram (metrics.py:1894-2042): truth's rank among the n_member
 * members of each sample, binned by (n_member + 1) / n_bins, as float64.
 * Sample (o, pt): members at ens[(m * member_stride) + ens_slab[o] * n_point + pt]
 * (member_stride in ELEMENTS), truth at truth[truth_slab[o] * n_point + pt];
 * NULL tables mean identity.  rank = #{x_m < t}; ties (x_m == t) are broken
 * uniformly at random from a counter-based hash of (seed, o, pt) when
 * break_ties != 0 (the reference perturbs with NumPy's RNG, :1955-1980 --
 * same distribution, different stream), else truth goes first.  NaN members
 * rank highest.
 *   acc_row == NULL: out[n_outer][n_point][n_bins] is fully written (one-hot).
 *   acc_row != NULL: out[acc_row[o]][n_point][n_bins] += 1 per sample (the
 *                    caller zero-fills `out`; the temporal mean of Metric.compute
 *                    :117-138 is then out / n_time).
 * Fails when (n_member + 1) % n_bins != 0 (:1933-1938).
 */
int wb2_rank_histogram(int dtype, const void* ens, const int64_t* ens_slab,
                       const void* truth, const int64_t* truth_slab,
                       int32_t n_member, int64_t member_stride, int64_t n_outer,
                       int64_t n_point, int32_t n_bins, int break_ties,
                       uint64_t seed, const int64_t* acc_row, double* out,
                       void* stream);

/* As wb2_ens_partials, additionally storing the six pointwise values
 * (skill, spread, (t-mean)^2, var, std^2, debiased; NaN where undefined) to
 * maps[6][n_outer][n_row*n_col] (fp64, may be NULL): the Spatial* ensemble
 * metrics, metrics.py:718-772, 1244-1266, 1366-1399. */
int wb2_ens_partials_maps(int dtype, int skipna, const void* ens,
                          const int64_t* ens_slab, const void* truth,
                          const int64_t* truth_slab, int32_t n_member,
                          int64_t member_stride, int64_t n_outer,
                          int32_t n_row, int32_t n_col, const double* w_row,
                          const double* w_col, const double* wfield,
                          const int32_t* chunk_row0, const int32_t* chunk_nrow,
                          int32_t n_chunk, int32_t n_ctile,
                          const int32_t* seg_col0, const int32_t* seg_eoff,
                          int32_t n_seg, int32_t n_ts, double* partials,
                          double* maps, void* stream);

/* As wb2_ens_partials for slabs given by ADDRESS: ens_addr[o] is the byte
 * address of member 0's slab of outer index o (member m follows at
 * m * member_stride elements), truth_addr[o] that of the truth slab (both DEV
 * int64[n_outer]).  The variables of one `init_time=1,lead_time=1` ensemble
 * chunk (docs/source/official-evaluation.md:765-860) are separate allocations:
 * one launch takes all that share a member stride.  Same kernels (and bits) as
 * wb2_ens_partials for every member count. */
int wb2_ens_partials_addr(int dtype, int skipna, const int64_t* ens_addr,
                          const int64_t* truth_addr, int32_t n_member,
                          int64_t member_stride, int64_t n_outer, int32_t n_row,
                          int32_t n_col, const double* w_row,
                          const double* w_col, const double* wfield,
                          const int32_t* chunk_row0, const int32_t* chunk_nrow,
                          int32_t n_chunk, int32_t n_ctile,
                          const int32_t* seg_col0, const int32_t* seg_eoff,
                          int32_t n_seg, int32_t n_ts, double* partials,
                          void* stream);

/* As wb2_ens_partials_maps for a GATHERED ensemble: member m of outer index o
 * is the [n_row][n_col] slab at device address member_ptr[o * n_member + m]
 * (DEV int64[n_outer][n_member]) -- no stride, no common base: the forecast of
 * a probabilistic-climatology baseline (evaluation.py:458-470, 714-726: one
 * member per climatological year, gathered by (dayofyear, hour) of the valid
 * time) is read in place from the resident observations; a hole of the gather
 * (29 February in a common year) points at a slab of NaNs.  Register-sort
 * kernels only: n_member <= 128 (float32) / 64 (float64). */
int wb2_ens_partials_gather(int dtype, int skipna, const int64_t* member_ptr,
                            const void* truth, const int64_t* truth_slab,
                            int32_t n_member, int64_t n_outer, int32_t n_row,
                            int32_t n_col, const double* w_row,
                            const double* w_col, const double* wfield,
                            const int32_t* chunk_row0,
                            const int32_t* chunk_nrow, int32_t n_chunk,
                            int32_t n_ctile, const int32_t* seg_col0,
                            const int32_t* seg_eoff, int32_t n_seg,
                            int32_t n_ts, double* partials, double* maps,
                            void* stream);

/* Region fold + finalisation for the ensemble pass (same tables as
 * wb2_det_combine); metrics is double[WB2_NMETRIC_ENS][n_region][n_outer]. */
int wb2_ens_combine(int skipna, const double* partials, int64_t n_outer,
                    int32_t n_chunk, int32_t nwf, int32_t n_seg,
                    const int32_t* seg_eoff, int32_t n_ts,
                    const int32_t* band_chunk0, int32_t n_band,
                    const double* coef_band, const double* coef_seg,
                    const int32_t* region_wf, const double* region_wsum,
                    int32_t n_region, double* sums, double* metrics,
                    void* stream);

/*
 * Running temporal mean (Metric.compute's .mean(init_time) metrics.py:125-138
 * and the (sum, count) combiner of xbeam.Mean, evaluation.py:740-744).
 *   values DEV double[n_lead][n_time][n_tail] viewed as (lead.., time, tail..)
 *   sum, count DEV double[n_lead][n_tail]  (in/out, caller zero-initialises)
 * skipna != 0: NaN values add nothing to sum nor count.
 * The sum continues FROM the accumulator, value by value in time order
 * (sum = ((sum + v_0) + v_1) + ...): feeding the time steps one call at a time
 * or several per call gives the same bits.
 */
int wb2_time_accumulate(const double* values, int64_t n_lead, int64_t n_time,
                        int64_t n_tail, int skipna, double* sum, double* count,
                        void* stream);

/* The same for float32 or float64 values (dtype WB2_F32 / WB2_F64; float32
 * widens exactly: metric results in the reference's float32 result dtype need
 * no conversion pass) with a destination table: result element idx of
 * [n_lead][n_tail] goes to accumulator element dst[idx] (DEV
 * int64[n_lead * n_tail], entries distinct).  Chunks that split the lead dim as well
 * (`input_chunks=init_time=1,lead_time=1`, docs/source/official-evaluation.md:
 * 537-549) accumulate into the rows of their lead labels: xbeam.Mean combines
 * per chunk key (evaluation.py:740-744).  dst == NULL: identity. */
int wb2_time_accumulate_scatter(int dtype, const void* values, int64_t n_lead,
                                int64_t n_time, int64_t n_tail, int skipna,
                                const int64_t* dst, double* sum, double* count,
                                void* stream);
/* The same with one table entry per RUN of `run` consecutive result elements
 * that go to consecutive accumulator elements: element idx goes to
 * dst[idx / run] + idx % run (dst: DEV int64[n_lead * n_tail / run]; run must
 * divide n_lead * n_tail; the destination ranges must not overlap).  Map-valued
 * results (the Spatial* metrics, metrics.py:304-374) split by lead time need
 * one entry per slab instead of one per grid point.  count may be NULL when
 * skipna == 0 (every element gains n_time: a caller may keep that number on
 * the host). */
int wb2_time_accumulate_runs(int dtype, const void* values, int64_t n_lead,
                             int64_t n_time, int64_t n_tail, int skipna,
                             const int64_t* dst, int64_t run, double* sum,
                             double* count, void* stream);

/*
 * One chunk of the deterministic suite in ONE call: K1 (wb2_stream_partials_ex /
 * _addr) -> K2 (wb2_det_combine) -> the running temporal mean
 * (wb2_time_accumulate_scatter), enqueued back to back on `stream`.  This is
 * what evaluation._evaluate_chunk + TemporalMean do for one chunk
 * (evaluation.py:583-599, 735-744) and what a caller that evaluates many
 * chunks on one grid should call: the host work per chunk is one function call
 * (no per-kernel argument marshalling), and the kernels and their bits are
 * exactly those of the three separate entry points.
 *
 * `plan` collects the tables that do not change between chunks of one grid and
 * region set (every pointer DEV, meanings as in wb2_stream_partials_ex /
 * wb2_det_combine); the struct itself lives in HOST memory and is only read
 * during the call.
 *
 *  in / slab     as wb2_stream_partials_ex; in == NULL selects the by-address
 *                form (slab[i][o] = byte address of input i's slab o,
 *                `aligned16` as in wb2_stream_partials_addr; ignored otherwise)
 *  partials      DEV scratch, double[n_outer][n_chunk][nwf][n_ts][K]
 *  metrics       DEV double[NM][n_region][n_outer] (out; NM = WB2_NMETRIC for
 *                DET / DET_ACC / WIND, KQ for the generic modes)
 *  sum / count   DEV accumulators or NULL (no temporal accumulation).  `metrics`
 *                is then read as [acc_lead][acc_time][acc_tail] (their product
 *                must be NM * n_region * n_outer) and summed over acc_time into
 *                sum / count [acc_lead][acc_tail], through `dst` if not NULL,
 *                NaNs skipped when acc_skipna != 0 -- wb2_time_accumulate_scatter.
 */
typedef struct wb2_plan_tables {
  int32_t n_row, n_col;
  int32_t n_chunk, n_ctile;
  int32_t n_seg, n_ts;
  int32_t n_band, n_region;
  const double* w_row;
  const double* w_col;
  const void* wfield;          /* NULL: no 2-D weight field (nwf = 1) */
  int32_t wfield_dtype;        /* WB2_F64 / WB2_F32 */
  int32_t reserved;            /* 0 */
  const double* aux;           /* WB2_MODE_SEEPS: p1; else NULL */
  double scalar;               /* WB2_MODE_SEEPS: dry threshold */
  const int32_t* chunk_row0;
  const int32_t* chunk_nrow;
  const int32_t* seg_col0;
  const int32_t* seg_eoff;
  const int32_t* band_chunk0;
  const double* coef_band;
  const double* coef_seg;
  const int32_t* region_wf;
  const double* region_wsum;
} wb2_plan_tables;

int wb2_det_suite_step(const wb2_plan_tables* plan, int mode, int dtype,
                       int skipna, const void* const* in,
                       const int64_t* const* slab, int aligned16,
                       int64_t n_outer, double* partials, double* metrics,
                       int64_t acc_lead, int64_t acc_time, int64_t acc_tail,
                       int acc_skipna, const int64_t* dst, double* sum,
                       double* count, void* stream);

/* wb2_det_suite_step for a launch with wind-vector pairs
 * (wb2_stream_partials_pairs): K1 over the slabs outside the pairs, the pair
 * kernel, K2 over all n_outer slabs -> metrics[WB2_NMETRIC][n_region][n_outer],
 * K2 in mode WIND over the pairs -> wind_metrics[WB2_NMETRIC][n_region][n_pair]
 * (MSE and RMSE rows meaningful).  No accumulation step: the caller adds the
 * chunk's values where it wants them (wb2_gather_accumulate). */
int wb2_det_wind_suite_step(const wb2_plan_tables* plan, int mode, int dtype,
                            int skipna, const void* const* in,
                            const int64_t* const* slab, int aligned16,
                            int64_t n_outer, int64_t n_pair, double* partials,
                            double* wind_partials, double* metrics,
                            double* wind_metrics, void* stream);

/* The running temporal mean of a whole chunk result in ONE launch (what
 * TemporalMean / xbeam.Mean does with the Dataset _evaluate_chunk returns,
 * evaluation.py:583-599, 735-744, for every variable of it at once): output
 * element e sums, over the chunk's n_time time steps in order,
 *   v = src[e * n_time + t] < 0 ? NaN : arena[src[e * n_time + t]]
 * (rounded to float32 first where round32[e] != 0: the reference's float32
 * result dtype) into the accumulators at the DEVICE ADDRESSES sum_addr[e] /
 * count_addr[e] (distinct per e), NaNs skipped when skipna != 0.  `arena` holds
 * the `metrics` outputs of the chunk's wb2_det_suite_step calls side by side;
 * the caller derives `src` once per chunk structure (which result element
 * reads which metrics element).  All pointers DEV. */
int wb2_gather_accumulate(const double* arena, const int32_t* src,
                          const uint8_t* round32, int64_t n_out, int64_t n_time,
                          int skipna, const int64_t* sum_addr,
                          const int64_t* count_addr, void* stream);

/* wb2_gather_accumulate for a sink that KEEPS the time steps
 * (`temporal_mean=False`, evaluation.py:735: the reference skips TemporalMean
 * and the output keeps init_time): entry e is added rows[sel[e]] * rsz8[e]
 * BYTES behind sum_addr[e] / count_addr[e].  `rows` (DEV int64) are the storage
 * rows of the chunk's (time, lead) label pairs -- all a chunk brings --, `sel`
 * (DEV int32[n_out]) which of them entry e belongs to and `rsz8` (DEV
 * int64[n_out]) the bytes of one row of e's storage: structural. */
int wb2_gather_accumulate_rows(const double* arena, const int32_t* src,
                               const uint8_t* round32, int64_t n_out,
                               int64_t n_time, int skipna,
                               const int64_t* sum_addr,
                               const int64_t* count_addr, const int64_t* rows,
                               const int32_t* sel, const int64_t* rsz8,
                               void* stream);

/*
 * Chunk programs: every launch of one chunk STRUCTURE recorded once, replayed
 * per chunk in ONE call -- what _evaluate_chunk + TemporalMean do per chunk
 * (evaluation.py:583-599, 735-744), 2 920 x 40 times in the official 0.25
 * degree run, with nothing changing between chunks but the addresses of their
 * arrays and their valid times.
 *
 *  wb2_program_add_launch   one K1 + K2 step (wb2_det_suite_step, or
 *      wb2_det_wind_suite_step when n_pair > 0) over n_outer slabs given by
 *      address: input j of slab o is read at ptrs[slot[j * n_outer + o]] +
 *      rel[j * n_outer + o] (slot / rel: HOST, copied).  `partials` (and
 *      `wind_partials`) are the launch's DEV scratch, sized as for the suite
 *      step; its metrics are written at arena + arena_offset (per-variable
 *      block, then the wind block).  side_stream != 0: the launch runs on the
 *      program's second stream beside the others (small, latency-bound
 *      passes) and is joined before the sinks.
 *  wb2_program_add_ens_launch   one ensemble pass (wb2_ens_partials_addr +
 *      wb2_ens_combine: the `probabilistic` config, scripts/evaluate.py:496-520)
 *      over n_outer slabs: slot / rel [2][n_outer] = (member 0's slab, truth
 *      slab) of every outer index; `plan` carries the ENSEMBLE tile geometry
 *      (n_ctile, seg_eoff, n_ts for wb2_ens_tile_cols(n_col); wfield float64 or
 *      NULL); `partials` sized as for wb2_ens_partials; the WB2_NMETRIC_ENS x
 *      n_region x n_outer values are written at arena + arena_offset.
 *  wb2_program_add_gather   entries [first, first + count) of input `input` of
 *      the launch added LAST are read from a resident array by valid time
 *      (climatology.sel(dayofyear, hour), metrics.py:398-404) instead:
 *      address = ptrs[source] + (values[value_offset + cell[k]] + base[k]) *
 *      step_bytes -- values = the slab number of every (time, lead) cell of
 *      the chunk (per chunk), cell / base structural (HOST, copied).
 *  wb2_program_add_sink     one wb2_gather_accumulate over the arena per eval
 *      config (src / round32: DEV, kept by the caller); sel / rsz8 != NULL:
 *      wb2_gather_accumulate_rows with at most max_rows rows per chunk.
 *  wb2_program_finalize     arena = DEV double[...], the launches' outputs side
 *      by side; n_ptrs / n_values = lengths every replay must bring.
 *  wb2_program_replay       ptrs / values: HOST.  sink_args: HOST int64[3] per
 *      sink = {sum table address, count table address (DEV int64 tables as in
 *      wb2_gather_accumulate), number of rows of this sink in `rows`}; rows:
 *      HOST int64[n_rows], the kept sinks' rows one sink after the other.
 *      Everything is enqueued on `stream` (use ONE stream per program); the
 *      host only waits when it is more than four replays ahead of the copies.
 * Results are those of the separate calls, bit for bit (same kernels, same
 * order of additions). */
int wb2_program_create(void** program);
int wb2_program_destroy(void* program);
int wb2_program_add_launch(void* program, const wb2_plan_tables* plan, int mode,
                           int dtype, int skipna, int32_t n_in, int64_t n_outer,
                           int64_t n_pair, const int32_t* slot,
                           const int64_t* rel, double* partials,
                           double* wind_partials, int64_t arena_offset,
                           int side_stream);
int wb2_program_add_ens_launch(void* program, const wb2_plan_tables* plan,
                               int dtype, int skipna, int32_t n_member,
                               int64_t member_stride, int64_t n_outer,
                               const int32_t* slot, const int64_t* rel,
                               double* partials, int64_t arena_offset);
int wb2_program_add_gather(void* program, int32_t input, int64_t first,
                           int64_t count, int32_t source, int64_t step_bytes,
                           int32_t value_offset, const int32_t* cell,
                           const int64_t* base);
int wb2_program_add_sink(void* program, const int32_t* src,
                         const uint8_t* round32, int64_t n_out, int64_t n_time,
                         int skipna, const int32_t* sel, const int64_t* rsz8,
                         int64_t max_rows);
int wb2_program_finalize(void* program, double* arena, int32_t n_ptrs,
                         int32_t n_values);
int wb2_program_replay(void* program, const int64_t* ptrs, int32_t n_ptrs,
                       const int64_t* values, int32_t n_values,
                       const int64_t* sink_args, const int64_t* rows,
                       int32_t n_rows, void* stream);
/* Host seconds the replays of `program` have spent, by phase: seconds[0]
 * waiting for a free table slot (the GPU is more than four replays behind:
 * the run is GPU-bound), [1] filling the address table, [2] its copy, [3] the
 * launches, [4] the sinks; *replays = number of calls. */
int wb2_program_stats(void* program, double* seconds, int64_t* replays);

/*
 * The energy score in ONE read of the ensemble (metrics.py:1403-1517;
 * scripts/evaluate.py:541-565 evaluates score, spread and skill per chunk):
 *   skill  = mean_m     sqrt(_spatial_average((x_m - y)^2))
 *   spread = mean_{m<M-1} sqrt(_spatial_average((x_m - x_{m+1})^2))   (0 for M = 1)
 *   score  = skill - 0.5 spread
 * for every region of `plan` at once: out[3][n_region][n_outer] = (score,
 * spread, skill), fp64.  The 2 M - 1 weighted sums per region are accumulated
 * by blocks of `block` consecutive members (one wave per block, the blocks of a
 * row chunk side by side in one workgroup: HBM traffic (M + 1) elements per
 * point), folded by the combine kernel and finished by a small third kernel.
 * skipna as in _spatial_average / .mean(ensemble_dim, skipna): NaNs drop out of
 * the spatial means and NaN members out of the member means.
 *
 *  plan      tables as for wb2_det_suite_step, with n_ctile / n_ts / seg_eoff
 *            for the ENSEMBLE tile width (wb2_ens_tile_cols), wfield float64
 *  ens, ens_slab, truth, truth_slab, n_member, member_stride: as wb2_ens_partials
 *  partials  DEV scratch double[n_outer * n_block][n_chunk][nwf][n_ts][n_slot]
 *  means     DEV scratch double[2 * block][n_region][n_outer * n_block]
 *            (block, n_block, n_slot from wb2_energy_layout)
 */
int wb2_energy_layout(int32_t n_member, int skipna, int has_wfield,
                      int32_t* block, int32_t* n_block, int32_t* n_slot);
int wb2_energy_score(int dtype, int skipna, const void* ens,
                     const int64_t* ens_slab, const void* truth,
                     const int64_t* truth_slab, int32_t n_member,
                     int64_t member_stride, int64_t n_outer,
                     const wb2_plan_tables* plan, double* partials,
                     double* means, double* out, void* stream);

/*
 * K5: the Spatial* metrics (no spatial reduction): SpatialBias / SpatialMSE /
 * SpatialMAE (weatherbench2/metrics.py:304-374).
 *
 * wb2_spatial_maps: per-time maps, written in the INPUT dtype like the
 *   reference's elementwise arrays; slab o of `forecast`/`truth` is resolved
 *   through the optional int64[n_outer] tables; any of bias/mse/mae may be NULL.
 *   Outputs are [n_outer][n_point].
 * wb2_spatial_accumulate: the temporal mean of those maps (Metric.compute
 *   :117-138; xbeam.Mean evaluation.py:740-744) without materialising them:
 *   adds, for every (rest, point), the chunk's n_time steps of d, d^2, |d|
 *   (d = forecast - truth in the input dtype) to sum[3][n_rest][n_point]
 *   (order bias, mse, mae) and, when skipna, the number of non-NaN terms to
 *   count[3][n_rest][n_point].  The sums CONTINUE from the accumulators value
 *   by value (sum = ((sum + v_0) + v_1) ...), as in
 *   wb2_spatial_accumulate_addr.  Slab of (time i, rest j) =
 *   table[i * n_rest + j] (identity when NULL).
 * wb2_spatial_accumulate_addr: the same for EVERY variable of a chunk (or of a
 *   window of chunks) in one launch, into accumulators that are separate
 *   allocations -- what `deterministic_spatial` (scripts/evaluate.py:471-478)
 *   does per `init_time=1,lead_time=1` chunk before xbeam.Mean.  Destination j
 *   (a (variable, lead, level) slab of the running mean) receives the chunk's
 *   n_time steps in order; the sums CONTINUE from the accumulators value by
 *   value (sum = ((sum + v_0) + v_1) ...: the bits do not depend on how many
 *   steps a call brings).
 *     f_addr, t_addr  DEV int64[n_time][n_dst]: byte address of the slab
 *                     (n_point elements of `dtype`) of step i for destination j
 *     sum_addr        DEV int64[3][n_dst]: byte address of double[n_point] for
 *                     bias / mse / mae of destination j; 0 = not wanted
 *     count_addr      the same for the counts of non-NaN terms (skipna != 0
 *                     only; NULL otherwise: the caller adds n_time itself)
 *     aligned16       != 0: every slab address is 16-byte aligned and n_point
 *                     is a multiple of 16 / sizeof(dtype)
 */
int wb2_spatial_accumulate_addr(int dtype, int skipna, int aligned16,
                                const int64_t* f_addr, const int64_t* t_addr,
                                int64_t n_time, int64_t n_dst, int64_t n_point,
                                const int64_t* sum_addr,
                                const int64_t* count_addr, void* stream);
int wb2_spatial_maps(int dtype, const void* forecast, const int64_t* f_slab,
                     const void* truth, const int64_t* t_slab, int64_t n_outer,
                     int64_t n_point, void* bias, void* mse, void* mae,
                     void* stream);
int wb2_spatial_accumulate(int dtype, int skipna, const void* forecast,
                           const int64_t* f_slab, const void* truth,
                           const int64_t* t_slab, int64_t n_time,
                           int64_t n_rest, int64_t n_point, double* sum,
                           double* count, void* stream);

/*
 * K4: zonal energy spectrum, ZonalEnergySpectrum.compute
 * (weatherbench2/derived_variables.py:592-626): batched real-to-complex FFT
 * along longitude (rocFFT through hipFFT), then
 *   S[row, k] = |F[k] / n_lon|^2 * (k == 0 ? 1 : 2) * circumference[row % n_lat]
 * in fp64 (numpy widens float32 power * int64 to float64 at the same point).
 *
 *  plan        host handle for (dtype, n_lon, n_rows) -- create once, reuse.
 *              For the 22 row lengths with a one-kernel LDS transform
 *              (spectrum_fused.hip) creation makes twiddle tables only; the
 *              hipFFT plan behind the other lengths takes seconds (rocFFT
 *              compiles its kernels at run time) and is made at creation --
 *              or, for a one-kernel length, by the first call that cannot take
 *              that kernel (x not 16-byte aligned, n_time >= 65536).
 *  x           DEV [n_rows][n_lon], longitude contiguous; rows ordered
 *              (time, ..., latitude) with latitude the fastest row index
 *  circumference DEV double[n_lat] = cos(lat * pi / 180) * 2 pi R   (:578-581)
 *  n_time      0: out is double[n_rows][n_lon/2+1] (what compute() returns);
 *              > 0: rows are [n_time][n_rows / n_time] and out is the mean over
 *              time, double[n_rows / n_time][n_lon/2+1]
 *              (scripts/compute_zonal_energy_spectrum.py:234); skipna as in
 *              xbeam.Mean.
 *  workspace   DEV, wb2_spectrum_plan_workspace(plan) bytes, 256-byte aligned
 */
int wb2_spectrum_plan_create(int dtype, int32_t n_lon, int64_t n_rows,
                             void** plan);
int wb2_spectrum_plan_destroy(void* plan);
int64_t wb2_spectrum_plan_workspace(void* plan);
int wb2_zonal_spectrum(void* plan, const void* x, const double* circumference,
                       int32_t n_lat, int64_t n_time, int skipna, double* out,
                       void* workspace, void* stream);

/* wb2_rank_histogram with the reference's SEEDED tie breaking reproduced
 * (metrics.py:1955-1980: np.random.default_rng(seed).uniform over the
 * concatenated [truth, members] array): pcg_state_inc[4] (HOST) = the 128-bit
 * state and increment of np.random.PCG64(seed) as (state hi, state lo, inc hi,
 * inc lo); element (outer o, row r, col c, j) of the reference's concatenated
 * array (j = 0 truth, j >= 1 member j - 1; n_point = n_row * n_col points per
 * slab) has the C-order index
 *   ref_outer_off[o] (DEV int64[n_outer]) + r ref_strides[0] + c ref_strides[1]
 *   + j ref_strides[2]      (ref_strides: HOST int64[3]),
 * which is where in NumPy's stream its perturbation comes from.  Everything else
 * as wb2_rank_histogram with break_ties = 1. */
int wb2_rank_histogram_seeded(
    int dtype, const void* ens, const int64_t* ens_slab, const void* truth,
    const int64_t* truth_slab, int32_t n_member, int64_t member_stride,
    int64_t n_outer, int64_t n_point, int32_t n_col, int32_t n_bins,
    const uint64_t* pcg_state_inc, const int64_t* ref_outer_off,
    const int64_t* ref_strides, const int64_t* acc_row, double* out,
    void* stream);

/* The histogram summed (mean == 0) or averaged (mean != 0: counts / n_time,
 * the temporal mean of the one-hots, Metric.compute metrics.py:117-138) over
 * the MIDDLE axis of the outer index o = (l * n_time + t) * n_tail + j, without
 * the per-sample one-hots and without atomics (a wave owns 64 points of a
 * result row, counts in LDS): out[n_lead * n_tail][n_point][n_bins] is WRITTEN,
 * every element once.  Samples, slab tables, ranks, ties as above;
 * pcg_state_inc != NULL selects the seeded (NumPy PCG64) ties of
 * wb2_rank_histogram_seeded and needs ref_outer_off[n_lead * n_time * n_tail],
 * ref_strides and n_col.  n_bins <= 256. */
int wb2_rank_histogram_mean(
    int dtype, const void* ens, const int64_t* ens_slab, const void* truth,
    const int64_t* truth_slab, int32_t n_member, int64_t member_stride,
    int64_t n_lead, int64_t n_time, int64_t n_tail, int64_t n_point,
    int32_t n_col, int32_t n_bins, int break_ties, uint64_t seed,
    const uint64_t* pcg_state_inc, const int64_t* ref_outer_off,
    const int64_t* ref_strides, int mean, double* out, void* stream);

/* BASELINE configs[3] in one pass: the latitude-weighted mean of the zonal energy
 * spectrum WITHOUT materialising the per-latitude spectra,
 *   out[field][k] = scale * sum_lat row_weight[lat] * S[field][lat][k],
 * S = ZonalEnergySpectrum.compute (derived_variables.py:592-626) of the plan's
 * rows viewed as [field][n_lat]; row_weight[n_lat] (DEV, float64) = latitude
 * weight x circumference (the x circumference of :626 folded in), scale =
 * 1 / sum(latitude weights) for the area-weighted mean.  Every (field, latitude
 * segment) is reduced by one wave in registers into partial[field][n_seg][bins]
 * (DEV scratch, float64), the segments are then added in order (deterministic).
 * n_seg from wb2_zonal_spectrum_latmean_segments (0 = this plan has no fused
 * path: use wb2_zonal_spectrum + wb2_axis_moments); out[field][n_lon/2+1] DEV. */
int wb2_zonal_spectrum_latmean_segments(void* plan, int32_t n_lat);
int wb2_zonal_spectrum_latmean(void* plan, const void* x,
                               const double* row_weight, int32_t n_lat,
                               int32_t n_seg, double scale, double* partial,
                               double* out, void* stream);

/* ---------------------------------------------------------------------------
 * Host-side helpers and the path's one exchange step (csrc/comm.cpp)
 * ------------------------------------------------------------------------- */

/* Latitude / area weights, normalised to mean 1: replaces get_lat_weights
 * (weatherbench2/metrics.py:35-60).  `latitude` (HOST, increasing, degrees) and
 * `out` (HOST, n values) have element type `dtype`; the arithmetic runs in that
 * type like NumPy's does (metrics.py:41, 57: the weights inherit the coordinate
 * dtype).  float64: the C library's sin -- bit-identical to NumPy where NumPy
 * calls libm, else within 1-2 ulp; float32: NumPy's SIMD sinf differs from libm's
 * in the last ulp, which the cell-area difference sin(upper) - sin(lower)
 * amplifies next to the poles (<= 5e-5 relative there).  The Python host keeps
 * using NumPy itself (plan.get_lat_weights). */
int wb2_lat_weights(int dtype, const void* latitude, int64_t n, void* out);

/* Staging of PAGEABLE host chunks: the Beam pipeline hands _evaluate_chunk
 * NumPy-backed datasets (weatherbench2/evaluation.py:583-599, 693-705), i.e.
 * malloc'ed pages a DMA engine cannot read.  An uploader owns a ring of
 * `n_slots` page-locked slots of `slot_bytes` each and a pool of `n_threads`
 * copy threads: wb2_uploader_upload cuts the source into slot-sized slices,
 * the pool copies slice k + 1 into a free slot while the DMA of slice k
 * (hipMemcpyAsync on `stream`) is in flight.  The call returns once the last
 * slice has been STAGED -- `src` may be reused or freed; `dst` (DEV) is
 * complete in `stream` order.  One uploader serves one calling thread at a
 * time.  (HOST pointers: uploader_out, src.) */
int wb2_uploader_create(int32_t n_threads, int64_t slot_bytes, int32_t n_slots,
                        void** uploader_out);
/* The pool's copy on its own: dst[0:nbytes] = src[0:nbytes] (HOST, HOST) by
 * n_threads threads over 4 KiB-aligned pieces; for callers that keep their own
 * pinned buffers (feeder.ChunkFeeder). */
int wb2_host_copy(void* dst, const void* src, int64_t nbytes,
                  int32_t n_threads);
int wb2_uploader_destroy(void* uploader);
int wb2_uploader_upload(void* uploader, void* dst, const void* src,
                        int64_t nbytes, void* stream);
/* The same for the n buffers of one chunk (its variables) in ONE call:
 * dst[i] (DEV) <- src[i] (HOST), nbytes[i] each; the arrays themselves are
 * HOST.  A Python caller holds no interpreter lock for the whole chunk. */
int wb2_uploader_upload_many(void* uploader, int32_t n, void* const* dst,
                             const void* const* src, const int64_t* nbytes,
                             void* stream);

/* The way back: results that leave for the host (the float64 time-mean maps
 * of the Spatial* metrics are gigabytes per variable; the reference writes
 * them out after xbeam.Mean, weatherbench2/evaluation.py:735-752).  dst (HOST,
 * pageable) <- src (DEV), nbytes, through the same ring: the DMAs of the next
 * n_slots - 1 slices run on `stream` (behind whatever produced src there) while
 * the pool copies the slice that has arrived out of its slot.  Returns when
 * dst is complete. */
int wb2_uploader_download(void* uploader, void* dst, const void* src,
                          int64_t nbytes, void* stream);

/* RCCL communicator for callers that do not use torch.distributed: rank 0 makes
 * a 128-byte id (wb2_comm_unique_id), distributes it by any means (file, MPI,
 * socket), every rank calls wb2_comm_init_rank with the device it computes on
 * current (hipSetDevice).  `*comm_out` is an ncclComm_t. */
int wb2_comm_unique_id(void* id128);
int wb2_comm_init_rank(const void* id128, int32_t n_ranks, int32_t rank,
                       void** comm_out);
int wb2_comm_destroy(void* comm);

/* The all-reduce of the temporal mean over init-time shards: replaces the
 * combiner of xbeam.Mean (weatherbench2/evaluation.py:735-744) across ranks.
 * sum[n], count[n] (DEV, float64, e.g. the accumulators of wb2_time_accumulate)
 * are summed IN PLACE over all ranks of `comm` (an ncclComm_t, from
 * wb2_comm_init_rank or any other RCCL initialisation) as one grouped RCCL
 * operation on `stream`; the caller then divides sum / count.  Every rank must
 * call it with the same n. */
int wb2_time_mean_allreduce(double* sum, double* count, int64_t n, void* comm,
                            void* stream);

/*
 * K8: derived variables materialised as one more field of a chunk
 * (weatherbench2/derived_variables.py).  Streaming maps; slab o of an input is
 * `base + table[o] * slab elements` (identity when the table is NULL), so that
 * strided views, gathers and the variables of a chunk are read where they lie.
 *
 * wb2_derived_pointwise
 *   WB2_POINT_WIND_SPEED         out = sqrt(a * a + b * b), three correctly
 *     rounded operations in `dtype` (WindSpeed :76-99; out_dtype == dtype):
 *     bit-identical to NumPy.
 *   WB2_POINT_RELATIVE_HUMIDITY  a = temperature (K), b = specific humidity,
 *     slab_scalar[o] (DEV, n_slab values of out_dtype) = pressure (hPa) of slab
 *     o (RelativeHumidity :433-468).  The vapour-pressure and mixing-ratio
 *     terms are evaluated in `dtype`, everything the pressure enters in
 *     out_dtype = the dtype NumPy gives (input op pressure coordinate).
 *   out is [n_slab][n_point] of out_dtype.
 */
#define WB2_POINT_WIND_SPEED 0
#define WB2_POINT_RELATIVE_HUMIDITY 1
int wb2_derived_pointwise(int mode, int dtype, int out_dtype, const void* a,
                          const int64_t* a_slab, const void* b,
                          const int64_t* b_slab, const void* slab_scalar,
                          int64_t n_slab, int64_t n_point, void* out,
                          void* stream);

/*
 * wb2_derived_stencil: the horizontal derivatives _d_dx / _d_dy (:102-121) of
 * (n_row, n_col) slabs and what the reference combines them into.
 *   inputs[0]  DEV the field differentiated along longitude
 *   inputs[1]  DEV the field differentiated along latitude
 *   inputs[2], inputs[3]  DEV u and v, read pointwise (WB2_STENCIL_AGEO_* only)
 *   slabs      HOST array of 4 DEV int64[n_slab] tables (or NULL / NULL entries)
 *   lat_rows   != 0: rows are latitudes (…, latitude, longitude); 0: columns are
 *   row_coef, col_coef  DEV double[4][n]: a, b, c, den of np.gradient(f, x,
 *     edge_order=1) along the axis.  Where the axis is uniform (np.diff(x)
 *     exactly constant; *_uniform != 0) and at both ends of any axis
 *       g[i] = dtype(double(f[min(i+1, n-1)] - f[max(i-1, 0)]) / den[i])
 *     (the difference formed in `dtype`), elsewhere
 *       g[i] = dtype(a[i] f[i-1] + b[i] f[i] + c[i] f[i+1])   (in double).
 *   lat_cos, lat_coriolis  DEV double[n_lat]: cos(lat) and 2 Omega sin(lat)
 *     (the latter for the geostrophic modes only).  d/dx is
 *     g_lon / cos / m_per_deg, 0.0 where cos <= 1e-6 (_zero_poles); d/dy is
 *     g_lat / m_per_deg in `dtype`.  Division by a zero Coriolis parameter is
 *     NOT hidden: the equator row is +-inf / NaN like the reference's.
 *   out  DEV double[n_slab][n_row][n_col].
 * Both axes need at least two points (np.gradient).
 * wb2_derived_stencil_geometry: columns per workgroup tile and rows per row
 * chunk of that kernel (wide != 0: 16-byte loads; rows that are a multiple of
 * 16 / sizeof(dtype) long and 16-byte aligned buffers).
 */
#define WB2_STENCIL_DIVERGENCE 0  /* d/dx in0 + d/dy in1   :124-125 */
#define WB2_STENCIL_VORTICITY 1   /* d/dx in0 - d/dy in1   :128-129 */
#define WB2_STENCIL_GEO_U 2       /* -d/dy in1 / f         :231-244 */
#define WB2_STENCIL_GEO_V 3       /* +d/dx in0 / f */
#define WB2_STENCIL_GEO_SPEED 4
#define WB2_STENCIL_AGEO_U 5      /* u - u_geo             :313-338 */
#define WB2_STENCIL_AGEO_V 6
#define WB2_STENCIL_AGEO_SPEED 7
int wb2_derived_stencil(int mode, int dtype, int lat_rows,
                        const void* const* inputs,
                        const int64_t* const* slabs, int64_t n_slab,
                        int32_t n_row, int32_t n_col, const double* row_coef,
                        int row_uniform, const double* col_coef,
                        int col_uniform, const double* lat_cos,
                        const double* lat_coriolis, double m_per_deg,
                        double* out, void* stream);
int wb2_derived_stencil_geometry(int dtype, int wide, int32_t* tile_cols,
                                 int32_t* chunk_rows);

/*
 * K9: derived variables that walk the `level` axis of a grid column.  A column
 * slab c holds n_level blocks of n_point contiguous points; level l of column
 * slab c of input k starts `slabs[k][c * n_level + l] * n_point` elements after
 * inputs[k] (the tables are always given: a contiguous tensor, a strided view
 * of whole blocks and a gather differ in the table alone).  A thread owns
 * adjacent points (16-byte loads where n_point and the buffers allow) and
 * walks the levels.
 *
 * wb2_derived_column, with T = dtype, O = out_dtype, x = the level coordinate
 * and spacing[l] = x[l + 1] - x[l] (DEV double[n_level - 1], formed on the host
 * in the coordinate's dtype):
 *   WB2_COLUMN_INTEGRAL        out[c] = scale * trapz(in0, x)
 *     (TotalColumnWater :365-385, scale = 1 / g)
 *   WB2_COLUMN_TRANSPORT       out[c] = scale * sqrt(trapz(in0 * in1)^2 +
 *     trapz(in0 * in2)^2) (IntegratedWaterTransport :388-430; in0 = the water
 *     species, in1 = u, in2 = v, the products formed in T)
 *   WB2_COLUMN_EDDY            out[c] = scale * trapz((in0 - m0)^2 +
 *     (in1 - m1)^2) (EddyKineticEnergy :212-228, scale = 1 / 2); m0 = inputs[2]
 *     and m1 = inputs[3] are DEV T[n_column][n_level][n_mean] zonal means, the
 *     one of point i being entry (i / mean_div) % n_mean
 *     (wb2_derived_zonal_mean writes them)
 *   These three read the levels [level_begin, level_end) only, give exactly
 *   0.0 where fewer than two are selected, and write O[n_column][n_point].  As
 *   np.trapezoid does, y[l + 1] + y[l] is formed in T, multiplied by the
 *   spacing in O and halved; the sum over levels is kept in float64 and
 *   rounded to O once.  O >= T.
 *   WB2_COLUMN_GRADIENT_RATIO  out[c][l] = d(in0)/dx / (T(scale) * d(in1)/dx)
 *     (LapseRate :341-362, scale = 1 / g), T[n_column][n_level][n_point];
 *     d/dx is np.gradient(edge_order=1) from level_coef = DEV double[4][n_level]
 *     and level_uniform exactly as wb2_derived_stencil applies row_coef.
 *     O == T; at least two levels.
 *   WB2_COLUMN_CUMULATIVE      field[c][l] = sum_{k <= l} spacing[k - 1] *
 *     ((-field[c][k]) + (-field[c][k - 1])) / 2, field[c][0] = 0: scipy's
 *     cumulative_trapezoid(-field, x, initial=0), IN PLACE on out = DEV double,
 *     addressed through slabs[0] (VerticalVelocity :179-209 over the divergence
 *     of wb2_derived_stencil, spacing in Pa).  inputs is not read.
 * NaN propagates in every mode.  Unused arguments may be NULL / 0.
 * wb2_derived_column_geometry: points per workgroup tile (wide != 0: 16-byte
 * loads) and the number of levels a thread requests before it combines any.
 * wb2_derived_zonal_mean: out = DEV T[n_slab][n_lat], the mean over longitude
 * of every (n_row, n_col) slab that skips NaN (NaN where a latitude circle
 * holds no other value); slab o starts slab[o] * n_row * n_col elements after
 * `in` (identity when NULL).  lat_rows != 0: rows are latitudes.
 */
#define WB2_COLUMN_INTEGRAL 0
#define WB2_COLUMN_TRANSPORT 1
#define WB2_COLUMN_GRADIENT_RATIO 2
#define WB2_COLUMN_CUMULATIVE 3
#define WB2_COLUMN_EDDY 4
int wb2_derived_column(int mode, int dtype, int out_dtype,
                       const void* const* inputs, const int64_t* const* slabs,
                       int64_t n_column, int32_t n_level, int64_t n_point,
                       int32_t level_begin, int32_t level_end,
                       const double* spacing, const double* level_coef,
                       int level_uniform, int64_t mean_div, int32_t n_mean,
                       double scale, void* out, void* stream);
int wb2_derived_column_geometry(int dtype, int wide, int32_t* tile_points,
                                int32_t* levels_ahead);
int wb2_derived_zonal_mean(int dtype, int lat_rows, const void* in,
                           const int64_t* slab, int64_t n_slab, int32_t n_row,
                           int32_t n_col, void* out, void* stream);

/*
 * K10: derived variables that act along the lead-time axis.  The data is
 * T[n_outer][n_lead][n_point], T = dtype: n_point is the contiguous block after
 * the lead axis, n_outer everything before it.  Lead l of outer index o starts
 * `slab[o * n_lead + l] * n_point` elements after `in` (DEV int64; NULL = the
 * identity o * n_lead + l), so a contiguous tensor, a lead-sliced view and a
 * gather differ in the table alone.  out = DEV T[n_outer][n_lead][n_point],
 * contiguous; every lead is written.  A thread owns adjacent points (16-byte
 * loads where n_point and the buffers allow) and walks the leads.
 *
 * wb2_derived_lead_window, with w = window >= 1 and x the series of one point:
 *   WB2_LEAD_DIFF_SUM  d[l] = x[l] - x[l - 1] formed in T; out[l] = NaN for
 *     l < w (lead 0 included), else ((d[l-w+1] + d[l-w+2]) + ...) + d[l]; with
 *     clamp_negative != 0 a sum < 0 becomes 0.0 (NaN and -0.0 stay)
 *     (PrecipitationAccumulation :504-528)
 *   WB2_LEAD_SUM       out[l] = NaN for l < w - 1, else the same ordered sum of
 *     x[l-w+1 .. l]; clamp_negative is ignored
 *     (AggregatePrecipitationAccumulation :709-720)
 * These are xarray's rolling(dim=w).sum() with min_periods = w: every window
 * is summed afresh, oldest term first, in T, so a NaN gives NaN for exactly
 * the windows that hold it.  w >= n_lead is not an error (all NaN, but for
 * out[n_lead - 1] of WB2_LEAD_SUM at w == n_lead).  The window counts of
 * wb2_derived_lead_geometry keep their terms in registers and read every
 * element once; any other count gives the same values by reading the terms of
 * each window again.
 * wb2_derived_lead_geometry: points per workgroup tile (wide != 0: 16-byte
 * loads), the number of leads a thread requests before it combines any, and
 * the window counts with a register ring (a static table of *n_windows
 * entries).
 */
#define WB2_LEAD_DIFF_SUM 0
#define WB2_LEAD_SUM 1
int wb2_derived_lead_window(int mode, int dtype, const void* in,
                            const int64_t* slab, int64_t n_outer,
                            int32_t n_lead, int64_t n_point, int32_t window,
                            int clamp_negative, void* out, void* stream);
int wb2_derived_lead_geometry(int dtype, int wide, int32_t* tile_points,
                              int32_t* leads_ahead, const int32_t** windows,
                              int32_t* n_windows);

/*
 * K11: horizontal regridding (weatherbench2/regridding.py).  A slab is one
 * 2-D field of T = dtype: (lat, lon) with longitude contiguous when lat_rows
 * != 0 (the layout of everything else here), (lon, lat) with latitude
 * contiguous when lat_rows == 0 (the reference's regrid_array).  Slab o starts
 * `slab[o] * n_src_lat * n_src_lon` elements after `in` (DEV int64; NULL = the
 * identity), so a contiguous tensor, a strided view of whole slabs and a
 * gather differ in the table alone.  out = DEV T[n_slab][target slab],
 * contiguous, in the layout of the input.
 *
 * wb2_regrid_separable acts on each axis in turn.  Each axis has a table in
 * CSR form, built on the host from the dense (target, source) float64 weight
 * matrix of that axis: ptr = DEV int32[n_target + 1], idx = DEV int32[], w =
 * DEV double[], nan = DEV uint8[n_target].  Entries ptr[k] .. ptr[k + 1] - 1
 * belong to target index k: the entries of row k with w != 0, in ascending
 * source index; for the longitude of a periodic source a band that runs over
 * the seam (its wrap-around gap is smaller than its largest inner gap) starts
 * behind that largest gap, so that it is in ascending position within the
 * band.  nan[k] != 0: row k holds a NaN (the target index is not covered by
 * the source), it has no entries and every result along it is NaN.  idx < the
 * source extent of its axis; the tables are trusted.
 * With a = target longitude, c = target latitude, b / d = source longitude /
 * latitude, f the slab, all arithmetic in float64, every multiply and every
 * add rounded on its own (no FMA contraction), sums started at 0.0 and run in
 * table order:
 *   WB2_REGRID_NANMEAN (ConservativeRegridder :505-536)
 *     inner_t[b,c] = sum_d wlat[c,d] * (isnan(f[b,d]) ? 0.0 : f[b,d])
 *     inner_n[b,c] = sum_d wlat[c,d] * (isnan(f[b,d]) ? 0.0 : 1.0)
 *     total[a,c] = sum_b wlon[a,b] * inner_t[b,c], count[a,c] likewise over
 *     inner_n; out[a,c] = T(total / count): 0 / 0 -> NaN.  An infinity reaches
 *     the cells whose bands hold it and no other.
 *   WB2_REGRID_LINEAR (BilinearRegridder :256-294)
 *     every target index has exactly two entries: idx = (i0, i1), w = (t, *);
 *     lerp(f0, f1, t) = t == 0 ? f0 : f0 + t * (f1 - f0) (a target node on a
 *     source node takes that node's value whatever its neighbour holds;
 *     otherwise NaN propagates).  g[b,c] = lerp(f[b,i0], f[b,i1], t) along
 *     latitude, out[a,c] = T(lerp(g[j0,c], g[j1,c], u)) along longitude.
 *     Clamping at the poles, NaN outside the source and the wrap of a periodic
 *     source are in the table (t = 0 with i1 = i0; nan).
 * Workgroups of the (lat, lon) layout own one target latitude: a thread walks
 * the latitude band of its source longitudes (16-byte loads where wide: the
 * row length a multiple of the vector and `in` aligned), the longitude sums
 * run over the row of partial results in LDS.  Workgroups of the (lon, lat)
 * layout own one target longitude and stage the meridians of its band in LDS.
 * A thread requests `band` entries before it combines any; longer bands are
 * walked in pieces of that length and give the same values.  A contiguous
 * axis longer than `max_contig` takes a kernel of one thread per target cell.
 *
 * wb2_regrid_gather (NearestRegridder :230-248): out[o][j] = in_slab_o[
 * index[j]], index = DEV int32[n_tgt] into a slab of n_src elements of
 * elem_size = 1, 2, 4 or 8 bytes.  The host permutes the index table for the
 * layout: the kernel knows none.
 *
 * wb2_regrid_geometry, for wb2_regrid_separable: contiguous-axis elements per
 * workgroup pass (wide != 0: 16-byte loads), target rows (columns) per
 * workgroup, band entries in flight per thread, the longest contiguous axis of
 * the workgroup kernels, and the slabs per grid row (more are folded into the
 * grid's third dimension).
 */
#define WB2_REGRID_NANMEAN 0
#define WB2_REGRID_LINEAR 1
int wb2_regrid_separable(int mode, int dtype, int lat_rows, const void* in,
                         const int64_t* slab, int64_t n_slab,
                         int32_t n_src_lon, int32_t n_src_lat,
                         int32_t n_tgt_lon, int32_t n_tgt_lat,
                         const int32_t* lon_ptr, const int32_t* lon_idx,
                         const double* lon_w, const uint8_t* lon_nan,
                         const int32_t* lat_ptr, const int32_t* lat_idx,
                         const double* lat_w, const uint8_t* lat_nan,
                         void* out, void* stream);
int wb2_regrid_gather(int elem_size, const void* in, const int64_t* slab,
                      int64_t n_slab, int64_t n_src, const int32_t* index,
                      int64_t n_tgt, void* out, void* stream);
int wb2_regrid_geometry(int dtype, int lat_rows, int wide, int32_t* tile_elems,
                        int32_t* run_targets, int32_t* band_ahead,
                        int32_t* max_contig, int32_t* grid_slabs);

/*
 * K12: exact quantiles along one axis (scripts/compute_quantiles.py, whose
 * numerical content is xarray's quantile: NumPy's quantile / nanquantile with
 * method='linear').  The data is T[n_outer][n_red][n_inner], T = dtype:
 * n_inner is the contiguous block after the reduced axis, n_outer everything
 * before it.  Sample r of outer index o starts `slab[o * n_red + r] * n_inner`
 * elements after `in` (DEV int64; NULL = the identity o * n_red + r), so a
 * contiguous tensor, a sliced view, a gather and a permuted sample order
 * differ in the table alone.  q = HOST double[n_q], each in [0, 1], taken as
 * given (unsorted, duplicates, 0 and 1); out = DEV double[n_q][n_outer][
 * n_inner], row i belonging to q[i].  Every count is at least 1.
 *
 * wb2_quantile_select, for the series x of one point:
 *   skipna == 0: a NaN in x makes every quantile of that point (and of no
 *     other) NaN; otherwise m = n_red.  skipna != 0: NaNs are dropped and m is
 *     the number of values left; m == 0 gives NaN.
 *   With s the m values in ascending order (+-inf are ordinary values):
 *     v = q * (m - 1) in float64, lo = floor(v), hi = min(lo + 1, m - 1),
 *     t = v - lo, a = s[lo], b = s[hi], d = b - a formed in T;
 *     out = double(a) + double(d) * t where t < 0.5,
 *           double(b) - double(d) * (1 - t) where t >= 0.5
 *   (no FMA contraction).  This is NumPy's result bit for bit, its NaNs from
 *   infinities included (inf - inf); where +0.0 and -0.0 both occur the sign
 *   of a zero result is not pinned (NumPy's is not either).
 * Selection is exact and sorts nothing: values become order-preserving
 * unsigned keys of their own width (NaN above +inf, counted in the first
 * pass); the key of rank lo is found from the most significant bit down,
 * key_bits_per_pass bits per counting pass, after the leading bits that the
 * smallest and the largest key of the series share; one more pass counts the
 * keys <= it and takes the smallest key above it, which is s[hi] unless the
 * found key repeats past lo.
 *   n_red <= max_resident: a workgroup stages its tile of tile_points adjacent
 *     points (64 bytes per sample row; 16-byte loads where n_inner is a
 *     multiple of the vector and `in` is 16-byte aligned) into LDS once, as
 *     keys; a wave then serves one quantile of the tile at a time, its lanes
 *     being (slice of the samples, point) pairs that add their counters up by
 *     lane exchange: the input is read from memory once, whatever n_q is (up
 *     to 64 per launch; more are served in groups of 64).
 *   longer series: lanes are spread over (point, slice of the samples) and
 *     walk the samples through the table once per pass, targets_per_pass
 *     quantiles at a time, the groups looped over inside the call.  The input
 *     is read 1 + ceil(n_q / targets_per_pass) * (passes + 1) times: from L2 or
 *     the Infinity Cache where the problem fits there.  This is the correct
 *     and simple fallback, not a tuned path.
 * wb2_quantile_geometry: points per workgroup tile (the same with wide != 0:
 * wide loads change how a tile is staged, not its extent), the longest series
 * of the resident regime, the quantiles that share a streaming pass and the
 * key bits settled per counting pass.
 */
int wb2_quantile_select(int dtype, int skipna, const void* in,
                        const int64_t* slab, int64_t n_outer, int64_t n_red,
                        int64_t n_inner, const double* q, int32_t n_q,
                        double* out, void* stream);
int wb2_quantile_geometry(int dtype, int wide, int32_t* tile_points,
                          int64_t* max_resident, int32_t* targets_per_pass,
                          int32_t* key_bits_per_pass);

/*
 * K13: statistics over runs of a time axis (scripts/resample_in_time.py:
 * 270-309: xarray's resample(...) and rolling(...) followed by mean, min, max
 * or sum).  The data is T[n_outer][n_time][n_point], T = dtype: n_point is the
 * contiguous block after the time axis, n_outer everything before it.  Time
 * step t of outer index o starts `slab[o * n_time + t] * n_point` elements
 * after `in` (DEV int64; NULL = the identity o * n_time + t), so a contiguous
 * tensor, a time-sliced view, a gather and a permuted time order differ in the
 * table alone.
 *
 * wb2_time_bin_stats: bin b covers the time steps [bin_range[b][0],
 * bin_range[b][1]) of every series (DEV int32[n_bin][2]).  Bins may overlap
 * (rolling windows: output t has the range [t - w + 1, t + 1)) and need not be
 * ordered.  stat_mask is a sum of WB2_STAT_*; out = HOST array of the four DEV
 * outputs in the order sum, mean, min, max, each a contiguous
 * T[n_outer][n_bin][n_point], NULL where the statistic is not in the mask.
 * Every bin of every outer index is written.  A bin with begin >= end, begin <
 * 0 or end > n_time is empty or incomplete: NaN in every statistic, sum
 * included, and nothing is read for it.  Otherwise, with x0 .. x(n-1) its
 * samples in time order, m of them not NaN, all arithmetic in T without FMA
 * contraction:
 *   sum   skipna == 0: ((x0 + x1) + x2) + ..., starting from x0 itself (a bin
 *         of -0.0 alone gives -0.0); skipna != 0: the same chain with +0.0 in
 *         the place of every NaN (all NaN gives +0.0)
 *   mean  skipna == 0: sum / T(n); skipna != 0: the skipna sum / T(m), NaN if
 *         m == 0
 *   min, max  skipna == 0: NaN if any sample is NaN; skipna != 0: over the
 *         samples that are not NaN, NaN if m == 0.  +-inf are ordinary values;
 *         where +0.0 and -0.0 both occur in a bin the sign of a zero result is
 *         not pinned (NumPy's is not either).
 * Each bin is computed afresh: no running update across bins, so a NaN touches
 * exactly the bins that hold it.  All statistics of the mask come from one read
 * of the input, and a statistic has the same bits whatever else is in the
 * mask.  A thread owns adjacent points (16-byte loads where n_point is a
 * multiple of the vector and `in` and the outputs are 16-byte aligned, scalar
 * loads otherwise) and requests steps_ahead time steps before it combines
 * any.  A workgroup handles one tile of points and bins_per_group >= 1
 * consecutive bins, one after another: a small count for disjoint bins
 * (parallelism over points x bins), a larger one for overlapping bins, whose
 * shared terms then come from the workgroup's own cache lines.  The value
 * changes no result.  Zero sizes are a no-op.
 * wb2_time_window_geometry: points per workgroup tile (wide != 0: 16-byte
 * loads), the number of time steps a thread requests before it combines any,
 * and the number of outer indices per grid row (more are split over a further
 * grid dimension).
 */
#define WB2_STAT_SUM 1
#define WB2_STAT_MEAN 2
#define WB2_STAT_MIN 4
#define WB2_STAT_MAX 8
#define WB2_STAT_ALL 15
int wb2_time_bin_stats(int stat_mask, int dtype, int skipna, const void* in,
                       const int64_t* slab, int64_t n_outer, int32_t n_time,
                       int64_t n_point, const int32_t* bin_range,
                       int32_t n_bin, int32_t bins_per_group,
                       void* const* out, void* stream);
int wb2_time_window_geometry(int dtype, int wide, int32_t* tile_points,
                             int32_t* steps_ahead, int32_t* max_grid_outer);

/*
 * K14: day-of-year climatology from one read (scripts/compute_climatology.py,
 * weatherbench2/utils.py:73-287).  The reference stacks the years, pads the
 * day-of-year axis cyclically, builds a W-wide window and takes a weighted mean
 * or std over (window, year).  The weights do not depend on the year and the
 * padding wraps inside each year's row, so the statistic is a cyclic weighted
 * combination of per-day-of-year moments; nothing is read W times.
 *
 * Semantics:
 *   explicit  per hour and point, A the sorted union of the days of year
 *             present (n of them; 365 must be among them), X[y, a] the sample
 *             of year y or NaN; a NaN X[y, a] is replaced by X[y, doy 365]
 *             (fillna: day 366 of a common year, gap days and data NaNs
 *             alike).  Over the entries that are not NaN, positions mod n,
 *             H = W / 2, k = -H .. H:
 *               mean[a] = S_y S_k w[k+H] X[y, a+k] / S_y S_k w[k+H]
 *               std[a]  = sqrt(S w (X - mean[a])^2 / S w)
 *             NaN where no entry is left.
 *   fast      m[a], s[a] the NaN-skipping mean and ddof=0 std of the group of
 *             day a (no fill, no year alignment); the result at a is the
 *             NaN-skipping plain mean over i = -H .. H of
 *             v[(a - i) mod n] * w[i+H].
 *   weights   create_window_weights(W): odd W, linspace up and down, divided
 *             by its mean (the caller passes them).
 *
 * The data is T[n_outer][n_time][n_point] with K13's slab table (NULL = the
 * identity), T = float32 or float64; 16-byte loads where `in`, the outputs and
 * n_point allow, scalar loads otherwise.
 *
 * wb2_group_moments: group g holds member[group_begin[g] .. group_begin[g+1])
 * (DEV int32; `group_begin_host` is the caller's HOST copy of the n_group + 1
 * offsets, on which 0 = begin[0] <= ... <= begin[n_group] = n_member is checked
 * before anything is enqueued; the kernel cuts a device list that disagrees to
 * the members and never follows it out of them).  member[j] is a time step; a
 * value outside [0, n_time) is an absent sample (NaN, nothing is read).
 * fill[j] (DEV int32, or NULL) is the time step of the substitute, outside
 * [0, n_time) for none.  pivot (DEV float64 [n_outer][n_point], or NULL = 0).
 * Per group, for each member in order: read x; if it is NaN and has a fill,
 * read the fill step instead; if it is still NaN, skip it; otherwise y =
 * double(x) - pivot, count += 1, sum += y, sumsq += y * y (float64, no FMA
 * contraction, starting from +0.0).  count, sum, sumsq: DEV float64
 * [n_outer][n_group][n_point]; an empty group gives 0, 0, 0.  A thread owns 4
 * float32 or 2 float64 adjacent points and requests members_ahead members
 * before it combines any; a workgroup handles one point tile of one group; the
 * grid is tiles x groups x outer.  No atomics, no LDS.
 * wb2_first_finite: pivot[o][i] = the first sample of the point, in member
 * order, that is neither NaN nor +-inf, 0.0 if there is none.
 * wb2_cycle_smooth: groups are g = c * n_pos + a: n_cycle independent cycles
 * of n_pos positions.  WB2_SMOOTH_EXPLICIT: W0, W1, W2 = S_k w[k+H] * (count,
 * sum, sumsq)[(a + k) mod n_pos] in the order k = -H .. H; m = W1 / W0; mean =
 * pivot + m; v = W2 / W0 - m * m; std = sqrt(v < 0 ? 0 : v) (a NaN v stays
 * NaN); W0 == 0 gives NaN.  WB2_SMOOTH_FAST: per position pivot + S / C and
 * sqrt(max-as-above(Q / C - (S / C)^2)), NaN where C == 0; then, for each of
 * the two, the sum in the order i = -H .. H of the products value[(a - i) mod
 * n_pos] * w[i+H] that are not NaN, divided by their number (NaN if none).
 * weights: DEV float64[n_w], n_w odd and positive; H >= n_pos is legal.  Either
 * of mean, std (DEV float64 [n_outer][n_cycle * n_pos][n_point]) may be NULL.
 * wb2_climatology_geometry: points per workgroup tile of wb2_group_moments
 * (wide != 0: 16-byte loads), the members requested ahead and the outer
 * indices per grid row (more are split over a further grid dimension).
 * Zero sizes of n_outer, n_point, n_group, n_cycle or n_pos are a no-op.
 */
#define WB2_SMOOTH_EXPLICIT 0
#define WB2_SMOOTH_FAST 1
int wb2_group_moments(int dtype, const void* in, const int64_t* slab,
                      int64_t n_outer, int32_t n_time, int64_t n_point,
                      const int32_t* group_begin,
                      const int32_t* group_begin_host, int32_t n_group,
                      const int32_t* member, const int32_t* fill,
                      int32_t n_member, const double* pivot, double* count,
                      double* sum, double* sumsq, void* stream);
int wb2_first_finite(int dtype, const void* in, const int64_t* slab,
                     int64_t n_outer, int32_t n_time, int64_t n_point,
                     const int32_t* member, int32_t n_member, double* pivot,
                     void* stream);
int wb2_cycle_smooth(int mode, const double* count, const double* sum,
                     const double* sumsq, const double* pivot, int64_t n_outer,
                     int32_t n_cycle, int32_t n_pos, int64_t n_point,
                     const double* weights, int32_t n_w, double* mean,
                     double* std, void* stream);
int wb2_climatology_geometry(int dtype, int wide, int32_t* tile_points,
                             int32_t* members_ahead, int32_t* max_grid_outer);

/*
 * K15: weighted quantiles and SEEPS thresholds over the rolling day-of-year
 * window (scripts/compute_climatology.py:130-216: the `quantile` and `seeps`
 * statistics, through weatherbench2/utils.py:88-124 with a callable stat_fn).
 *
 * Semantics, per (outer, cycle c, position a, point), groups g = c * n_pos + a
 * as in K14 (member, fill, absent samples and the slab table alike): the
 * samples of a are X[y, (a + k) mod n_pos], k = -H .. H, H = n_w / 2, sample
 * (k, y) with the integer weight m[k + H] (the reference's window weights are
 * proportional to H - |k|; xarray's weighted quantile normalises them, so the
 * scale is free).  H >= n_pos is legal: the window wraps, a position then
 * enters once per k.
 *   dry       with use_dry != 0, t = T(dry_threshold): a sample x < t, compared
 *             in T, is dry.  dry_fraction = (dry samples of the window, weight
 *             zero included) / denominator; a NaN sample is not dry.
 *   kept      samples that are not NaN, not dry and have m > 0.  M = S m and
 *             Q = S m^2 over them (exact integers); M == 0 gives NaN.
 *   quantile  xarray's _weighted_quantile_1d, method 'linear', skipna: with
 *             n = M M / Q, h = (n - 1) q + 1, A = (h - 1) / n M and
 *             B = h / n M, clamped to [0, M], all float64 in this order,
 *               result = n / M * S_v v |[C<(v), C<=(v)] ^ [A, B]|
 *             over the distinct kept values v, C<(v) and C<=(v) the weight
 *             below and up to v.  Evaluated as: kA the smallest v with C<=(v) >
 *             A, kB the smallest v with C<=(v) >= B, mid = S x m over the kept
 *             samples with kA < x < kB (float64, fixed order);
 *               kA == kB:  s = kA (B - A)
 *               else       s = (kA (C<=(kA) - A) + mid) + kB (B - C<(kB))
 *             result = n / M * s, no FMA contraction.  A window that holds
 *             +-inf is not pinned.
 * wb2_window_quantile: `weights` = HOST int32[n_w], n_w odd, each >= 0; q =
 * HOST double[n_q], each in [0, 1], taken as given; quantile = DEV double
 * [n_q][n_outer][n_cycle * n_pos][n_point]; dry_fraction = DEV double
 * [n_outer][n_cycle * n_pos][n_point] or NULL (it needs use_dry and
 * denominator > 0).  Checked before anything is enqueued: K14's conditions on
 * group_begin_host, the weights, and that (largest group) * S m and * S m^2
 * fit the kernel's 32-bit counters; the kernel cuts a device list that
 * disagrees to the members.  One launch per 64 quantiles.  A workgroup owns
 * (outer, cycle, tile of tile_points adjacent points, block of `positions`
 * consecutive positions): it stages the positions + n_w - 1 cyclic positions'
 * member rows into LDS once, as K12's order-preserving keys (NaN / absent and
 * dry samples as two keys above every value), so the input of a block is read
 * from memory once whatever n_q is; a wave then serves one (position,
 * quantile) at a time, its lanes being (slice of the window's samples, point)
 * pairs that add integer weight counters up by lane exchange: one pass for M,
 * Q and the dry count, counting passes of key_bits_per_pass bits for kA and
 * kB together, one pass for the sums.  No atomics; every trip count comes from
 * the arguments.  Zero sizes of n_outer, n_cycle, n_pos, n_point or n_q are a
 * no-op.
 * wb2_window_quantile_geometry: for groups of at most n_year members and n_w
 * weights, the tile is the widest of 64 bytes, 32, ... , one point whose
 * staging leaves room for 4 positions (one point: 1) in 160 KiB of LDS;
 * `positions` is what fits, at most 32 (a launch uses min(positions, n_pos));
 * lds_bytes = (positions + n_w - 1) * n_year * tile_points * sizeof(T) + 4 *
 * n_w * n_year.  Both calls fail where not even one position of one point
 * fits (n_w * n_year above about 20 000 samples for float32): there is no
 * streaming regime.
 */
int wb2_window_quantile(int dtype, const void* in, const int64_t* slab,
                        int64_t n_outer, int32_t n_time, int64_t n_point,
                        const int32_t* group_begin,
                        const int32_t* group_begin_host, int32_t n_cycle,
                        int32_t n_pos, const int32_t* member,
                        const int32_t* fill, int32_t n_member,
                        const int32_t* weights, int32_t n_w, int use_dry,
                        double dry_threshold, int32_t denominator,
                        const double* q, int32_t n_q, double* quantile,
                        double* dry_fraction, void* stream);
int wb2_window_quantile_geometry(int dtype, int64_t n_year, int32_t n_w,
                                 int32_t* tile_points, int32_t* positions,
                                 int64_t* lds_bytes,
                                 int32_t* key_bits_per_pass);

/*
 * K16: time re-indexing as a one-read slab scatter
 * (scripts/expand_climatology.py, scripts/index_on_valid_time.py,
 * scripts/compute_probabilistic_climatological_forecasts.py: datasets built by
 * re-indexing whole slabs along time, where one source slab feeds many
 * destinations).
 *
 * wb2_slab_scatter: source s is the n_point elements that start
 * `src_slab[s] * n_point` after `in` (K13's slab convention, so a contiguous
 * tensor, a time-sliced view and a gather's base differ in the table alone).
 * For every d in dst_slab[dst_begin[s] .. dst_begin[s + 1]) the slab d of
 * `out` (n_point elements of out_dtype each) becomes that source cast to
 * out_dtype.  A source of -1 is read from nowhere and stores quiet NaN; a
 * source without destinations is skipped; an entry may repeat a source.  The
 * three tables are DEV int64: src_slab[n_source], dst_begin[n_source + 1]
 * (CSR offsets, ascending from 0), dst_slab[dst_begin[n_source]].  The
 * destinations are disjoint by contract and every table value is the
 * caller's to check: the kernel cannot.  Dtype pairs: f32 -> f32, f64 -> f64
 * and f64 -> f32 (round to nearest even; beyond float32's range gives inf);
 * every other pair is refused.
 * A thread owns adjacent points: 16-byte loads and stores where n_point is a
 * multiple of the vector (4 points; 2 for f64 -> f64) and `in` and `out` are
 * 16-byte aligned, scalar ones otherwise.  It loads its points once, before
 * its first store.  A workgroup owns one tile of points of one source and
 * blocks of dests_per_group >= 1 consecutive destinations of it.  The
 * destination counts are on the device only, so the grid is (tiles x lanes) x
 * sources: lane j takes the blocks j, j + lanes, ... of its source and reads
 * nothing if it has none; one lane where sources x tiles fill the device, up
 * to 64 where they do not.  No atomics, no LDS; neither dests_per_group nor
 * the lane count changes a bit.  Checked before anything is enqueued: the
 * dtype pair, dests_per_group, negative sizes, null pointers and a grid that
 * does not fit.  Zero sizes of n_source or n_point are a no-op.
 * wb2_slab_scatter_geometry: points per workgroup tile (wide != 0: 16-byte
 * lanes) and the sources per grid row (more are split over a further grid
 * dimension).
 */
int wb2_slab_scatter(int in_dtype, int out_dtype, const void* in,
                     const int64_t* src_slab, const int64_t* dst_begin,
                     const int64_t* dst_slab, int64_t n_source, int64_t n_point,
                     int32_t dests_per_group, void* out, void* stream);
int wb2_slab_scatter_geometry(int in_dtype, int out_dtype, int wide,
                              int32_t* tile_points, int32_t* max_grid_outer);

/*
 * K17: dataset slicing as one box gather (scripts/slice_dataset.py: .isel,
 * .sel and .drop_sel on the last two dims of a variable, together with
 * whatever was selected on the dims before them).
 *
 * wb2_box_gather: the input is [n_slab][n_row_in][n_col_in] elements of
 * elem_size bytes (4 or 8), the output [n_out_slab][n_row_out][n_col_out], and
 *   out[s][i][j] = in[src_slab[s] * n_row_in * n_col_in
 *                     + row[i] * n_col_in + col(j)]
 * with col(j) = col_list[j] where col_list is given and col0 + j * col_step
 * (any non-zero step) where it is null.  src_slab is DEV int64 in K13's slab
 * convention (a contiguous tensor, a time-sliced view, a permuted order and a
 * gather's base differ in the table alone), row and col_list are DEV int32;
 * null means identity for src_slab and row.  A bit copy: no holes, no casts,
 * no atomics, no LDS; NaN payloads and -0.0 survive.  Every table value is
 * the caller's to check: the kernel cannot.
 * Column forms (wb2_box_gather_form says which one a call takes):
 *   WB2_BOX_RUN       col_step == 1; `in` and `out` 16-byte aligned, n_col_in,
 *                     n_col_out and col0 multiples of the 16-byte lane (4
 *                     elements of 4 bytes, 2 of 8): 16-byte loads and stores
 *   WB2_BOX_REVERSED  col_step == -1; aligned likewise with col0 + 1 a
 *                     multiple of the lane: a 16-byte load from the mirrored
 *                     address, reversed in registers, a 16-byte store
 *   WB2_BOX_SCALAR    every other affine run: one element per access,
 *                     coalesced where |col_step| == 1
 *   WB2_BOX_LIST      the column list: one element per access
 * A thread owns adjacent output columns (one 16-byte lane, or one element) of
 * 4 output rows of one output slab and requests all of them before it stores
 * any.  A workgroup of 256 threads owns a tile of tile_rows x tile_cols points
 * of one slab, tile_cols the least power of two of lanes that covers
 * n_col_out (256 lanes at most); slabs go along the grid, max_grid_outer per
 * grid row.  Loads and stores stream.  Checked before anything is enqueued:
 * the element size, negative sizes, a zero step, null `in` / `out`, more
 * output rows than input rows without a row table, an affine run that leaves
 * [0, n_col_in) and a grid that does not fit.  Zero sizes of n_out_slab,
 * n_row_out or n_col_out are a no-op.
 */
enum {
  WB2_BOX_RUN = 0,
  WB2_BOX_REVERSED = 1,
  WB2_BOX_SCALAR = 2,
  WB2_BOX_LIST = 3
};
int wb2_box_gather(int elem_size, const void* in, const int64_t* src_slab,
                   int64_t n_out_slab, int32_t n_row_in, int32_t n_col_in,
                   const int32_t* row, int32_t n_row_out, int32_t col0,
                   int32_t col_step, const int32_t* col_list,
                   int32_t n_col_out, void* out, void* stream);
int wb2_box_gather_form(int elem_size, const void* in, const void* out,
                        int32_t n_col_in, int32_t col0, int32_t col_step,
                        int32_t has_col_list, int32_t n_col_out);
int wb2_box_gather_geometry(int elem_size, int form, int32_t n_col_out,
                            int32_t* tile_rows, int32_t* tile_cols,
                            int32_t* max_grid_outer);

/*
 * K18: joint exceedance tables for threshold-event verification (reliability
 * diagram, ROC, Brier decomposition, contingency table).  The reference stops
 * at one score per threshold (metrics.py:1524-1891) and has no such table.
 *
 * One point under one threshold: k = the number of members with x > thr, obs
 * = truth > thr (IEEE comparisons: a NaN threshold exceeds nothing, equality
 * is not exceedance; +-inf are ordinary values); the point is invalid iff the
 * truth or any member is NaN.
 *   code = obs * (n_member + 1) + k           for a valid point,
 *   code = 2 * (n_member + 1)                 for an invalid one,
 *   n_code = 2 * (n_member + 1) + 1.
 *
 * wb2_event_counts:
 *   cnt[t][o][i][c][code] (DEV int32, every element written) = the number of
 *   columns j with col_class[j] == c in row i of outer index o whose point has
 *   `code` under threshold t.
 * Member m of outer index o is the n_row * n_col elements that start
 * (ens_slab[o] * n_row * n_col + m * member_stride) after `ens`; the truth
 * slab starts truth_slab[o] slabs after `truth`, threshold t's slab
 * thr_slab[t * n_outer + o] slabs after threshold[t] (the convention of
 * wb2_ens_threshold_partials: a contiguous tensor, a lead-sliced view, a
 * gather's base and a threshold with fewer dims differ in the tables alone).
 * The slab tables are DEV int64, null = identity; `threshold` is a HOST array
 * of n_threshold DEV pointers; col_class is DEV int32[n_col] with values in
 * [0, n_class).  Every table value is the caller's to check: the kernel
 * cannot.  Layout (lat, lon): rows are latitudes.
 * A workgroup of 256 threads owns rows_per_group adjacent rows of one outer
 * index and walks that contiguous run: 16-byte lanes where `ens`, `truth` and
 * every threshold pointer are 16-byte aligned and n_col and member_stride are
 * whole lanes (4 float32, 2 float64), one element per access otherwise.  Per
 * point it loads the truth and the thresholds of the launch, then the members
 * four at a time (requested before any is compared), and adds 1 to an LDS
 * histogram [threshold][row][class][code] with integer LDS atomics; after a
 * barrier the histogram is stored with plain stores.  Integer adds commute:
 * two runs are bit-equal.  No global atomics, no float atomics.  Up to 4
 * thresholds share ONE read of the members and the truth ((n_member + 1 + T)
 * elements per point); more thresholds, or a histogram above the budget, are
 * split into launches here.  Outer indices go along the grid, max_grid_outer
 * per grid row.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 128 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), n_threshold >= 1, the histogram of one row of one threshold
 * against the budget ("LDS budget"), a negative member_stride, negative
 * sizes, null pointers ("null pointer") and the grid.  Zero n_outer, n_row or
 * n_col is a no-op whatever the pointers are.
 *
 * wb2_event_counts_geometry: thresholds_per_launch = the most of min(
 * n_threshold, 4) for which a histogram fits 65536 bytes, rows_per_group = the
 * most of 4, 2, 1 that fits with them, and
 *   lds_bytes = thresholds_per_launch * rows_per_group * n_class * n_code * 4.
 * `wide` (16-byte lanes) changes none of them.
 *
 * wb2_event_fold: cnt is [n_cell][n_row][n_class][n_code] (n_cell = thresholds
 * x outer indices), wrow DEV float64[n_region][n_row] (latitude weight x row
 * multiplicity), mult DEV int32[n_region][n_class] (column multiplicity of a
 * class), and
 *   table[cell][r][code] = sum_i wrow[r][i] *
 *                          (double)(sum_c mult[r][c] * cnt[cell][i][c][code])
 * with the inner sum in int64 and the rows in increasing order, one plain
 * sequential float64 sum (acc = acc + wrow * s, no fused multiply-add) from
 * 0.0: a fixed order.  One thread per output element: the simple path.  Zero
 * n_cell or n_region is a no-op.
 */
int wb2_event_counts(int dtype, const void* ens, const int64_t* ens_slab,
                     const void* truth, const int64_t* truth_slab,
                     const void* const* threshold, const int64_t* thr_slab,
                     int32_t n_threshold, int32_t n_member,
                     int64_t member_stride, int64_t n_outer, int32_t n_row,
                     int32_t n_col, const int32_t* col_class, int32_t n_class,
                     int32_t* cnt, void* stream);
int wb2_event_fold(const int32_t* cnt, int64_t n_cell, int32_t n_row,
                   int32_t n_class, int32_t n_code, const double* wrow,
                   const int32_t* mult, int32_t n_region, double* table,
                   void* stream);
int wb2_event_counts_geometry(int dtype, int32_t n_member, int32_t n_class,
                              int32_t n_threshold, int wide,
                              int32_t* rows_per_group,
                              int32_t* thresholds_per_launch,
                              int64_t* lds_bytes, int32_t* max_grid_outer);

/*
 * K19: neighbourhood verification, the sufficient statistics of the fractions
 * skill score (FSS, Roberts & Lean 2008).  The reference has no counterpart.
 *
 * wb2_event_codes: K18's operands and slab-table convention (ens, ens_slab,
 * truth, truth_slab, a HOST array of n_threshold DEV threshold pointers,
 * thr_slab[t * n_outer + o], n_member, member_stride, n_outer; tables DEV
 * int64, null = identity, every value the caller's to check) and K18's
 * per-point definitions.  Instead of a histogram it writes
 *   code[t][o][i][j] (DEV uint16, every element written)
 *     = k | obs << 8 | invalid << 9,   k = obs = 0 where invalid,
 * k = the members with x > thr (0..128), obs = truth > thr, invalid iff the
 * truth or any member is NaN.  One thread per 16-byte lane of points (where
 * ens, truth, every threshold pointer and code are 16-byte aligned and n_col
 * and member_stride are whole lanes: 4 float32, 2 float64) or per point
 * otherwise; up to 4 thresholds share ONE read of the members and the truth
 * ((n_member + 1 + T) elements read and 2 T bytes written per point); the
 * members are requested four at a time before any is compared.  More
 * thresholds become further launches here.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 128 ("n_member="), n_threshold >= 1, a negative
 * member_stride, negative sizes, null pointers ("null pointer") and the grid.
 * Zero n_outer, n_row or n_col is a no-op whatever the pointers are.
 *
 * wb2_fss_sums: code is a plane [n_cell][n_row][n_col] of such codes (n_cell =
 * thresholds x outer indices), window a HOST list of n_window odd window sizes
 * n = 2 h + 1 in grid points (1 <= n <= 255, n <= n_col), col_class DEV
 * int32[n_col] with values in [0, n_class) (the caller's to check).  The
 * window of centre (i, j) is the rows max(0, i - h) .. min(n_row - 1, i + h)
 * (clipped) and the columns (j - h .. j + h) mod n_col (cyclic).  With
 *   F = the sum of k over the window,  O = n_member * the sum of obs,
 *   sums[cell][w][i][c][0..5] (DEV int64, every element written) = the sums
 *   over the valid centres j of class c in row i of
 *     (F - O)^2,  F^2,  O^2,  F,  O,  1.
 * An invalid point counts as k = obs = 0 in every window and is no centre.
 * Integer work only, no global atomics, no float: two runs are bit-equal.
 * A workgroup of 256 threads owns one cell and rows_per_group adjacent rows
 * at full row width, thread t the ceil(n_col / 256) columns from t times that
 * on.  Per window it keeps the vertical running sum of every column in LDS (k
 * and obs in the halves of one word), adds the entering and subtracts the
 * leaving row, re-read from the plane (the first row of a group sums its
 * window directly); an inclusive scan of that row in LDS makes a horizontal
 * window two reads, the cyclic wrap an index and a multiple of the row total.
 * The six sums reach the LDS sums [window][class][6] by a wave reduction where
 * the columns of a wave are one class, by 64-bit integer LDS adds otherwise,
 * and leave with plain stores.  All windows of a launch share the walk;
 * windows_per_launch = the most of min(n_window, 4) for which
 *   lds_bytes = windows * (n_class * 48 + n_col * 12) + 128
 * fits 163840 bytes; more windows become further launches here.  Cells go
 * along the grid, max_grid_outer per grid row.  No overflow: F, O < 2^24, a
 * sum is below (n_member * n^2)^2 * n_col < 2^63.
 * Checked before anything is enqueued, in this order: 1 <= n_member <= 128
 * ("n_member="), 1 <= n_class <= 64 ("n_class="), n_window >= 1, one window
 * against the budget ("LDS budget"), negative sizes, null pointers ("null
 * pointer"), every window ("window=") and the grid.  Zero n_cell, n_row or
 * n_col is a no-op whatever the pointers are.
 *
 * wb2_fss_sums_geometry: rows_per_group (32), windows_per_launch, lds_bytes
 * and max_grid_outer as above, with the same checks.
 *
 * wb2_fss_fold: sums as above, w DEV float64[n_window][3][n_region][n_row]
 * (three groups of row weights per window), mult DEV int32[n_region][n_class],
 *   table[cell][w][r][q] = sum_i w[w][g(q)][r][i] *
 *                          (double)(sum_c mult[r][c] * sums[cell][w][i][c][q])
 * with g(q) = 0 for q = 0, 1, 2, 1 for q = 3, 4 and 2 for q = 5, the inner sum
 * in int64 and the rows in increasing order, acc = acc + w * s from 0.0 with no
 * fused multiply-add: wb2_event_fold's rule with int64 inputs and a weight
 * group per q.  One wave per (cell, w, r) and all six q: lane l takes row
 * i0 + l of a block of 64 rows (its 48 contiguous bytes of every class, the
 * integer sums, the six products), then the wave adds the block's products
 * to the accumulators lane by lane, i.e. in increasing row order; the loads
 * and the integer work are spread over the lanes, the float sum is the one a
 * single thread would take.  Still a first form: untuned.  Zero n_cell,
 * n_window or n_region is a no-op.
 */
int wb2_event_codes(int dtype, const void* ens, const int64_t* ens_slab,
                    const void* truth, const int64_t* truth_slab,
                    const void* const* threshold, const int64_t* thr_slab,
                    int32_t n_threshold, int32_t n_member,
                    int64_t member_stride, int64_t n_outer, int32_t n_row,
                    int32_t n_col, uint16_t* code, void* stream);
int wb2_fss_sums(const uint16_t* code, int64_t n_cell, int32_t n_row,
                 int32_t n_col, int32_t n_member, const int32_t* window,
                 int32_t n_window, const int32_t* col_class, int32_t n_class,
                 int64_t* sums, void* stream);
int wb2_fss_sums_geometry(int32_t n_col, int32_t n_class, int32_t n_window,
                          int32_t* rows_per_group,
                          int32_t* windows_per_launch, int64_t* lds_bytes,
                          int32_t* max_grid_outer);
int wb2_fss_fold(const int64_t* sums, int64_t n_cell, int32_t n_window,
                 int32_t n_row, int32_t n_class, const double* w,
                 const int32_t* mult, int32_t n_region, double* table,
                 void* stream);

/*
 * K20: the per-rank-bin sums of Hersbach's CRPS decomposition (Wea.
 * Forecasting 2000): reliability, potential CRPS, the bin widths g_i and the
 * observed frequencies o_i are host arithmetic on them.  The reference has the
 * CRPS (metrics.py:760-830) and no counterpart of the decomposition.
 *
 * One point with truth y and the members sorted x_1 <= ... <= x_M, all
 * arithmetic in float64 after an exact widening, bins b = 0 .. M:
 *   b = 0:      alpha = 0,                    beta = max(x_1 - y, 0)
 *   b = M:      alpha = max(y - x_M, 0),      beta = 0
 *   0 < b < M:  c = min(max(y, x_b), x_{b+1}), alpha = c - x_b,
 *               beta = x_{b+1} - c
 *   below = y < x_1, above = y > x_M (strict: a tie is no outlier).
 * The point is invalid iff the truth or any member is NaN (K18's rule).
 * Points that hold +-inf are not pinned.
 *
 * wb2_crps_bin_sums: K18's operands and slab-table convention (ens, ens_slab,
 * truth, truth_slab, n_member, member_stride, n_outer; tables DEV int64, null
 * = identity; col_class DEV int32[n_col] with values in [0, n_class); every
 * table value the caller's to check).  With n_bin = n_member + 1,
 *   sums[o][i][c][0][b], sums[o][i][c][1][b] (DEV float64, every element
 *     written) = the sums of alpha_b and beta_b over the valid points of the
 *     columns j with col_class[j] == c in row i of outer index o,
 *   cnt[o][i][c][0..2] (DEV int32, every element written) = the numbers of
 *     those points with `below`, with `above`, and of all of them.  (The
 *     invalid count is the column count of the class minus cnt[..][2].)
 * THE ORDER OF THE SUM of one (o, i, c, term, b): one sequential float64
 * chain s = s + v from +0.0 over the valid points of the class in INCREASING
 * COLUMN ORDER; an invalid point adds nothing.  It does not depend on the
 * tile, on the other classes or on the launch: two runs are bit-equal, and a
 * host loop over the columns reproduces the bits.
 * One wave (a workgroup of its own: rows_per_group = 1) owns one row of one
 * outer index and walks it in tiles of tile_cols = 64 columns.  Per tile a
 * lane requests the truth and the n_member members of its point, all before
 * any is looked at -- each element is read ONCE: (n_member + 1) elements per
 * point --, sorts the members in registers (the networks of K3, +inf padding
 * to the next power of two >= 2) and stores them and the truth in a
 * wave-private LDS tile [n_bin][65].  Then lane b takes bin b (lane 0: beta_0
 * and alpha_M, whose signs are the two outlier flags) and the wave walks the
 * points of the tile in column order, eight at a time: each lane reads x_b,
 * x_{b+1} and y of the eight from the tile, forms its alphas and betas and
 * adds them to its running sums one after the other.  Where the class of the
 * column changes (wave-uniform) the lane stores its sums to `sums` and takes
 * up those of the new class -- read back from `sums` if the row met the class
 * before, +0.0 otherwise.  Plain stores; no atomics at all.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 64 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), a negative member_stride, negative sizes, null pointers
 * ("null pointer") and the grid.  Zero n_outer, n_row or n_col is a no-op
 * whatever the pointers are.
 *
 * wb2_crps_bins_geometry: min_member = 1, max_member = 64 (both dtypes),
 * tile_cols = 64, rows_per_group = 1,
 *   lds_bytes = (n_member + 1) * 65 * sizeof(element)   (at most 33800),
 * max_grid_outer outer indices per grid row.  The same checks of dtype,
 * n_member and n_class.
 *
 * wb2_crps_bin_fold: sums is [n_cell][n_row][n_class][n_slot] (n_slot =
 * 2 n_bin), wrow DEV float64[n_region][n_row], mult DEV int32[n_region][
 * n_class], and
 *   table[cell][r][s] = sum_i wrow[r][i] *
 *                       (sum_c (double)mult[r][c] * sums[cell][i][c][s])
 * with the classes and then the rows in increasing order, both plain
 * sequential float64 sums from +0.0 (t = t + m * v, acc = acc + wrow * t, no
 * fused multiply-add): a fixed order.  One thread per output element: the
 * simple path.  The counts go through wb2_event_fold (n_code = 3 or 4).  Zero
 * n_cell or n_region is a no-op.
 */
int wb2_crps_bin_sums(int dtype, const void* ens, const int64_t* ens_slab,
                      const void* truth, const int64_t* truth_slab,
                      int32_t n_member, int64_t member_stride, int64_t n_outer,
                      int32_t n_row, int32_t n_col, const int32_t* col_class,
                      int32_t n_class, double* sums, int32_t* cnt,
                      void* stream);
int wb2_crps_bin_fold(const double* sums, int64_t n_cell, int32_t n_row,
                      int32_t n_class, int32_t n_slot, const double* wrow,
                      const int32_t* mult, int32_t n_region, double* table,
                      void* stream);
int wb2_crps_bins_geometry(int dtype, int32_t n_member, int32_t n_class,
                           int32_t* min_member, int32_t* max_member,
                           int32_t* tile_cols, int32_t* rows_per_group,
                           int64_t* lds_bytes, int32_t* max_grid_outer);

/*
 * K21: the sums of the threshold-weighted CRPS (twCRPS; Gneiting & Ranjan
 * 2011, in the chaining-function form of Allen, Ginsbourger & Ziegel 2023)
 * with the tail weights 1[z >= t] (upper) and 1[z <= t] (lower).  The
 * reference has the CRPS (metrics.py:760-830) and no counterpart.
 *
 * One point with truth y, the members sorted x_1 <= ... <= x_M and the
 * threshold value t, all arithmetic in float64 after an exact widening:
 *   v(z) = z < t ? t : z   (upper, lower == 0: max(z, t))
 *   v(z) = z > t ? t : z   (lower != 0: min(z, t))
 *   A = sum_{i=1..M} |v(x_i) - v(y)|, added in sorted-member order from +0.0
 *   B = sum_{k=1..M-1} (double)(k (M - k)) * (v(x_{k+1}) - v(x_k)), added in
 *       increasing k from +0.0, each product rounded before it is added (no
 *       fused multiply-add); B = 0 for M = 1.  This is the gap form of
 *       sum_{i<j} |v(x_i) - v(x_j)|: every term is >= 0, a gap wholly beyond
 *       the threshold is exactly 0.
 * twCRPS = A / M - B / M^2; the divisions are the caller's.  v is monotone, so
 * one sort serves every threshold.  The point is invalid FOR THRESHOLD t iff
 * the truth, any member or that threshold's value at the point is NaN (K18's
 * rule, per threshold: it does not depend on how the thresholds are grouped
 * into launches).  t = -inf (upper) and t = +inf (lower) are ordinary and give
 * the plain CRPS terms; any other +-inf is not pinned.
 *
 * wb2_twcrps_sums: K18's operands and slab-table convention (ens, ens_slab,
 * truth, truth_slab, a HOST array of n_threshold DEV threshold pointers,
 * thr_slab[t * n_outer + o], n_member, member_stride, n_outer; tables DEV
 * int64, null = identity; col_class DEV int32[n_col] with values in [0,
 * n_class); every table value the caller's to check).
 *   sums[t][o][i][c][0], sums[t][o][i][c][1] (DEV float64, every element
 *     written) = the sums of A and of B over the points, valid for threshold
 *     t, of the columns j with col_class[j] == c in row i of outer index o,
 *   cnt[t][o][i][c] (DEV int32, every element written) = their number.  (The
 *     invalid count is the column count of the class minus cnt.)
 * Threshold-major: the folds below take n_cell = n_threshold * n_outer.
 * THE ORDER OF THE SUM of one (t, o, i, c, term): one sequential float64 chain
 * s = s + v from +0.0 over the points of the class in INCREASING COLUMN ORDER,
 * where a point that is invalid for t enters as +0.0.  Every summand is >=
 * +0.0, so that +0.0 changes no bit: the chain is the one over the valid
 * points.  It does not depend on the tile, on the other classes or thresholds
 * or on the launch: two runs are bit-equal, and a host loop over the columns
 * reproduces the bits.
 * One wave (a workgroup of its own: rows_per_group = 1) owns one row of one
 * outer index and walks it in tiles of tile_cols = 64 columns.  Per tile a
 * lane requests the truth, the thresholds of the launch and the n_member
 * members of its point, all before any is looked at -- each element is read
 * ONCE: (n_member + 1 + T) elements per point --, and sorts the members in
 * registers (the networks of K3, +inf padding to the next power of two >= 2).
 * Each of the up to 4 thresholds of a launch is then a pass over the sorted
 * registers that leaves the lane's A and B in a wave-private LDS tile
 * [2 T][65] of float64.  Then lane s < 2 T takes slot (threshold s / 2, term
 * s % 2) and walks the points of the tile in column order, eight LDS reads at
 * a time, adding each to its running sum.  Where the class of the column
 * changes (wave-uniform) the lane stores its sum to `sums` and takes up that
 * of the new class -- read back from `sums` if the row met the class before,
 * +0.0 otherwise.  The counts are popcounts of the validity ballots.  Plain
 * stores; no atomics at all.  More than 4 thresholds become further launches
 * here, each with its own read of the members.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 64 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), n_threshold >= 1 ("n_threshold="), a negative member_stride,
 * negative sizes, null pointers ("null pointer") and the grid.  Zero n_outer,
 * n_row or n_col is a no-op whatever the pointers are.
 *
 * wb2_twcrps_geometry: min_member = 1, max_member = 64 (both dtypes),
 * thresholds_per_launch = min(n_threshold, 4), tile_cols = 64, rows_per_group
 * = 1,
 *   lds_bytes = 2 * thresholds_per_launch * 65 * 8   (at most 4160),
 * max_grid_outer outer indices per grid row.  The same checks of dtype,
 * n_member, n_class and n_threshold.
 *
 * The fold: the sums go through wb2_crps_bin_fold (n_cell = n_threshold *
 * n_outer, n_slot = 2), the counts through wb2_event_fold (n_code = 2: valid,
 * invalid).
 */
int wb2_twcrps_sums(int dtype, const void* ens, const int64_t* ens_slab,
                    const void* truth, const int64_t* truth_slab,
                    const void* const* threshold, const int64_t* thr_slab,
                    int32_t n_threshold, int32_t n_member,
                    int64_t member_stride, int64_t n_outer, int32_t n_row,
                    int32_t n_col, const int32_t* col_class, int32_t n_class,
                    int lower, double* sums, int32_t* cnt, void* stream);
int wb2_twcrps_geometry(int dtype, int32_t n_member, int32_t n_class,
                        int32_t n_threshold, int32_t* min_member,
                        int32_t* max_member, int32_t* thresholds_per_launch,
                        int32_t* tile_cols, int32_t* rows_per_group,
                        int64_t* lds_bytes, int32_t* max_grid_outer);

/*
 * K22: box pooling of (latitude, longitude) slabs -- the mean or the maximum
 * over an odd window n = 2 h + 1 in grid points ("upscaling", Ebert 2008; the
 * average- and max-pooled scores of Price et al. 2025).  The reference has no
 * counterpart.
 *
 * The window of point (i, j) of a slab of n_row x n_col is K19's: the rows
 * r0 = max(0, i - h) .. r1 = min(n_row - 1, i + h) (clipped at the poles), the
 * columns (j - h .. j + h) mod n_col (cyclic), N_i = n * (r1 - r0 + 1) points.
 * THE TWO ORDERS:
 *   kind = WB2_POOL_MEAN: float64 after an exact widening.
 *     H[r][j] = the sequential chain s = s + x[r][(j + d) mod n_col] over the
 *       column offsets d = -h, ..., +h in that order, STARTED FROM THE FIRST
 *       TERM (not from +0.0: -0.0 survives n = 1),
 *     V[i][j] = the sequential chain of H[r][j] over r = r0 .. r1, increasing,
 *       started from H[r0][j],
 *     out = V / (double)N_i, rounded once to the input dtype (to nearest
 *       even).  No fused multiply-add.  NaN and +-inf follow IEEE in that
 *       order -- a window that holds a NaN is NaN, +inf and -inf in one window
 *       are NaN --; nothing is special-cased; the payload and the sign of a
 *       NaN are not pinned.
 *   kind = WB2_POOL_MAX: the input dtype, the same two passes with
 *     m = first; for each next v: m = (v > m || v != v) ? v : m.
 *     A NaN propagates; the sign of a zero result is that of the first zero
 *     met in that order.
 * n = 1 returns the input's values (bit-equal but for NaN payloads).  Running
 * or prefix sums round differently and are not an implementation of this.
 *
 * wb2_pool_fields: K18's operand convention.  Field (o, m), o < n_outer, m <
 * n_member, starts in_slab[o] * n_row * n_col + m * member_stride ELEMENTS
 * after `in` (in_slab DEV int64[n_outer], null = identity; every table value
 * the caller's to check); a field without members is n_member = 1.
 * `windows` is a HOST int32[n_window].  out[w][o][m][i][j] (DEV, contiguous,
 * the input dtype, every element written).
 * A workgroup of 1024 threads owns one field and a tile of tile_rows x
 * tile_cols outputs.  It stages the tile and its halo for the largest window
 * of the launch in LDS once (rows clipped, the column index wrapped), then per
 * window writes the horizontal chains of the rows that window reaches to a
 * second LDS tile (8 bytes a chain) and walks them vertically.  Consecutive
 * lanes hold consecutive columns in both passes.  Up to windows_per_launch = 4
 * windows share one staging; further windows are further launches, each staged
 * for its own largest window.  Where `in`, `out` are 16-byte aligned and n_col
 * and member_stride are multiples of 16 / sizeof(element), the tile's own
 * columns are read with 16-byte loads and the results leave in 16-byte
 * streaming stores; otherwise one element per access.  The halo is always one
 * element per access.  Both forms give the same bits.  Plain stores, no
 * atomics: two runs are bit-equal.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), kind ("kind="), 1 <= n_member <= 128 ("n_member="), n_window >= 1
 * ("n_window="), a negative member_stride, n_outer, n_row or n_col ("is
 * negative"), `windows` ("null pointer"), every window odd, 1 to 255 and at
 * most n_col ("window=") and at most max_window ("max_window"); then zero
 * n_outer, n_row or n_col is a no-op whatever `in` and `out` are; then `in`
 * and `out` ("null pointer") and the grid.
 *
 * wb2_pool_geometry: tile_cols = 64; tile_rows = the first of 32, 16, 8 whose
 * staging for the LARGEST window of the call,
 *   lds_bytes = round8((tile_rows + 2 h) * (64 + 2 h) * sizeof(element))
 *               + (tile_rows + 2 h) * 64 * 8,
 * is at most 160 KiB (every launch of the call uses that tile);
 * windows_per_launch = min(n_window, 4); max_window = the largest window whose
 * staging fits at tile_rows = 8 (123 for float32, 99 for float64);
 * max_grid_outer fields per grid row.  The same checks of dtype, n_window,
 * n_col and the windows.
 */
#define WB2_POOL_MEAN 0
#define WB2_POOL_MAX 1
int wb2_pool_fields(int dtype, const void* in, const int64_t* in_slab,
                    int32_t n_member, int64_t member_stride, int64_t n_outer,
                    int32_t n_row, int32_t n_col, const int32_t* windows,
                    int32_t n_window, int kind, void* out, void* stream);
int wb2_pool_geometry(int dtype, int32_t n_col, const int32_t* windows,
                      int32_t n_window, int32_t* windows_per_launch,
                      int32_t* tile_rows, int32_t* tile_cols,
                      int64_t* lds_bytes, int32_t* max_window,
                      int32_t* max_grid_outer);

/*
 * K23: count-weighted means of a time axis, one per bootstrap replicate (the
 * block bootstrap of per-time results, weatherbench2_amd/bootstrap.py).  The
 * reference has no counterpart.
 *
 * The data is K13's: T[n_outer][n_time][n_point], T = dtype; time step t of
 * outer index o starts `slab[o * n_time + t] * n_point` elements after `in`
 * (DEV int64; NULL = the identity o * n_time + t; every table value the
 * caller's to check).  Replicate b draws time step t counts[b][t] >= 0 times
 * (how the counts are passed: below).
 * out is a contiguous DEV double[n_rep][n_outer][n_point], every element
 * written.
 *
 * THE ORDER.  For replicate b, outer index o, point p:
 *   walk t = 0 .. n_time - 1 in increasing order, n = counts[b][t];
 *   a step with n == 0 is LEFT OUT: it is not multiplied, so a NaN or +-inf at
 *     a time the replicate did not draw cannot reach it;
 *   x = the value widened exactly to float64; with skipna != 0 a NaN x is
 *     left out;
 *   term = (double)n * x, one rounding;
 *   the first used term starts the chain, every later one is S = S + term, one
 *     rounding (started at -0.0 the chain has the same bits: (-0.0) + term is
 *     term, and that is how the kernel and the host path do it);
 *   W = the integer sum of the used n;
 *   out = S / (double)W, one rounding; with no used term 0.0 / 0.0 (NaN).
 * No fused multiply-add for float64 input.  For float32 input n * x is exact
 * in float64, so there an fma gives the same bits and is used.  NaN and +-inf
 * at a used step follow IEEE in that order; the payload and the sign of a NaN
 * are not pinned.  Plain stores, no atomics: two runs are bit-equal.
 *
 * The counts arrive widened to float64 and laid out for the kernel, with R =
 * replicates_per_group, A = steps_ahead and n_group = ceil(n_rep / R):
 *   weights  DEV double[n_group][ceil(n_time / A) * A][R]: weights[g][t][r] =
 *            (double)counts[g * R + r][t]; the replicates >= n_rep and the
 *            steps >= n_time are padding and hold +0.0
 *   totals   DEV double[n_group * R]: the row sums of the counts
 * so the counts a group needs next are the next bytes.  The caller guarantees
 * counts >= 0 and row sums < 2^31 (engine.resampled_means checks them on the
 * host and builds both tables).  A count is zero iff all bits of its weight
 * are; W = totals minus, with skipna, the counts of the point's NaNs, both
 * exact.
 *
 * A workgroup of 256 threads owns a tile of points and R consecutive
 * replicates, whose chains every thread keeps in registers: a loaded value
 * serves R replicates.  A thread owns adjacent points (16-byte loads where
 * n_point is a multiple of the vector and `in` and `out` are 16-byte aligned,
 * one element per access otherwise, with the same bits) and requests the A
 * time steps after the ones it is combining before it combines any.  The
 * counts do not depend on the thread: they are fetched with scalar loads, and
 * a zero count is a branch the whole wave takes.  With skipna a NaN enters as
 * -0.0 (S + n * (-0.0) has the bits of S: left out).  Grid: (point tiles x
 * replicate groups) x outer indices.  No LDS.
 *
 * Refused before anything is enqueued: an unknown dtype ("unknown dtype");
 * n_rep, n_time or n_point < 1 or a negative n_outer ("bad sizes"); then
 * n_outer == 0 is a no-op; then null `in`, `weights`, `totals` or `out`
 * ("null pointer"); a problem that does not fit a grid ("bad sizes").
 * wb2_resampled_means_geometry: points per workgroup tile (wide != 0: 16-byte
 * loads), the replicates of a group, the time steps a thread requests ahead
 * (4 for float64, 2 for float32; it does not depend on `wide`), and the outer
 * indices per grid row.
 */
int wb2_resampled_means(int dtype, int skipna, const void* in,
                        const int64_t* slab, int64_t n_outer, int32_t n_time,
                        int64_t n_point, const double* weights,
                        const double* totals, int32_t n_rep, double* out,
                        void* stream);
int wb2_resampled_means_geometry(int dtype, int wide, int32_t* tile_points,
                                 int32_t* replicates_per_group,
                                 int32_t* steps_ahead,
                                 int32_t* max_grid_outer);

/*
 * K24: the per-bin sums of conditional verification: the spread-error
 * diagnostic (Leutbecher & Palmer 2008) and the conditional bias (Murphy &
 * Winkler 1987).  The reference has the region means (EnsembleVariance,
 * EnsembleMeanMSE, Bias) and no stratified counterpart.
 *
 * One point with truth y and the members x_0 .. x_{M-1} in STORAGE order
 * (nothing is sorted), all arithmetic in float64 after an exact widening, no
 * fused multiply-add, every product rounded before it is added:
 *   S = x_0;  S = S + x_m  (m = 1 .. M-1);  mu = S / (double)M
 *   d_m = x_m - mu;  Q = d_0 d_0;  Q = Q + d_m d_m  (m = 1 .. M-1)
 *   s2 = Q / (double)(M - 1);  M = 1: s2 = +0.0
 *   e = mu - y;  se = e e
 *   v = s2 (mode 0, spread), mu (mode 1, forecast) or y (mode 2, truth)
 *   bin = #{k : edges[k] <= v}  (searchsorted side='right': a value on an
 *         edge belongs to the upper bin; n_bin = n_edge + 1, the first and the
 *         last bin are open-ended)
 * For mode 0 the caller passes SQUARED edges: variances are compared and no
 * root is taken.  The point is invalid iff the truth or any member is NaN
 * (K18's rule).  Points that hold +-inf are not pinned.
 *
 * wb2_conditional_sums: K20's operands and slab-table convention (ens,
 * ens_slab, truth, truth_slab, n_member, member_stride, n_outer; tables DEV
 * int64, null = identity; col_class DEV int32[n_col] with values in [0,
 * n_class); every table value the caller's to check) and edges, a DEV
 * float64[n_edge], finite and strictly increasing (the caller's to check; null
 * is allowed for n_edge = 0).
 *   sums[o][i][c][b][0..3] (DEV float64, every element written) = the sums of
 *     mu, y, s2 and se over the valid points of bin b among the columns j with
 *     col_class[j] == c in row i of outer index o,
 *   cnt[o][i][c][b] (DEV int32, every element written) = their number.  (The
 *     invalid count is the column count of the class minus the bins' total.)
 * THE ORDER OF THE SUM of one (o, i, c, b, term): one sequential float64 chain
 * s = s + v from +0.0 over the columns of the class in INCREASING COLUMN
 * ORDER, where a point that is invalid or lies in another bin enters as +0.0.
 * A chain started at +0.0 never holds -0.0 (x + (-x) and +0.0 + (-0.0) both
 * round to +0.0), so that +0.0 changes no bit: the chain is the one over the
 * bin's own points.  It does not depend on the tile, on the other classes or
 * bins or on the launch: two runs are bit-equal, and a host loop over the
 * columns reproduces the bits.
 * One wave (a workgroup of its own: rows_per_group = 1) owns one row of one
 * outer index and walks it in tiles of tile_cols = 64 columns.  Per tile a
 * lane requests the truth and the n_member members of its point, all before
 * any is looked at -- each element is read ONCE: (n_member + 1) elements per
 * point --, forms mu, y, s2, se and the bin in registers (lane k keeps edge k;
 * the edges go round by v_readlane) and stores them in a wave-private LDS tile
 * of [4][64] float64 and [64] int32 (bin -1: invalid or past the row end).
 * Then lane b < n_bin takes bin b and walks the points of the tile in column
 * order, eight at a time: it reads the bin and the four values of each point
 * (broadcasts) and adds the value, or +0.0, to each of its four running sums.
 * Where the class of the column changes (wave-uniform) the lane stores its
 * sums and count and takes up those of the new class -- read back from `sums`
 * and `cnt` if the row met the class before, 0 otherwise.  Plain stores; no
 * atomics at all.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 64 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), 0 <= n_edge <= 63 ("n_edge="), the mode ("mode="), a negative
 * member_stride, negative sizes, null pointers ("null pointer") and the grid.
 * Zero n_outer, n_row or n_col is a no-op whatever the pointers are.
 *
 * wb2_conditional_geometry: min_member = 1, max_member = 64 (both dtypes),
 * max_edges = 63, tile_cols = 64, rows_per_group = 1,
 *   lds_bytes = 4 * 64 * 8 + 64 * 4 = 2304,
 * max_grid_outer outer indices per grid row.  The same checks of dtype,
 * n_member, n_class and n_edge.
 *
 * The fold: the sums go through wb2_crps_bin_fold (n_slot = 4 n_bin), the
 * counts through wb2_event_fold (n_code = n_bin + 1: the bins, then invalid).
 */
int wb2_conditional_sums(int dtype, const void* ens, const int64_t* ens_slab,
                         const void* truth, const int64_t* truth_slab,
                         int32_t n_member, int64_t member_stride,
                         int64_t n_outer, int32_t n_row, int32_t n_col,
                         const int32_t* col_class, int32_t n_class, int mode,
                         const double* edges, int32_t n_edge, double* sums,
                         int32_t* cnt, void* stream);
int wb2_conditional_geometry(int dtype, int32_t n_member, int32_t n_class,
                             int32_t n_edge, int32_t* min_member,
                             int32_t* max_member, int32_t* max_edges,
                             int32_t* tile_cols, int32_t* rows_per_group,
                             int64_t* lds_bytes, int32_t* max_grid_outer);

/*
 * K25: the zonal cross-spectrum of forecast and truth, the sufficient
 * statistic of scale-dependent verification (coherence, spectral correlation,
 * amplitude ratio, phase error, error spectrum, effective resolution).  The
 * reference has the spectrum of one field (ZonalEnergySpectrum) and no
 * counterpart.
 *
 * Per outer index o, row i and member m, with N = n_col, NB = N / 2 + 1,
 * F_m = rfft(member row, norm='forward'), T = rfft(truth row, norm='forward'),
 * s_0 = 1 and s_k = 2 otherwise (the Nyquist bin is doubled too, as
 * wb2_zonal_spectrum has it) and C_i = circumference[i]:
 *   sums[o][i][0][k] = power_forecast = sum_m s_k C_i |F_m[k]|^2
 *   sums[o][i][1][k] = power_truth    =       s_k C_i |T[k]|^2
 *   sums[o][i][2][k] = cospectrum     = sum_m s_k C_i Re(F_m[k] conj T[k])
 *   sums[o][i][3][k] = quadrature     = sum_m s_k C_i Im(F_m[k] conj T[k])
 * SIGN: a forecast that is the truth displaced EASTWARD by d degrees has
 * atan2(quadrature, cospectrum) = -2 pi k d / 360 (mod 2 pi).
 * Arithmetic: the transform (K4f's: N / 2 complex points, the plan's twiddle
 * tables, fft_core.hpp) and the products x x + y y, F.x T.x + F.y T.y and
 * F.y T.x - F.x T.y are in the row dtype (whether the compiler contracts them
 * is not pinned); each product is widened to float64 and multiplied once by
 * s_k C_i; the member terms are added in STORAGE order, the first term
 * starting the chain.  The sums are NOT divided by n_member.
 * A row is INVALID iff the truth row or any member row holds a non-finite
 * value (NaN or +-inf): all four terms of the row are +0.0 then.
 *   cnt[o][i][0..1] (DEV int32, every element written) = (1, 0) for a valid
 *   row, (0, 1) for an invalid one.
 *
 * wb2_cross_spectrum_rows: `plan` is a wb2_spectrum_plan_create plan of the
 * same dtype and n_lon = n_col (any n_rows), whose twiddle tables are used;
 * K20's operands and slab-table convention (ens, ens_slab, truth, truth_slab,
 * n_member, member_stride, n_outer; tables DEV int64, null = identity; every
 * table value the caller's to check), slabs of n_row x n_col elements;
 * circumference DEV float64[n_row]; sums DEV float64 [n_outer][n_row][4][NB],
 * every element written.
 * One WAVE owns one row (o, i): it transforms the truth row into an LDS slab
 * of its own (pass 0 straight from memory with non-temporal loads), then every
 * member row into a second slab, recombines both for the bin pairs (k, N / 2 -
 * k) from one pair of LDS reads each and forms the products.  The finiteness
 * test rides on the pass-0 loads (one comparison per loaded value, one wave
 * ballot).  The member sums are kept in the lane's registers and stored once,
 * except for the long rows whose transform leaves no registers for them
 * (float32: N >= 2560; float64: N >= 1800), which keep them in the lane's own
 * elements of `sums`: the same chain, the same bits.  Plain stores, no
 * atomics: two runs are bit-equal.  waves_per_group is fixed per (length,
 * dtype): the most of 4, 2 and 1 whose two slabs per wave and the twq table
 * fit 160 KiB; a launch has at most max_grid_outer workgroups, whose waves
 * stride over the rows.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), an n_col that is not instantiated ("not instantiated", with the
 * list of lengths: the 22 of wb2_zonal_spectrum's one-kernel path),
 * 1 <= n_member <= 128 ("n_member="), a negative member_stride, negative
 * sizes, the alignment of the pass-0 loads (ens and truth on 8 bytes for
 * float32 and 16 for float64, an even member_stride: "aligned"), null
 * pointers ("null pointer"), the grid ("the grid does not fit": more than
 * 2^40 rows) and a plan of another dtype or length ("the plan").  Zero n_outer
 * or n_row is a no-op whatever the pointers are.
 *
 * wb2_cross_spectrum_geometry: supported = 1 for an instantiated n_col (else
 * 0, and the other extents are 0), waves_per_group,
 *   lds_bytes = complex size * ((N / 4 + 2) + waves_per_group * 2 * slab),
 * slab = the complex slots of K4f's padded slab (N / 2 without padding; 840
 * for N = 1440), max_grid_outer = the most workgroups of a launch.  The same
 * checks of dtype and n_member.
 *
 * The fold: the sums go through wb2_crps_bin_fold (n_class = 1, n_slot = 4
 * NB, mult = 1), the flags through wb2_event_fold (n_code = 2).
 */
int wb2_cross_spectrum_rows(void* plan, int dtype, const void* ens,
                            const int64_t* ens_slab, const void* truth,
                            const int64_t* truth_slab, int32_t n_member,
                            int64_t member_stride, int64_t n_outer,
                            int32_t n_row, int32_t n_col,
                            const double* circumference, double* sums,
                            int32_t* cnt, void* stream);
int wb2_cross_spectrum_geometry(int dtype, int32_t n_col, int32_t n_member,
                                int32_t* supported, int32_t* waves_per_group,
                                int64_t* lds_bytes, int32_t* max_grid_outer);

/*
 * K26: the joint frequency table of forecast and truth CATEGORIES (Murphy &
 * Winkler 1987), the sufficient statistic of distributions-oriented
 * verification: the multi-category scores (proportion correct, Heidke, Peirce,
 * Gerrity), both marginal histograms and the two factorisations.  The
 * reference has no counterpart, and K18's per-threshold 2 x 2 tables cannot
 * give the cross terms (truth below edge 1 AND forecast above edge 2).
 *
 * With E = n_edge edges, B = E + 1 categories (the outer two open-ended):
 *   side 0 (right):  bin(v) = #{k : edges[k] <= v}  (searchsorted side=
 *                    'right': a value on an edge belongs to the upper
 *                    category; K24's rule)
 *   side 1 (left):   bin(v) = #{k : edges[k] <  v}  (being above edge k is
 *                    K18's event v > edges[k])
 * IEEE comparisons in float64 after an exact widening; +-inf are ordinary
 * values and land in the outer categories.  The point is invalid iff the truth
 * or any member is NaN (K18's rule).  One set of edges serves both.
 *
 * wb2_joint_counts: K20's operands and slab-table convention (ens, ens_slab,
 * truth, truth_slab, n_member, member_stride, n_outer; tables DEV int64, null
 * = identity; col_class DEV int32[n_col] with values in [0, n_class); every
 * table value the caller's to check) and edges, a DEV float64[n_edge], finite
 * and strictly increasing (the caller's to check; null is allowed for n_edge =
 * 0).  n_code = B * B + 1 and
 *   cnt[o][i][c][code] (DEV int32, every element written): over the columns j
 *   with col_class[j] == c in row i of outer index o,
 *     code = bin(y) * B + bin(x_m)  gets +1 PER MEMBER m of a valid point,
 *     code = B * B                  gets +1 per invalid point.
 *   The valid codes of a (row, class) sum to n_member x its valid points.
 * A workgroup of 256 threads owns rows_per_group adjacent rows of one outer
 * index and walks that contiguous run: 16-byte lanes where `ens` and `truth`
 * are 16-byte aligned and n_col and member_stride are whole lanes (4 float32,
 * 2 float64), one element per access otherwise; the bits are the same.  The
 * edges are wave-uniform: each is read once per workgroup by a uniform load
 * and kept in a register (those past n_edge are NaN).  side 1 is turned into
 * side 0 there: for a finite e, e < v exactly where succ(e) <= v, succ = the
 * next float64 up.  A point's validity is known only after its last member, so
 * nothing reaches the histogram before: per point and edge k a thread keeps g_k
 * = the members at or above edge k (<= 128: packed 8-bit counters, every index
 * a compile-time constant); category b then holds g_{b-1} - g_b members (g_{-1}
 * = n_member, g_B = 0) and the non-zero ones are added to an LDS histogram
 * [row][class][code] with workgroup-scope integer atomics.  The members are
 * requested four at a time before any is compared; each element is read ONCE,
 * (n_member + 1) elements per point.  After a barrier the histogram is stored
 * with plain stores.  Integer adds commute: two runs are bit-equal.  No global
 * atomics, no float atomics.  The kernel is instantiated for 4, 8, 12, 16, 24
 * and 32 edge slots; a call takes the least that holds n_edge.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 128 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), 0 <= n_edge <= 31 ("n_edge="), the histogram of one row
 * against the budget ("LDS budget"), side ("side="), a negative
 * member_stride, negative sizes, null pointers ("null pointer"), a row group
 * of 2^30 elements or more ("too long") and the grid.  Zero n_outer, n_row or
 * n_col is a no-op whatever the pointers are.
 *
 * wb2_joint_counts_geometry: rows_per_group = the most of 4, 2, 1 whose
 * histogram fits 65536 bytes (K18's budget),
 *   lds_bytes = rows_per_group * n_class * (B * B + 1) * 4,
 * max_edges = 31, max_grid_outer outer indices per grid row.  `wide` (16-byte
 * lanes) changes none of them.  The same checks of dtype, n_member, n_class,
 * n_edge and the budget, with the same error text.
 *
 * The fold: wb2_event_fold with n_code = B * B + 1,
 *   table[o][r][code] = sum_i wrow[r][i] *
 *                       (double)(sum_c mult[r][c] * cnt[o][i][c][code]),
 * the inner sum in int64, the rows in increasing order.  The caller divides
 * the B * B valid codes by their total, n_member x the valid mass.
 */
int wb2_joint_counts(int dtype, const void* ens, const int64_t* ens_slab,
                     const void* truth, const int64_t* truth_slab,
                     int32_t n_member, int64_t member_stride, int64_t n_outer,
                     int32_t n_row, int32_t n_col, const int32_t* col_class,
                     int32_t n_class, const double* edges, int32_t n_edge,
                     int side, int32_t* cnt, void* stream);
int wb2_joint_counts_geometry(int dtype, int32_t n_member, int32_t n_class,
                              int32_t n_edge, int wide,
                              int32_t* rows_per_group, int64_t* lds_bytes,
                              int32_t* max_edges, int32_t* max_grid_outer);

/*
 * K27: the structure functions of forecast and truth and the variogram score
 * (Scheuerer & Hamill 2015): the verification of the DIFFERENCES between grid
 * points, which the pointwise tables and the energy score (Pinson & Tastu
 * 2013) are nearly blind to.  The reference has no counterpart.
 *
 * A lag is a pair of grid offsets (a, b): a >= 0 in rows, counted in the order
 * the rows are handed over, b in columns (may be negative), (a, b) != (0, 0).
 * The partner of the anchor (i, j) is (i + a, (j + b) mod n_col): the columns
 * are cyclic.  The pair exists iff i + a < n_row.  The offsets are in GRID
 * POINTS, the same count in every row (the convention of K19 and K22).
 * One existing pair with truth y, y' and the members x_m, x'_m in STORAGE
 * order, all arithmetic in float64 after an exact widening, no fused
 * multiply-add, every product rounded before it is added:
 *   g(d) = |d|            (order_code 1: order 1)
 *        = d * d          (order_code 2: order 2)
 *        = sqrt_rn(|d|)   (order_code 0: order 0.5, the correctly rounded root)
 *   gy = g(y - y')
 *   G = g(x_0 - x'_0);  G = G + g(x_m - x'_m)  (m = 1 .. M-1);  gf = G / (double)M
 *   s = gy - gf;  sc = s * s
 * The pair is invalid iff any of y, y', x_m, x'_m is NaN (K18's rule, at both
 * ends).  Pairs that hold +-inf are not pinned.  A pair that does not exist is
 * neither valid nor invalid.
 *
 * wb2_variogram_sums: K20's operands and slab-table convention (ens, ens_slab,
 * truth, truth_slab, n_member, member_stride, n_outer; tables DEV int64, null
 * = identity; col_class DEV int32[n_col] with values in [0, n_class); every
 * table value the caller's to check) and lags, a HOST int32[n_lag][2] of (a,
 * b) pairs, read before the call returns.
 *   sums[o][i][c][l][0..2] (DEV float64, every element written) = the sums of
 *     gy, gf and sc over the valid pairs of lag l whose anchor lies in row i of
 *     outer index o, in a column j with col_class[j] == c,
 *   cnt[o][i][c][l][0..1] (DEV int32, every element written) = the number of
 *     valid and of invalid pairs among them.
 * THE ORDER OF THE SUM of one (o, i, c, l, term): one sequential float64 chain
 * s = s + v from +0.0 over the columns of the class in INCREASING COLUMN
 * ORDER, where a pair that is invalid or does not exist enters as +0.0.  A
 * chain started at +0.0 never holds -0.0, so that +0.0 changes no bit: the
 * chain is the one over the valid pairs.  It does not depend on the tile, on
 * the other classes or lags or on the launch: two runs are bit-equal, and a
 * host loop over the columns reproduces the bits.
 * Weighting is the caller's: a pair carries the weight of its ANCHOR, so a
 * region owns the pairs whose anchor it holds, wherever the partner lies.
 * One wave (a workgroup of its own: rows_per_group = 1) owns one anchor row of
 * one outer index and walks it in tiles of tile_cols = 64 columns.  The truth
 * ("member -1") and the members go through wave-private LDS strips, four items
 * at a time: per item and per DISTINCT row offset among the lags (0 always)
 * the wave requests the tile's 64 columns of that row and the halo that the
 * lags of that row offset reach to the left and to the right, the index
 * wrapped at the seam; the four items of up to five row offsets are requested
 * before any is stored.  A strip holds 64 + 2 * max_col_offset = 128 columns.
 * Column-shifted partners are read from the strips, never from memory again: a
 * lane issues 1 + (distinct non-zero row offsets the row reaches) requests per
 * member, plus the halos' share, not 1 + n_lag.  Each lane keeps gy, G and one
 * invalid bit per lag in registers, every index a compile-time constant; the
 * kernel is instantiated per dtype and order for 4, 8 and 16 lag slots and a
 * call takes the least that holds n_lag.  After the last member the lane
 * stores gy, gf, sc of every lag -- +0.0 where the pair is invalid or absent --
 * and a word of the pairs' states into an LDS tile [point][3 n_lag | 1] that
 * takes the strips' place.  Then lane s < 3 n_lag takes slot s = 3 l + term and
 * adds the points of the tile in column order, eight LDS reads in flight (K24's
 * walk); lanes 3 l and 3 l + 1 count the valid and the invalid pairs.  Where
 * the class of the column changes (wave-uniform) the lane stores its sum and
 * takes up the new class's -- read back from `sums` and `cnt` if the row met
 * the class before, 0 otherwise.  Plain stores; no atomics at all.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 128 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), 1 <= n_lag <= 16 ("n_lag="), the order code ("order_code="),
 * a null `lags` ("null pointer"), per lag 0 <= a <= 16 ("row offset"), |b| <=
 * 32 ("column offset"), |b| < n_col ("below n_col"; not where n_col = 0) and
 * (a, b) != (0, 0) ("(0, 0)"), the strips and the tile against the budget of
 * 65536 bytes ("LDS budget"), a negative member_stride, negative sizes, null
 * pointers ("null pointer"), a row of 2^28 elements or more ("too long") and
 * the grid.  Zero n_outer, n_row or n_col is a no-op whatever the pointers are.
 *
 * wb2_variogram_geometry: min_member = 1, max_member = 128, max_lags = 16,
 * max_row_offset = 16, max_col_offset = 32, tile_cols = 64, rows_per_group =
 * 1,
 *   lds_bytes = max(4 * n_off * 128 * sizeof(dtype), 64 * (3 n_lag | 1) * 8)
 *               + 256   (n_off = the distinct row offsets of `lags`, 0 among
 *               them; the 256 bytes are the states of the 64 points),
 * max_grid_outer outer indices per grid row.  The same checks of dtype,
 * n_member, n_class, n_lag, the order code, the lags (but for |b| < n_col) and
 * the budget, with the same error text: float64 lags with 16 or more distinct
 * row offsets do not fit.
 *
 * The fold: the sums go through wb2_crps_bin_fold (n_slot = 3 n_lag), the
 * counts through wb2_event_fold (n_code = 2 n_lag: per lag valid, invalid).
 */
int wb2_variogram_sums(int dtype, const void* ens, const int64_t* ens_slab,
                       const void* truth, const int64_t* truth_slab,
                       int32_t n_member, int64_t member_stride,
                       int64_t n_outer, int32_t n_row, int32_t n_col,
                       const int32_t* col_class, int32_t n_class,
                       int order_code, const int32_t* lags, int32_t n_lag,
                       double* sums, int32_t* cnt, void* stream);
int wb2_variogram_geometry(int dtype, int32_t n_member, int32_t n_class,
                           int order_code, const int32_t* lags, int32_t n_lag,
                           int32_t* min_member, int32_t* max_member,
                           int32_t* max_lags, int32_t* max_row_offset,
                           int32_t* max_col_offset, int32_t* tile_cols,
                           int32_t* rows_per_group, int64_t* lds_bytes,
                           int32_t* max_grid_outer);

/*
 * K28: the sums behind the verification of QUANTILE forecasts: the pinball
 * (quantile) loss, the forecast quantile, and how often the truth lies below
 * or on it -- the quantile score, quantile reliability and the coverage, width
 * and interval score (Winkler 1972) of central prediction intervals are host
 * arithmetic on them.  The reference has no counterpart.
 *
 * One point, truth y, level l, all arithmetic in float64 after an exact
 * widening, no fused multiply-add, every product rounded before it is added:
 *   mode 0 (sorted ensemble): the M members sorted x_0 <= ... <= x_{M-1};
 *     d = x_hi[l] - x_lo[l] in the DATA's dtype;
 *     q = x_lo + d t[l]             (t[l] < 1/2)
 *       = x_hi - d (1 - t[l])       (otherwise: K12's interpolation)
 *   mode 1 (direct): the M "members" are quantile values in STORAGE order;
 *     q = x_lo[l]; nothing is sorted, nothing interpolated; lo == hi
 *   u = y - q;  pinball = tau[l] u (u >= 0), one_minus_tau[l] (-u) (otherwise)
 *   below = y < q;  tie = y == q   (IEEE compares: -0.0 ties with +0.0)
 * The point is invalid iff the truth or any member is NaN (K18's rule).
 * Points that hold +-inf are not pinned.  The kernel knows no quantile method:
 * lo, hi, t, tau and one_minus_tau are HOST tables of n_level entries, read
 * before the call returns.
 *
 * wb2_quantile_score_sums: K20's operands and slab-table convention (ens,
 * ens_slab, truth, truth_slab, n_member, member_stride, n_outer; tables DEV
 * int64, null = identity; col_class DEV int32[n_col] with values in [0,
 * n_class); every table value the caller's to check).
 *   sums[o][i][c][l][0..1] (DEV float64, every element written) = the sums of
 *     pinball and q over the valid points of row i of outer index o in the
 *     columns j with col_class[j] == c,
 *   cnt[o][i][c][l][0..1] (DEV int32, every element written) = the number of
 *     those points with `below` and with `tie`,
 *   valid[o][i][c][0..1] (DEV int32, every element written) = the number of
 *     valid and of invalid points of the (row, class).
 * THE ORDER OF THE SUM of one (o, i, c, l, term): one sequential float64 chain
 * s = s + v from +0.0 over the columns of the class in INCREASING COLUMN
 * ORDER, where an invalid point enters as +0.0.  A chain started at +0.0
 * never holds -0.0, so that +0.0 changes no bit.  It does not depend on the
 * tile, on the other classes or levels or on the launch: two runs are
 * bit-equal, and a host loop over the columns reproduces the bits.
 * One wave (a workgroup of its own: rows_per_group = 1) owns one row of one
 * outer index and walks it in tiles of tile_cols = 64 columns.  A lane
 * requests its point's class, truth and members, all before any is looked at,
 * sorts the members in registers (mode 0; the networks padded to 2, 4, ..,
 * 64) and stores them in a wave-private LDS tile [M][64]; per level it reads
 * x_lo and x_hi back at the wave-uniform rows lo[l], hi[l] and keeps q,
 * pinball and the flags under compile-time indices (instantiated per dtype and
 * padded member count for 4, 8 and 16 level slots; a call takes the least that
 * holds n_level).  The values -- +0.0 where the point is invalid -- go into an
 * LDS tile [point][2 n_level | 1] that takes the members' place, the flags as
 * one word per point.  Then lane s < 2 n_level takes slot s = 2 l + term and
 * adds the points in column order, eight LDS reads in flight (K24's walk);
 * lane 2 l counts below, lane 2 l + 1 tie; the valid and invalid counts come
 * from two ballots.  At a class change (wave-uniform) the lane stores its sum
 * and takes up the new class's -- read back if the row met the class before, 0
 * otherwise.  Plain stores; no atomics at all.
 * Checked before anything is enqueued, in this order: the dtype ("unknown
 * dtype"), 1 <= n_member <= 64 ("n_member="), 1 <= n_class <= 64
 * ("n_class="), the mode ("mode="), 1 <= n_level <= 16 ("n_level="), the tile
 * against the budget of 65536 bytes ("LDS budget"), null tables ("null
 * pointer"), per level 0 <= lo <= hi < n_member and, in mode 1, lo == hi
 * ("positions"), a negative member_stride, negative sizes, null pointers
 * ("null pointer"), a row of 2^28 elements or more ("too long") and the grid.
 * Zero n_outer, n_row or n_col is a no-op whatever the pointers are.
 *
 * wb2_quantile_score_geometry: min_member = 1, max_member = 64, max_levels =
 * 16, tile_cols = 64, rows_per_group = 1,
 *   lds_bytes = max(n_member * 64 * sizeof(dtype), 64 * (2 n_level | 1) * 8)
 *               + 256   (the 256 bytes are the flag words of the 64 points),
 * max_grid_outer outer indices per grid row.  The same checks of dtype,
 * n_member, n_class, mode, n_level and the budget, with the same error text.
 *
 * The fold: the sums go through wb2_crps_bin_fold (n_slot = 2 n_level), the
 * counts through wb2_event_fold (n_code = 2 n_level + 2: per level below, tie,
 * then valid, invalid).
 */
int wb2_quantile_score_sums(int dtype, const void* ens, const int64_t* ens_slab,
                            const void* truth, const int64_t* truth_slab,
                            int32_t n_member, int64_t member_stride,
                            int64_t n_outer, int32_t n_row, int32_t n_col,
                            const int32_t* col_class, int32_t n_class, int mode,
                            int32_t n_level, const int32_t* lo,
                            const int32_t* hi, const double* t,
                            const double* tau, const double* one_minus_tau,
                            double* sums, int32_t* cnt, int32_t* valid,
                            void* stream);
int wb2_quantile_score_geometry(int dtype, int32_t n_member, int32_t n_class,
                                int mode, int32_t n_level,
                                int32_t* min_member, int32_t* max_member,
                                int32_t* max_levels, int32_t* tile_cols,
                                int32_t* rows_per_group, int64_t* lds_bytes,
                                int32_t* max_grid_outer);

#ifdef __cplusplus
}
#endif
#endif  /* WB2HIP_H_ */
