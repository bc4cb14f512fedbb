"""The metric layer's region dispatch on the GPU (-m gpu): for every public
metric class, one region at a time equals all regions at once, bit for bit,
and both agree with the NumPy oracle at the tolerance of the class's family
suite.  Small shapes: a 6 x 7 grid (rows of one 4-wide float32 vector and a
tail), 2 times, 2 levels, 1 and 3 members, thresholds at two quantiles, and
three regions of which one selects no row (total weight 0)."""
import functools

import numpy as np
import pytest

from oracle import metrics_np as om
from oracle import regions_np as oreg
from oracle import thresholds_np as oth
from oracle.named import DS, NA
from tests import helpers

pytestmark = pytest.mark.gpu

g = helpers.to_gpu_dataset
N_LAT, N_LON, N_TIME, N_LEVEL = 6, 7, 2, 2
LAT = np.linspace(-75.0, 75.0, N_LAT)
LON = np.arange(N_LON) * (360.0 / N_LON)
TIME = np.array(['2020-01-01', '2020-01-02'], dtype='datetime64[ns]')
LEVEL = np.array([500, 850])
COORDS = {'time': TIME, 'level': LEVEL, 'latitude': LAT, 'longitude': LON}
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (N_TIME, N_LEVEL, N_LAT, N_LON)
QUANTILES = (0.3, 0.8)
PRECIP = 'total_precipitation_24hr'

OREGIONS = {
    'global': oreg.SliceRegion(),
    'band': oreg.SliceRegion(lat_slice=slice(-20, 50)),
    'empty': oreg.SliceRegion(lat_slice=slice(80, 85)),   # no row: weight 0
}

# tolerances of the family suites against the oracle
TOL_DET = dict(rtol=1e-9, atol=1e-12)      # test_det_gpu (RTOL), float64 data
TOL_ENS32 = dict(rtol=2e-6, atol=1e-7)     # test_ens_gpu, float32 members
TOL_TIER2 = dict(rtol=1e-9, atol=1e-12)    # test_tier2_gpu, test_thresholds_gpu
# compute_chunk + time mean against compute, as the family suites compare them
TOL_MAP_MEAN = dict(rtol=2e-7, atol=1e-7)       # test_spatial_gpu
TOL_ENS_MAP_MEAN = dict(rtol=3e-6, atol=1e-6)   # test_ens_gpu (Spatial*)
TOL_THR_MAP_MEAN = dict(rtol=1e-12, atol=1e-14)  # test_thresholds_gpu
TOL_SEEPS_MAP_MEAN = dict(rtol=1e-6, atol=1e-14)  # test_thresholds_gpu
TOL_RANK_MEAN = dict(rtol=0, atol=1e-15)        # test_rank_histogram_gpu


@pytest.fixture(scope='module')
def gm():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  from weatherbench2_amd import metrics as gm
  return gm


def gregions():
  return {k: helpers.to_gpu_region(v) for k, v in OREGIONS.items()}


def _rs(seed):
  return np.random.RandomState(seed)


@functools.lru_cache(maxsize=None)
def det_case(dtype=np.float64):
  rs = _rs(1)
  names = ('z', 'u', 'v')
  truth = DS({k: NA(rs.normal(size=SHAPE).astype(dtype), DIMS) for k in names},
             COORDS)
  forecast = DS({k: NA(rs.normal(size=SHAPE).astype(dtype), DIMS)
                 for k in names}, COORDS)
  return forecast, truth


@functools.lru_cache(maxsize=None)
def climatology_case():
  rs = _rs(2)
  dims = ('hour', 'dayofyear', 'level', 'latitude', 'longitude')
  shape = (1, 366, N_LEVEL, N_LAT, N_LON)
  coords = dict(COORDS, hour=np.array([0]), dayofyear=1 + np.arange(366))
  del coords['time']
  return DS({k: NA(rs.normal(size=shape), dims) for k in ('z', 'u', 'v')},
            coords)


@functools.lru_cache(maxsize=None)
def ens_case(n_member, dtype=np.float32):
  rs = _rs(3 + n_member)
  truth = DS({'z': NA(rs.normal(size=SHAPE).astype(dtype), DIMS)}, COORDS)
  forecast = DS(
      {'z': NA(rs.normal(size=(n_member,) + SHAPE).astype(dtype),
               ('realization',) + DIMS)},
      dict(COORDS, realization=np.arange(n_member)))
  return forecast, truth


@functools.lru_cache(maxsize=None)
def gauss_case():
  rs = _rs(7)
  truth = DS({'z': NA(rs.normal(size=SHAPE), DIMS)}, COORDS)
  forecast = DS({'z': NA(rs.normal(size=SHAPE), DIMS),
                 'z_std': NA(np.abs(rs.normal(size=SHAPE)) + 0.2, DIMS)},
                COORDS)
  return forecast, truth


@functools.lru_cache(maxsize=None)
def threshold_climatology():
  rs = _rs(8)
  dims = ('dayofyear', 'level', 'latitude', 'longitude')
  shape = (366, N_LEVEL, N_LAT, N_LON)
  coords = dict(COORDS, dayofyear=1 + np.arange(366))
  del coords['time']
  return DS({'z': NA(0.1 * rs.normal(size=shape), dims),
             'z_std': NA(np.abs(rs.normal(size=shape)) + 0.5, dims)}, coords)


def thresholds(gpu: bool):
  clim = threshold_climatology()
  if not gpu:
    return [oth.GaussianQuantileThreshold(clim, q) for q in QUANTILES]
  from weatherbench2_amd import thresholds as gth
  return [gth.GaussianQuantileThreshold(climatology=_shared_g(clim), quantile=q)
          for q in QUANTILES]


@functools.lru_cache(maxsize=None)
def seeps_case():
  rs = _rs(9)
  dims = ('time', 'latitude', 'longitude')
  shape = (N_TIME, N_LAT, N_LON)
  coords = {'time': TIME, 'valid_time': TIME, 'latitude': LAT,
            'longitude': LON}
  mk = lambda: DS({PRECIP: NA(np.abs(rs.normal(size=shape)) * 2e-3, dims)},
                  coords)
  forecast, truth = mk(), mk()
  cdims = ('hour', 'dayofyear', 'latitude', 'longitude')
  cshape = (1, 366, N_LAT, N_LON)
  climatology = DS({
      f'{PRECIP}_seeps_dry_fraction': NA(
          rs.uniform(0.02, 0.98, size=cshape), cdims),
      f'{PRECIP}_seeps_threshold': NA(
          rs.uniform(1e-3, 3e-3, size=cshape), cdims)},
      {'hour': np.array([0]), 'dayofyear': 1 + np.arange(366),
       'latitude': LAT, 'longitude': LON})
  return forecast, truth, climatology


@functools.lru_cache(maxsize=None)
def _shared_g(ds):
  """One product Dataset per oracle dataset (metric objects cache by it)."""
  return g(ds)


def _cases():
  """name -> (oracle metric, product metric factory(gm), forecast, truth,
  tolerance, has the `ensemble_size` attr)."""
  out = {}
  det = det_case()
  for name in ('MSE', 'RMSESqrtBeforeTimeAvg', 'MAE', 'Bias'):
    out[name] = (getattr(om, name)(), lambda gm, n=name: getattr(gm, n)(),
                 *det, TOL_DET)
  for name in ('WindVectorMSE', 'WindVectorRMSESqrtBeforeTimeAvg'):
    out[name] = (getattr(om, name)('u', 'v', 'wind'),
                 lambda gm, n=name: getattr(gm, n)('u', 'v', 'wind'), *det,
                 TOL_DET)
  wv = lambda m, cls: [getattr(m, cls)('u', 'v', 'wind')]
  out['MSE+wind'] = (
      om.MSE(wind_vector_mse=wv(om, 'WindVectorMSE')),
      lambda gm: gm.MSE(wind_vector_mse=wv(gm, 'WindVectorMSE')), *det,
      TOL_DET)
  out['RMSE+wind'] = (
      om.RMSESqrtBeforeTimeAvg(
          wind_vector_rmse=wv(om, 'WindVectorRMSESqrtBeforeTimeAvg')),
      lambda gm: gm.RMSESqrtBeforeTimeAvg(
          wind_vector_rmse=wv(gm, 'WindVectorRMSESqrtBeforeTimeAvg')), *det,
      TOL_DET)
  clim = climatology_case()
  out['ACC'] = (om.ACC(clim), lambda gm: gm.ACC(_shared_g(clim)), *det,
                TOL_DET)
  for m in (1, 3):
    for name in ('CRPS', 'CRPSSpread', 'CRPSSkill',
                 'EnsembleStddevSqrtBeforeTimeAvg', 'EnsembleVariance',
                 'EnsembleMeanRMSESqrtBeforeTimeAvg', 'EnsembleMeanMSE',
                 'DebiasedEnsembleMeanMSE'):
      out[f'{name}/M={m}'] = (getattr(om, name)(),
                              lambda gm, n=name: getattr(gm, n)(),
                              *ens_case(m), TOL_ENS32)
    for name in ('EnergyScore', 'EnergyScoreSpread', 'EnergyScoreSkill'):
      out[f'{name}/M={m}'] = (getattr(om, name)(),
                              lambda gm, n=name: getattr(gm, n)(),
                              *ens_case(m, np.float64), TOL_TIER2)
    for name in ('EnsembleBrierScore', 'DebiasedEnsembleBrierScore',
                 'EnsembleIgnoranceScore', 'EnsembleRPS'):
      out[f'{name}/M={m}'] = (
          getattr(om, name)(thresholds=thresholds(False)),
          lambda gm, n=name: getattr(gm, n)(thresholds=thresholds(True)),
          *ens_case(m, np.float64), TOL_TIER2)
  for name in ('GaussianCRPS', 'GaussianVariance'):
    out[name] = (getattr(om, name)(), lambda gm, n=name: getattr(gm, n)(),
                 *gauss_case(), TOL_TIER2)
  for name in ('GaussianBrierScore', 'GaussianIgnoranceScore', 'GaussianRPS'):
    out[name] = (getattr(om, name)(thresholds=thresholds(False)),
                 lambda gm, n=name: getattr(gm, n)(thresholds=thresholds(True)),
                 *gauss_case(), TOL_TIER2)
  sf, st, sclim = seeps_case()
  out['SEEPS'] = (om.SEEPS(climatology=sclim),
                  lambda gm: gm.SEEPS(climatology=_shared_g(sclim)), sf, st,
                  TOL_TIER2)
  return out


CASES = _cases()


def _host(ds):
  """{variable: (dims, dtype, values)} + coords + attrs, on the host."""
  from weatherbench2_amd import xarray_lite as xl
  ds = xl.as_dataset(ds)
  data = {k: (tuple(v.dims), np.asarray(v.values).dtype, np.asarray(v.values))
          for k, v in ds.data_vars.items()}
  coords = {k: (tuple(c.dims) if isinstance(c, xl.DataArray) else None,
                np.asarray(c.values if isinstance(c, xl.DataArray) else c))
            for k, c in ds.coords.items()}
  return data, coords, dict(ds.attrs)


def _assert_identical(got, want, what):
  gd, gc, ga = _host(got)
  wd, wc, wa = _host(want)
  assert list(gd) == list(wd), what
  for k in wd:
    assert gd[k][0] == wd[k][0], (what, k)           # dims
    assert gd[k][1] == wd[k][1], (what, k)           # dtype
    np.testing.assert_array_equal(gd[k][2], wd[k][2], err_msg=f'{what}/{k}')
  assert sorted(gc) == sorted(wc), what
  for k in wc:
    assert gc[k][0] == wc[k][0], (what, k)
    np.testing.assert_array_equal(gc[k][1], wc[k][1], err_msg=f'{what}/{k}')
  assert ga == wa, what


def _stacked(fn, regions):
  """evaluation.py:416-430: one call per region, expand_dims, concat -- inside
  the announcement of the loop's regions, as `_metric_and_region_loop` and
  `Metric._fan_out` make these calls: every region is then read off ONE pass.
  (A bare single-region call outside any announcement runs a pass of its own,
  over a plan with that one region; its float64 partial sums fold in another
  order, and the last bit may differ from the all-regions pass -- before the
  shared dispatch as after it: 94 of 558 (class, variable, region) results of
  these fixtures, by at most 2.5e-16 relative.)"""
  from weatherbench2_amd import metrics as gm
  from weatherbench2_amd import xarray_lite as xl
  with gm.fused_regions(regions):
    return xl.concat([xl.as_dataset(fn(region)).expand_dims({'region': [name]})
                      for name, region in regions.items()], 'region')


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_regions_at_once_equal_one_by_one_and_the_oracle(gm, name, skipna):
  ometric, make, forecast, truth, tol = CASES[name]
  metric, gf, gt, regions = make(gm), g(forecast), g(truth), gregions()
  every = metric.compute_chunk_regions(gf, gt, regions, skipna)
  assert every[list(every.data_vars)[0]].dims[0] == 'region'
  _assert_identical(
      every, _stacked(lambda r: metric.compute_chunk(gf, gt, region=r,
                                                     skipna=skipna), regions),
      f'{name}/compute_chunk')
  mean = metric.compute_regions(gf, gt, regions, skipna)
  _assert_identical(
      mean, _stacked(lambda r: metric.compute(gf, gt, region=r, skipna=skipna),
                     regions), f'{name}/compute')
  assert ('ensemble_size' in mean.attrs) == ('realization' in forecast.dims)
  for ri, (rname, region) in enumerate(OREGIONS.items()):
    with np.errstate(all='ignore'):
      want = ometric.compute_chunk(forecast, truth, region=region,
                                   skipna=skipna)
    assert sorted(want.keys()) == sorted(every.data_vars), name
    for var in want.keys():
      assert every[var].dims == ('region',) + tuple(want[var].dims), (name, var)
      helpers.assert_close(every[var].values[ri], want[var].data, **tol,
                           err_msg=f'{name}/{rname}/{var}')


def _map_cases():
  """name -> (oracle metric, product factory, forecast, truth, tolerance of
  compute_chunk + mean against compute)."""
  out = {}
  det32 = det_case(np.float32)
  for name in ('SpatialMSE', 'SpatialMAE', 'SpatialBias'):
    out[name] = (getattr(om, name)(), lambda gm, n=name: getattr(gm, n)(),
                 *det32, TOL_MAP_MEAN)
  for m in (1, 3):
    for name in ('SpatialCRPS', 'SpatialCRPSSpread', 'SpatialCRPSSkill',
                 'SpatialEnsembleVariance', 'SpatialEnsembleMeanMSE',
                 'DebiasedSpatialEnsembleMeanMSE'):
      out[f'{name}/M={m}'] = (getattr(om, name)(),
                              lambda gm, n=name: getattr(gm, n)(),
                              *ens_case(m), TOL_ENS_MAP_MEAN)
    for name in ('SpatialEnsembleBrierScore',
                 'SpatialDebiasedEnsembleBrierScore',
                 'SpatialEnsembleIgnoranceScore', 'SpatialEnsembleRPS'):
      out[f'{name}/M={m}'] = (
          getattr(om, name)(thresholds=thresholds(False)),
          lambda gm, n=name: getattr(gm, n)(thresholds=thresholds(True)),
          *ens_case(m, np.float64), TOL_THR_MAP_MEAN)
    out[f'RankHistogram/M={m}'] = (
        om.RankHistogram(), lambda gm: gm.RankHistogram(seed=5), *ens_case(m),
        TOL_RANK_MEAN)
  sf, st, sclim = seeps_case()
  out['SpatialSEEPS'] = (om.SpatialSEEPS(climatology=sclim),
                         lambda gm: gm.SpatialSEEPS(climatology=_shared_g(sclim)),
                         sf, st, TOL_SEEPS_MAP_MEAN)
  return out


MAP_CASES = _map_cases()


@pytest.mark.parametrize('name', list(MAP_CASES))
def test_map_chunk_then_time_mean_equals_compute(gm, name):
  ometric, make, forecast, truth, tol = MAP_CASES[name]
  metric, gf, gt = make(gm), g(forecast), g(truth)
  chunk = metric.compute_chunk(gf, gt)
  with np.errstate(all='ignore'):
    want = ometric.compute_chunk(forecast, truth)
  whole = metric.compute(gf, gt)
  for var in want.keys():
    assert chunk[var].dims == tuple(want[var].dims), (name, var)
    values = np.asarray(chunk[var].values, dtype=np.float64)
    axis = chunk[var].dims.index('time')
    assert whole[var].dims == tuple(d for d in chunk[var].dims if d != 'time')
    helpers.assert_close(whole[var].values, values.mean(axis), **tol,
                         err_msg=f'{name}/{var}')
  assert ('ensemble_size' in whole.attrs) == ('realization' in forecast.dims)
  # maps have no regions: one region at a time, stacked
  regions = gregions()
  _assert_identical(
      metric.compute_chunk_regions(gf, gt, regions),
      _stacked(lambda r: metric.compute_chunk(gf, gt, region=r), regions),
      f'{name}/compute_chunk')


@pytest.mark.parametrize('truth_dtype', [np.float64, np.int32])
def test_mixed_input_dtypes(gm, truth_dtype):
  """float32 forecast with a float64 / an int32 truth: one common dtype per
  pass, the same whichever way the regions are asked for."""
  forecast, truth = det_case(np.float32)
  truth = DS({k: NA((10 * v.data).astype(truth_dtype), DIMS)
              for k, v in truth.items()}, COORDS)
  ens, _ = ens_case(3)
  etruth = DS({'z': truth['z']}, COORDS)
  regions = gregions()
  for metric, gf, gt, of, ot, ometric in (
      (gm.MSE(), g(forecast), g(truth), forecast, truth, om.MSE()),
      (gm.CRPS(), g(ens), g(etruth), ens, etruth, om.CRPS())):
    every = metric.compute_chunk_regions(gf, gt, regions)
    _assert_identical(
        every, _stacked(lambda r: metric.compute_chunk(gf, gt, region=r),
                        regions), type(metric).__name__)
    if truth_dtype == np.float64:   # both sides subtract in float64
      tol = TOL_DET if isinstance(metric, gm.MSE) else TOL_ENS32
      for ri, region in enumerate(OREGIONS.values()):
        with np.errstate(all='ignore'):
          want = ometric.compute_chunk(of, ot, region=region)
        helpers.assert_close(every['z'].values[ri], want['z'].data, **tol)


def test_one_member_cases(gm):
  forecast, truth = ens_case(1)
  gf, gt, regions = g(forecast), g(truth), gregions()
  names = list(regions)
  spread = gm.CRPSSpread().compute_chunk_regions(gf, gt, regions)['z'].values
  assert np.isnan(spread[names.index('empty')]).all()
  for k in ('global', 'band'):
    assert (spread[names.index(k)] == 0).all()
  assert (gm.EnsembleVariance().compute_chunk_regions(
      gf, gt, regions)['z'].values == 0).all()
  assert np.isnan(gm.DebiasedEnsembleMeanMSE().compute_chunk_regions(
      gf, gt, regions)['z'].values).all()
  for name in ('CRPSSpread', 'EnsembleVariance'):   # one region at a time too
    one = getattr(gm, name)().compute_chunk(gf, gt, region=regions['empty'])
    assert np.isnan(one['z'].values).all() == (name == 'CRPSSpread')


# launches of one compute_chunk_regions, read at the parent of the commit that
# introduced the shared dispatch: it may not add one
LAUNCHES = {'MSE': {False: ['stream_partials'], True: ['stream_partials']},
            'CRPS': {False: ['ens_partials'], True: ['ens_partials']}}


@pytest.mark.parametrize('scoped', [False, True])
@pytest.mark.parametrize('name', ['MSE', 'CRPS'])
def test_launch_counts(gm, name, scoped):
  import contextlib
  from weatherbench2_amd import engine
  forecast, truth = det_case() if name == 'MSE' else ens_case(3)
  gf, gt, regions = g(forecast), g(truth), gregions()
  seen = []
  old = engine.set_launch_hook(lambda when, kernel: seen.append(kernel)
                               if when == 'begin' else None)
  try:
    with (gm.chunk_scope() if scoped else contextlib.nullcontext()):
      getattr(gm, name)().compute_chunk_regions(gf, gt, regions)
  finally:
    engine.set_launch_hook(old)
  print(f'LAUNCHES {name} scoped={scoped}: {sorted(seen)}')
  assert sorted(seen) == LAUNCHES[name][scoped], seen
