"""Window quantiles and SEEPS thresholds of the climatology module without a
GPU: the host path against the NumPy restatement, the reference's fixture
against the restatement (every value), independent pins of the weighted
quantile, and the public API."""
import numpy as np
import pytest

from tests import seeps_climatology_cases as sc
from tests import seeps_climatology_np as sn
from weatherbench2_amd import climatology as cl
from weatherbench2_amd import quantiles
from weatherbench2_amd import xarray_lite as xl

THR = sc.DRY_MM / 1000
CASES = sc.reference_cases()


@pytest.fixture(scope='module')
def golden():
  return sc.load_golden()


def dataset_of(case, data=None) -> xl.Dataset:
  return xl.Dataset(
      {sc.VAR: xl.DataArray(case['data'] if data is None else data,
                            case['dims'])}, coords={'time': case['times']})


def _kw(case):
  return dict(frequency=case['frequency'], window_size=case['window_size'],
              clim_years=case['clim_years'],
              hour_interval=case['hour_interval'])


_RESTATED = {}


def restate(name):
  """The restatement of a case, computed once: {'seeps', 'quantile'}, each the
  dict of `restate_hourly` with a leading hour axis."""
  if name not in _RESTATED:
    case = CASES[name]
    times, data = case['times'], case['data']
    hours = cl.hours_of(case['hour_interval']).tolist() \
        if case['frequency'] == 'hourly' else None
    if hours is None:  # daily means first: two steps a day
      assert case['hour_interval'] is None
      data = data.reshape(-1, 2, data.shape[1]).mean(axis=1)
      times = times[::2]
    w = case['window_size']
    _RESTATED[name] = {
        'seeps': sn.restate_hourly(times, data, hours, w, [2 / 3], THR),
        'quantile': sn.restate_hourly(times, data, hours, w,
                                      case['quantiles'])}
  return _RESTATED[name]


def _lead(values, case):
  """The public result with a leading hour axis, as the restatement has."""
  return values if case['frequency'] == 'hourly' else values[None]


# ---------------------------------------------------------------------------
# the host path against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_host_path_against_the_restatement(name):
  case = CASES[name]
  before = case['data'].copy()
  out = cl.compute_seeps_chunk(dataset_of(case),
                               seeps_threshold_mm={sc.VAR: sc.DRY_MM},
                               **_kw(case))
  r = restate(name)
  thr = _lead(out[sc.VAR + '_seeps_threshold'].values, case)
  dry = _lead(out[sc.VAR + '_seeps_dry_fraction'].values, case)
  assert thr.dtype == np.float64 and dry.dtype == np.float64
  assert np.array_equal(dry, r['seeps']['dry_fraction'])  # bit-equal
  sn.assert_within(thr, r['seeps']['quantile'][:, 0], sn.interval_bound(
      r['seeps']['k'][:, 0], r['seeps']['xmax'][:, 0]), name)
  quant = cl.compute_stat_chunk(dataset_of(case), statistic='quantile',
                                quantiles=case['quantiles'], **_kw(case))
  got = _lead(quant[sc.VAR + '_quantile'].values, case)
  sn.assert_within(got, r['quantile']['quantile'], sn.interval_bound(
      r['quantile']['k'], r['quantile']['xmax']), name + ' quantile')
  assert np.array_equal(before, case['data'], equal_nan=True)


# ---------------------------------------------------------------------------
# the reference's fixture against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_reference_fixture_against_the_restatement(golden, name):
  case = CASES[name]
  r = restate(name)
  hourly = case['frequency'] == 'hourly'
  lead = ('hour',) if hourly else ()
  assert golden[f'{name}/seeps_threshold/dims'].tolist() == list(
      lead + ('dayofyear', 'point'))
  assert golden[f'{name}/quantile/dims'].tolist() == list(
      lead + ('quantile', 'dayofyear', 'point'))
  for kind, key in (('seeps', 'seeps_threshold'), ('quantile', 'quantile')):
    want = r[kind]
    ref = _lead(golden[f'{name}/{key}'], case)
    if kind == 'seeps':
      ref = ref[:, None]
    assert ref.shape == want['quantile'].shape  # every value is compared
    bound = sn.reference_bound(want['n_sample'][:, None], want['n_eff'],
                               want['k'], want['xmax'], want['spread'])
    sn.assert_within(ref, want['quantile'], bound, f'{name} {key}')
  dry = _lead(golden[f'{name}/seeps_dry_fraction'], case)
  # the reference's mean of a bool array: count / size in float64
  assert np.array_equal(dry, r['seeps']['dry_fraction'])


# ---------------------------------------------------------------------------
# independent pins
# ---------------------------------------------------------------------------
def test_known_case(golden):
  data = sc.known_input()
  np.testing.assert_array_equal(golden['known/data'], data)
  np.testing.assert_allclose(golden['known/seeps_dry_fraction'], 1 / 5,
                             rtol=1e-12)
  np.testing.assert_allclose(golden['known/seeps_threshold'], 4 / 1000,
                             rtol=1e-12)
  name = 'total_precipitation_6hr'
  ds = xl.Dataset({name: xl.DataArray(data, ('dim_0',))})
  out = cl.SEEPSThreshold(0.25, name).compute(ds, dim=...)
  assert list(out.data_vars) == [name + '_seeps_threshold',
                                 name + '_seeps_dry_fraction']
  assert out[name + '_seeps_threshold'].dims == ()
  assert 'quantile' not in out.coords
  assert out[name + '_seeps_dry_fraction'].values == golden[
      'known/seeps_dry_fraction']
  assert out[name + '_seeps_threshold'].values == golden[
      'known/seeps_threshold']
  q = cl.Quantile([0.25, 0.5]).compute(ds, dim=...)
  np.testing.assert_array_equal(q[name].values, golden['known/quantile'])
  f32 = xl.Dataset({name: xl.DataArray(data.astype(np.float32), ('dim_0',))})
  out = cl.SEEPSThreshold(0.25, name).compute(f32, dim=('dim_0',))
  # (0.25 / 1000 rounded to float32 is not below itself: 1 / 5 again)
  assert out[name + '_seeps_dry_fraction'].values == 1 / 5
  with pytest.raises(NotImplementedError, match='rolling window'):
    cl.Quantile([0.5]).compute(ds, dim=..., weights=np.ones(5))


def test_equal_weights_are_numpys_linear_quantile():
  rng = np.random.default_rng(0)
  for n in (1, 2, 5, 37):
    x = rng.normal(size=n)
    for q in (0.0, 0.2, 0.5, 2 / 3, 1.0):
      want = np.quantile(x, q, method='linear')
      assert abs(sn.cumsum_form(x, np.full(n, 0.37), q) - want) <= 1e-12 * max(
          1.0, np.abs(x).max())
      got = sn.interval_form(x, np.full(n, 3), q)[0]
      assert abs(got - want) <= 1e-12 * max(1.0, np.abs(x).max())


def test_window_of_three_is_the_quantile_over_the_years():
  case = sc.hourly(np.float64, n_point=4, window_size=3, hour_interval=24)
  ds = dataset_of(case)
  out = cl.compute_hourly_stat(ds, 3, slice(None, None), 24,
                               cl.Quantile([0.25, 2 / 3]).compute)
  table, axis = sn.year_tables(case['times'], case['data'])
  years = xl.DataArray(table, ('year', 'dayofyear', 'point'))
  want = quantiles.quantile(years, [0.25, 2 / 3], 'year', skipna=True)
  assert out[sc.VAR].dims == ('hour', 'quantile', 'dayofyear', 'point')
  assert out.coords['dayofyear'].tolist() == axis.tolist()
  np.testing.assert_allclose(out[sc.VAR].values[0], want.values, rtol=1e-13,
                             atol=0)


def test_cumsum_form_is_the_interval_form_with_ties():
  rng = np.random.default_rng(5)
  for trial in range(200):
    n = int(rng.integers(1, 40))
    x = np.round(rng.gamma(1.0, 2.0, size=n) * 2) / 2  # ties
    m = rng.integers(1, 9, size=n)
    q = float(rng.choice([0.0, 1.0, 2 / 3, rng.uniform()]))
    got, k, xmax, spread, n_eff = sn.interval_form(x, m, q)
    want = sn.cumsum_form(x, m / m.mean(), q)
    bound = 8.0 * n_eff * sn.U * (n * spread + (k + 2) * xmax)
    assert abs(got - want) <= bound, (trial, got, want, bound)


# ---------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------
def _two_variables():
  rng = np.random.default_rng(8)
  times = sc.times_of('2019-01-01', '2021-12-31', 12)
  dims = ('time', 'latitude', 'longitude')
  coords = {'time': times, 'latitude': np.array([-10.0, 10.0]),
            'longitude': np.array([0.0, 120.0, 240.0])}
  shape = (times.size, 2, 3)
  return xl.Dataset({
      sc.VAR: xl.DataArray(sc.precipitation(rng, shape), dims),
      't': xl.DataArray(rng.normal(size=shape), dims),
      'static': xl.DataArray(np.zeros((2, 3)), dims[1:])}, coords)


def test_compute_climatology_names_dims_and_order():
  ds = _two_variables()
  kw = dict(frequency='hourly', hour_interval=12, window_size=5,
            start_year=2019, end_year=2021)
  out = cl.compute_climatology(
      ds, statistics=['std', 'seeps', 'quantile', 'mean'],
      seeps_dry_threshold_mm={sc.VAR: sc.DRY_MM, 'absent': 1.0},
      quantiles=[0.1, 0.9], **kw)
  assert list(out.data_vars) == [
      sc.VAR + '_std', 't_std', sc.VAR + '_seeps_threshold',
      sc.VAR + '_seeps_dry_fraction', sc.VAR + '_quantile', 't_quantile',
      sc.VAR, 't']
  plain = ('hour', 'dayofyear', 'latitude', 'longitude')
  assert out[sc.VAR + '_seeps_threshold'].dims == plain
  assert out[sc.VAR + '_seeps_dry_fraction'].dims == plain
  assert out['t_quantile'].dims == ('hour', 'quantile') + plain[1:]
  assert out['t_quantile'].values.shape == (2, 2, 366, 2, 3)
  assert out.coords['quantile'].tolist() == [0.1, 0.9]
  assert out.coords['hour'].tolist() == [0, 12]
  alone = cl.compute_climatology(ds, statistics='mean', **kw)
  np.testing.assert_array_equal(out['t'].values, alone['t'].values)
  daily = cl.compute_climatology(
      ds, statistics=['seeps'], seeps_dry_threshold_mm={sc.VAR: sc.DRY_MM},
      frequency='daily', window_size=5, start_year=2019, end_year=2021)
  assert list(daily.data_vars) == [sc.VAR + '_seeps_threshold',
                                   sc.VAR + '_seeps_dry_fraction']
  assert daily[sc.VAR + '_seeps_threshold'].dims == plain[1:]


def test_errors_and_refusals():
  case = CASES['hourly12']
  ds = dataset_of(case)
  kw = dict(window_size=3, clim_years=slice(None, None))
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_daily_stat(ds, stat_fn=lambda *a, **k: None, **kw)
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_daily_stat(ds, stat_fn=np.mean, **kw)
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_stat_chunk(ds, frequency='daily', statistic='quantile', **kw)
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_climatology(ds, statistics=['quantile'])
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_climatology(ds, statistics=['seeps'], quantiles=[0.5])
  with pytest.raises(NotImplementedError, match='explicit'):
    cl.compute_stat_chunk(ds, frequency='hourly', statistic='quantile',
                          quantiles=[0.5], hour_interval=12, method='fast',
                          **kw)
  with pytest.raises(NotImplementedError, match='SEEPS only tested for'):
    cl.compute_seeps_chunk(ds, frequency='hourly', hour_interval=12,
                           seeps_threshold_mm={sc.VAR: 0.25}, method='fast',
                           **kw)
  with pytest.raises(NotImplementedError, match='Frequency weekly'):
    cl.compute_seeps_chunk(ds, frequency='weekly', hour_interval=12,
                           seeps_threshold_mm={sc.VAR: 0.25}, **kw)
  with pytest.raises(KeyError):
    cl.compute_seeps_chunk(ds, frequency='hourly', hour_interval=12,
                           seeps_threshold_mm={'other': 0.25}, **kw)
  two = _two_variables()
  with pytest.raises(ValueError):
    cl.compute_seeps_chunk(two, frequency='hourly', hour_interval=12,
                           seeps_threshold_mm={sc.VAR: 0.25}, **kw)
  stat = cl.SEEPSThreshold(0.25, sc.VAR).compute
  series = dataset_of(sc.hourly(hour_interval=24, n_point=2))
  good = cl.create_window_weights(5)
  cl.compute_rolling_stat(series, good, stat)
  cl.compute_rolling_stat(series, good.values * 7.5, stat)  # any scale
  with pytest.raises(ValueError, match='create_window_weights'):
    cl.compute_rolling_stat(series, np.ones(5), stat)
  with pytest.raises(ValueError, match='create_window_weights'):
    cl.compute_rolling_stat(series, good.values * (1 + 1e-9 * np.arange(5)),
                            stat)
  with pytest.raises(ValueError, match='NaN'):
    cl.compute_rolling_stat(series, cl.create_window_weights(1), stat)
  with pytest.raises(ValueError, match='NaN'):
    cl.compute_daily_stat(series, 1, slice(None, None), stat)
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    cl.compute_rolling_stat(series, good, cl.Quantile([1.5]).compute)
  with pytest.raises(ValueError, match='Dataset'):
    cl.compute_rolling_stat(series[sc.VAR], good, stat)
  # an unbound `compute` is any other callable
  with pytest.raises(NotImplementedError, match='quantile and SEEPS'):
    cl.compute_rolling_stat(series, good, cl.Quantile.compute)


def test_rolling_stat_on_a_dataarray_and_integer_input():
  case = sc.hourly(np.float64, n_point=2, hour_interval=24)
  series = dataset_of(case)
  w = cl.create_window_weights(5)
  da = cl.compute_rolling_stat(series[sc.VAR], w, cl.Quantile(0.5).compute)
  assert da.dims == ('dayofyear', 'point')
  assert float(da.coords['quantile'].values) == 0.5
  both = cl.compute_rolling_stat(series, w, cl.Quantile([0.5]).compute)
  np.testing.assert_array_equal(both[sc.VAR].values[0], da.values)
  ints = np.round(case['data'] * 1e4).astype(np.int32)
  a = cl.compute_rolling_stat(dataset_of(case, ints), w,
                              cl.Quantile([0.3]).compute)
  b = cl.compute_rolling_stat(dataset_of(case, ints.astype(np.float64)), w,
                              cl.Quantile([0.3]).compute)
  assert a[sc.VAR].values.dtype == np.float64
  np.testing.assert_array_equal(a[sc.VAR].values, b[sc.VAR].values)


# ---------------------------------------------------------------------------
# the C ABI without a GPU: everything is checked before anything is enqueued
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_entry_point_validates_its_arguments(lib):
  import ctypes
  h = lib.load()
  buf = ctypes.create_string_buffer(256)
  ptr = ctypes.addressof(buf)
  Begin = ctypes.c_int32 * 3
  weights = lambda *m: (ctypes.c_int32 * len(m))(*m)
  qs = lambda *q: (ctypes.c_double * len(q))(*q)

  def call(dtype=lib.WB2_F32, inp=ptr, n_outer=1, n_time=4, n_point=4,
           begin=ptr, host=Begin(0, 2, 4), n_cycle=1, n_pos=2, member=ptr,
           n_member=4, m=weights(0, 1, 0), n_w=3, use_dry=1, den=6,
           q=qs(0.5), n_q=1, quant=ptr, dry=ptr):
    return h.wb2_window_quantile(
        dtype, inp, None, n_outer, n_time, n_point, begin, host, n_cycle,
        n_pos, member, None, n_member, m, n_w, use_dry, 0.00025, den, q, n_q,
        quant, dry, None)

  assert call(dtype=7) < 0 and b'unknown dtype' in h.wb2_last_error()
  for null in ('inp', 'begin', 'host', 'member', 'm', 'q', 'quant'):
    assert call(**{null: None}) < 0, null
    assert b'null pointer' in h.wb2_last_error()
  for bad in (Begin(1, 2, 4), Begin(0, 2, 3), Begin(0, 5, 4), Begin(0, -1, 4)):
    assert call(host=bad) < 0
    assert b'does not fit the members' in h.wb2_last_error()
  for n_w in (0, 2, -1, 513):
    assert call(n_w=n_w) < 0 and b'odd, positive' in h.wb2_last_error()
  assert call(m=weights(0, -1, 0)) < 0 and b'negative' in h.wb2_last_error()
  assert call(m=weights(2**30, 2**30, 2**30)) < 0
  assert b'integer counters' in h.wb2_last_error()
  # the sum of squares alone: 2 members x 40000^2 > 2^31 - 1
  assert call(m=weights(0, 40000, 0)) < 0
  assert b'integer counters' in h.wb2_last_error()
  for bad in (-0.1, 1.5, float('nan')):
    assert call(q=qs(bad)) < 0 and b'not in [0, 1]' in h.wb2_last_error()
  assert call(den=0) < 0 and b'denominator' in h.wb2_last_error()
  assert call(use_dry=0) < 0 and b'denominator' in h.wb2_last_error()
  for count in ('n_outer', 'n_cycle', 'n_pos', 'n_point', 'n_q'):
    assert call(**{count: 0}) == 0  # nothing to do, whatever the pointers
    assert call(**{count: 0, 'inp': None, 'quant': None, 'host': None}) == 0
    assert call(**{count: -1}) < 0 and b'negative' in h.wb2_last_error()
  for count in ('n_time', 'n_member'):
    assert call(**{count: -1}) < 0 and b'negative' in h.wb2_last_error()
  # a window that fits no tile: 511 weights x 50 members
  big = (ctypes.c_int32 * 101)(*range(0, 5001, 50))
  wide = weights(*([1] * 511))
  assert call(host=big, n_pos=100, n_member=5000, m=wide, n_w=511) < 0
  assert b'does not fit the LDS' in h.wb2_last_error()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_geometry_is_sane(lib, dtype):
  import torch
  from weatherbench2_amd import engine
  size = np.dtype(dtype).itemsize
  for n_year, n_w in ((1, 3), (3, 5), (31, 61), (7, 61), (100, 61), (300, 5)):
    geo = engine.window_quantile_geometry(getattr(torch, dtype), n_year, n_w)
    tile, d = geo['tile_points'], geo['positions']
    assert tile in (1, 2, 4, 8, 16) and tile * size <= 64
    assert 1 <= d <= 32 and (d >= 4 or tile == 1)
    assert geo['lds_bytes'] == ((d + n_w - 1) * n_year * tile * size
                                + 4 * n_w * n_year) <= 160 * 1024
    assert geo['key_bits_per_pass'] == 2
  with pytest.raises(lib.Wb2HipError, match='does not fit'):
    engine.window_quantile_geometry(getattr(torch, dtype), 400, 61)
  with pytest.raises(lib.Wb2HipError, match='odd'):
    engine.window_quantile_geometry(getattr(torch, dtype), 3, 4)
