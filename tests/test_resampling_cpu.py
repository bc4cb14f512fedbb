"""Resampling in time without a GPU: the NumPy restatement
(tests/resample_np.py) against the committed reference fixtures, the
reference's own known answers and pandas; the host path of
`resampling.resample_in_time` / `resample_in_time_core` against the
restatement bit for bit; names, order and errors; and the argument checks of
the two K13 entry points.  Reference: scripts/resample_in_time.py:187-352."""
import ctypes
import datetime
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import resample_cases as rc
from tests import resample_np as rn
from weatherbench2_amd import resampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, 'weatherbench2'))
CASES = sorted(rc.all_cases())
MODES = sorted(rc.MODES)


@pytest.fixture(scope='module')
def golden():
  out = rc.load_golden(GOLDEN_DIR)
  assert out, 'no reference_resample_v1.*.npz shard found'
  return out


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def to_lite(case, device=False):
  from weatherbench2_amd import xarray_lite as xl
  variables = {}
  for name, (dims, array) in case['vars'].items():
    data = array
    if device:
      import torch
      data = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    variables[name] = xl.DataArray(data, dims)
  return xl.Dataset(variables, dict(case['coords']))


def run_product(case, dataset, skipna):
  stats = case['stats']
  return resampling.resample_in_time(
      dataset, method=case['method'], period=case['period'],
      mean_vars=stats['mean'], min_vars=stats['min'], max_vars=stats['max'],
      sum_vars=stats['sum'], add_mean_suffix=case['add_mean_suffix'],
      skipna=skipna, time_dim=case['time_dim'], label_side=case['label_side'])


def check_against_fixture(values: dict, case, cname, mode, golden):
  """{output name: (dims, array)} within the bounds of the fixture of (case,
  mode): another ordering of the same terms."""
  _, ranges = rn.plan(case)
  skipna = rc.MODES[mode] and case['method'] != 'rolling'
  for new, name, stat in rn.output_names(case):
    dims, array = case['vars'][name]
    axis = dims.index(case['time_dim'])
    assert list(golden[f'{cname}/{mode}/{new}/dims']) == list(dims)
    abs_sum, lengths = rn.abs_sums(array, axis, ranges)
    counts = rn.valid_counts(array, axis, ranges) if skipna else None
    rn.assert_within_bound(values[new][1], golden[f'{cname}/{mode}/{new}'],
                           stat, abs_sum, lengths, axis, skipna, counts,
                           what=f'{cname}/{mode}/{new}')


def check_product(res, case, cname, mode, golden, device=False):
  """A product result: bit-equal to the restatement, within the bound of the
  fixture, names in the reference's order, labels, dims and coordinates."""
  from weatherbench2_amd import xarray_lite as xl
  assert isinstance(res, xl.Dataset)
  want = rn.resample(case, rc.MODES[mode])
  assert list(res.data_vars) == list(want)
  assert list(res.data_vars) == [
      k for k in (key[len(f'{cname}/{mode}/'):] for key in golden
                  if key.startswith(f'{cname}/{mode}/'))
      if '/' not in k and k not in ('coords', 'labels')]
  labels = np.asarray(res.coords[case['time_dim']])
  assert labels.dtype == rn.shifted_labels(case).dtype
  np.testing.assert_array_equal(labels, rn.shifted_labels(case))
  assert sorted(res.coords) == sorted(golden[f'{cname}/{mode}/coords'])
  values = {}
  for new, (dims, array) in want.items():
    da = res[new]
    assert da.dims == tuple(dims), new
    if device:
      import torch
      assert isinstance(da.data, torch.Tensor) and da.data.is_cuda, new
    else:
      assert isinstance(da.data, np.ndarray), new
    rn.assert_same(da.values, array, f'{cname}/{mode}/{new}')
    values[new] = (dims, da.values)
  check_against_fixture(values, case, cname, mode, golden)
  for k, c in case['coords'].items():
    if k != case['time_dim'] and k in res.coords:
      np.testing.assert_array_equal(np.asarray(res.coords[k]), c)


# ---------------------------------------------------------------------------
# fixtures and restatement
# ---------------------------------------------------------------------------
def test_one_shard_per_case_below_the_size_limit():
  paths = rc.golden_paths(GOLDEN_DIR)
  assert len(paths) == len(rc.cases()) + 1  # + the known-answer cases
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path


@pytest.mark.skipif(not HAVE_REFERENCE,
                    reason='the reference checkout is only present in the '
                           'build container')
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
  env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1',
             WB2_RESAMPLE_OUT=str(tmp_path))
  done = subprocess.run(
      [sys.executable, os.path.join(GOLDEN_DIR, 'make_resample_vectors.py')],
      env=env, capture_output=True, text=True)
  assert done.returncode == 0, done.stderr[-2000:]
  fresh = rc.load_golden(str(tmp_path))
  assert sorted(fresh) == sorted(golden)
  for key, want in golden.items():
    got = fresh[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    np.testing.assert_array_equal(got, want, err_msg=key)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_restatement_against_the_fixture(golden, cname, mode):
  """Labels, min and max exactly; sum within 2 n u sum|x| of the fixture, mean
  within that over the count plus u |mean|; NaN and inf in the same places."""
  case = rc.all_cases()[cname]()
  labels, ranges = rn.plan(case)
  want_labels = golden[f'{cname}/{mode}/labels']
  assert labels.dtype == want_labels.dtype
  np.testing.assert_array_equal(labels, want_labels)
  check_against_fixture(rn.resample(case, rc.MODES[mode]), case, cname, mode,
                        golden)


def test_the_cases_cover_what_they_claim():
  built = {k: b() for k, b in rc.cases().items()}
  lengths = {k: [e - b for b, e in rn.plan(c)[1]] for k, c in built.items()}
  assert lengths['first_f32'][0] == 3 and lengths['first_f32'][-1] == 2
  assert lengths['single_bin'] == [5]
  assert set(lengths['length_one']) == {1}
  assert lengths['gap_left'].count(0) == 2
  assert lengths['gap_right'].count(0) == 2
  assert set(lengths['weekly'][:2]) == {28}
  assert {c['period'] for c in built.values()} >= {'6h', '1d', '3d', '1w',
                                                  '30h'}
  assert {c['label_side'] for c in built.values()} == {'left', 'right'}
  windows = {k: lengths[k][-1] for k in built if k.startswith('rolling')}
  assert sorted(windows.values()) == [1, 4, 7, 12]
  axes = {c['vars'][next(iter(c['vars']))][0].index(c['time_dim'])
          for c in built.values()}
  assert axes >= {0, 1, 2}
  x = built['nan_f32']['vars']['field'][1]
  assert np.isnan(x[4:8, 11]).all()  # an all-NaN bin
  assert np.isinf(x[4:8, 13]).sum() == 2  # +inf and -inf in one bin


# ---------------------------------------------------------------------------
# the reference's own known answers (resample_in_time_test.py:30-189)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('insert_nan', [False, True])
def test_known_ten_days(insert_nan):
  case = rc.known_ten_days(insert_nan, 'resample')
  temperatures = case['vars']['temperature'][1]
  res = run_product(case, to_lite(case), False)
  np.testing.assert_array_equal(
      np.asarray(res.coords['time']),
      np.array(['2023-01-01', '2023-01-04', '2023-01-07', '2023-01-10'],
               dtype='datetime64[ns]'))
  np.testing.assert_array_equal(
      res['temperature'].values,
      [np.mean(temperatures[:3]), np.mean(temperatures[3:6]),
       np.mean(temperatures[6:9]), np.mean(temperatures[9:12])])
  assert np.isnan(res['temperature'].values[0]) == insert_nan
  rolling = run_product(rc.known_ten_days(insert_nan, 'rolling'),
                        to_lite(case), False)
  common = np.array(['2023-01-01', '2023-01-04', '2023-01-07'],
                    dtype='datetime64[ns]')
  at = np.isin(np.asarray(rolling.coords['time']), common)
  assert at.sum() == 3
  np.testing.assert_array_equal(rolling['temperature'].values[at],
                                res['temperature'].values[:3])


@pytest.mark.parametrize('k', range(len(rc.KNOWN_COMBINATIONS)))
def test_known_combinations_resample_and_rolling_agree(k):
  a = run_product(rc.known_combination(k, 'resample'),
                  to_lite(rc.known_combination(k, 'resample')), False)
  b = run_product(rc.known_combination(k, 'rolling'),
                  to_lite(rc.known_combination(k, 'rolling')), False)
  ta, tb = np.asarray(a.coords['time']), np.asarray(b.coords['time'])
  common = np.intersect1d(ta, tb)
  assert len(common) >= len(ta) - 1
  np.testing.assert_array_equal(a['temperature'].values[np.isin(ta, common)],
                                b['temperature'].values[np.isin(tb, common)])


# ---------------------------------------------------------------------------
# pandas
# ---------------------------------------------------------------------------
def _random_axis(rng, kind):
  start_h, step, n = rng.randint(0, 48), rng.randint(1, 25), rng.randint(1, 60)
  idx = np.arange(n)
  if rng.rand() < 0.5 and n > 4:
    idx = np.delete(idx, rng.choice(n, rng.randint(1, n // 2), replace=False))
  hours = (start_h + step * idx).astype('timedelta64[h]')
  return np.datetime64('2020-01-01') + hours if kind == 'M' else hours


def test_bin_planner_matches_pandas():
  pd = pytest.importorskip('pandas')
  rng = np.random.RandomState(20241)
  periods = ['1h', '6h', '7h', '1d', '30h', '3d', '1w']
  for it in range(200):
    kind = 'M' if it % 4 else 'm'
    times = _random_axis(rng, kind)
    period = periods[rng.randint(len(periods))]
    for side in ('left', 'right'):
      series = pd.Series(np.ones(len(times)), index=pd.Index(times))
      want = series.resample(pd.to_timedelta(period), label=side,
                             closed=side).count()
      if side == 'right':
        want = want.iloc[1:]
      labels, ranges = resampling.plan_resample(times, period, side)
      what = (it, kind, period, side)
      assert ranges.dtype == np.int32 and ranges.shape == (len(labels), 2)
      np.testing.assert_array_equal(
          labels, want.index.values.astype(labels.dtype), err_msg=str(what))
      np.testing.assert_array_equal(ranges[:, 1] - ranges[:, 0], want.values,
                                    err_msg=str(what))
      mine, mine_ranges = rn.resample_bins(times, rn.period_ns(period), side)
      np.testing.assert_array_equal(mine, labels, err_msg=str(what))
      assert [tuple(r) for r in ranges.tolist() if r[0] != r[1]] == [
          r for r in mine_ranges if r[0] != r[1]], what


def test_float64_values_match_pandas():
  pd = pytest.importorskip('pandas')
  from weatherbench2_amd import xarray_lite as xl
  rng = np.random.RandomState(20242)
  u = np.finfo(np.float64).eps / 2
  for it in range(20):
    times = _random_axis(rng, 'M')
    x = rng.standard_normal(len(times)) * 10
    x[rng.rand(len(times)) < 0.15] = np.nan
    period = ['6h', '1d', '30h', '3d'][it % 4]
    series = pd.Series(x, index=pd.Index(times))
    grouped = series.resample(pd.to_timedelta(period))
    total = series.abs().resample(pd.to_timedelta(period)).sum().values
    count = grouped.count().values
    ds = xl.Dataset({'x': xl.DataArray(x, ('time',))}, {'time': times})
    res = resampling.resample_in_time(
        ds, method='resample', period=period, mean_vars=['x'], min_vars=['x'],
        max_vars=['x'], skipna=True)
    n = np.array([e - b for b, e in resampling.plan_resample(
        times, period)[1].tolist()])
    for name, want in (('x', grouped.mean().values),
                       ('x_min', grouped.min().values),
                       ('x_max', grouped.max().values)):
      got = res[name].values
      assert np.array_equal(np.isnan(got), np.isnan(want)), (it, name)
      ok = ~np.isnan(got)
      if name != 'x':
        np.testing.assert_array_equal(got[ok], want[ok])
        continue
      bound = 2 * n * u * total / np.maximum(count, 1) + u * np.abs(want)
      assert np.all(np.abs(got - want)[ok] <= bound[ok]), (it, name)
  for w in (1, 4, 7):
    times = rc.time_axis('2020-01-01T00', 6, 30)
    x = rng.standard_normal(30) * 10
    x[11] = np.nan
    series = pd.Series(x, index=pd.Index(times))
    total = series.abs().fillna(0).rolling(w).sum().values
    ds = xl.Dataset({'x': xl.DataArray(x, ('time',))}, {'time': times})
    res = resampling.resample_in_time(
        ds, method='rolling', period=f'{6 * w}h', mean_vars=['x'],
        min_vars=['x'], max_vars=['x'], sum_vars=['x'], skipna=bool(w % 2))
    for name, want in (('x', series.rolling(w).mean().values),
                       ('x_min', series.rolling(w).min().values),
                       ('x_max', series.rolling(w).max().values),
                       ('x_sum', series.rolling(w).sum().values)):
      got = res[name].values
      assert np.array_equal(np.isnan(got), np.isnan(want)), (w, name)
      ok = ~np.isnan(got)
      bound = 2 * w * u * total
      if name == 'x':
        bound = bound / w + u * np.abs(want)
      if name in ('x_min', 'x_max'):
        np.testing.assert_array_equal(got[ok], want[ok])
      else:
        assert np.all(np.abs(got - want)[ok] <= bound[ok]), (w, name)


# ---------------------------------------------------------------------------
# the host path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_host_path_equals_the_restatement(golden, cname, mode):
  case = rc.all_cases()[cname]()
  before = {k: a.copy() for k, (_, a) in case['vars'].items()}
  res = run_product(case, to_lite(case), rc.MODES[mode])
  check_product(res, case, cname, mode, golden)
  for k, (_, a) in case['vars'].items():
    assert a.dtype == before[k].dtype
    np.testing.assert_array_equal(a, before[k])


def test_host_sum_goes_in_time_order_where_time_is_innermost():
  """Along a contiguous axis NumPy's own sum is pairwise: the host path is
  sequential like the kernel."""
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(5)
  x = (rs.standard_normal((3, 64)) * 1e3).astype(np.float32)
  times = rc.time_axis('2020-01-01T00', 1, 64)
  ds = xl.Dataset({'x': xl.DataArray(x, ('point', 'time'))}, {'time': times})
  res = resampling.resample_in_time(ds, method='resample', period='1w',
                                    sum_vars=['x'])
  want = x[:, 0].copy()
  for t in range(1, 64):
    want = want + x[:, t]
  np.testing.assert_array_equal(res['x_sum'].values[:, 0], want)
  assert not np.array_equal(want, x.sum(axis=1))  # (the case can tell)


@pytest.mark.parametrize('mode', MODES)
def test_core_gives_one_statistic_and_passes_the_rest_through(golden, mode):
  from weatherbench2_amd import xarray_lite as xl
  cname = 'first_f32'
  case = rc.all_cases()[cname]()
  ds = to_lite(case)
  _, ranges = rn.plan(case)
  for stat in rc.STATS:
    res = resampling.resample_in_time_core(ds, case['method'], case['period'],
                                           stat, rc.MODES[mode])
    assert list(res.data_vars) == list(case['vars'])
    np.testing.assert_array_equal(np.asarray(res.coords['time']),
                                  golden[f'{cname}/{mode}/labels'])
    for name, (dims, array) in case['vars'].items():
      if 'time' not in dims:
        assert res[name].data is ds[name].data
        continue
      want = rn.bin_stats(array, 0, ranges, rc.MODES[mode])[stat]
      rn.assert_same(res[name].values, want, f'{stat}/{name}')
    one = resampling.resample_in_time_core(ds['temperature'], case['method'],
                                           case['period'], stat,
                                           rc.MODES[mode])
    assert isinstance(one, xl.DataArray) and one.name == 'temperature'
    rn.assert_same(one.values, res['temperature'].values)
  # rolling through the core keeps the time axis (no label shift)
  case = rc.all_cases()['rolling_4']()
  res = resampling.resample_in_time_core(to_lite(case), 'rolling', '1d', 'max',
                                         rc.MODES[mode], label_side='right')
  np.testing.assert_array_equal(np.asarray(res.coords['time']),
                                case['coords']['time'])


# ---------------------------------------------------------------------------
# names and errors
# ---------------------------------------------------------------------------
def test_names_order_and_the_all_sentinel():
  case = rc.all_cases()['first_f32']()
  ds = to_lite(case)
  kw = dict(method='resample', period='1d')
  res = resampling.resample_in_time(ds, mean_vars=['ALL'], **kw)
  assert list(res.data_vars) == ['temperature', 'counts']
  res = resampling.resample_in_time(ds, mean_vars='ALL', max_vars=['ALL'],
                                    add_mean_suffix=True, **kw)
  assert list(res.data_vars) == ['temperature_mean', 'temperature_max',
                                 'counts_mean', 'counts_max']
  res = resampling.resample_in_time(
      ds, sum_vars=['temperature'], min_vars=['counts', 'temperature'],
      mean_vars=['counts'], max_vars=['counts'], **kw)
  assert list(res.data_vars) == ['temperature_min', 'temperature_sum',
                                 'counts', 'counts_min', 'counts_max']
  assert res['counts_min'].dtype == np.float64  # integers become float64
  assert res['temperature_min'].dtype == np.float32
  assert 'orography' not in res.data_vars
  assert sorted(res.coords) == ['latitude', 'longitude', 'time']
  assert len(resampling.resample_in_time(ds, **kw).data_vars) == 0


def test_period_forms():
  day = 86400 * 10**9
  assert resampling.parse_period('1d') == day
  assert resampling.parse_period('1w') == 7 * day
  assert resampling.parse_period('30h') == 30 * 3600 * 10**9
  assert resampling.parse_period('90min') == 90 * 60 * 10**9
  assert resampling.parse_period('45s') == 45 * 10**9
  assert resampling.parse_period(np.timedelta64(6, 'h')) == day // 4
  assert resampling.parse_period(datetime.timedelta(days=3)) == 3 * day
  for bad in ('1M', 'd', '1.5d', '-1d', '', 'one day', 3, 6.0, None,
              np.timedelta64('NaT'), '0h', datetime.timedelta(0)):
    with pytest.raises(ValueError):
      resampling.parse_period(bad)


def test_every_value_error():
  from weatherbench2_amd import xarray_lite as xl
  case = rc.all_cases()['first_f32']()
  ds = to_lite(case)
  kw = dict(method='resample', period='1d')
  with pytest.raises(ValueError, match='Unhandled method'):
    resampling.resample_in_time_core(ds, 'nearest', '1d', 'mean', False)
  with pytest.raises(ValueError, match='Unhandled method'):
    resampling.resample_in_time(ds, method='nearest', period='1d')
  with pytest.raises(ValueError, match='Unhandled label_side'):
    resampling.resample_in_time_core(ds, 'resample', '1d', 'mean', False,
                                     label_side='middle')
  with pytest.raises(ValueError, match='Unhandled label_side'):
    resampling.resample_in_time(ds, label_side='middle', **kw)
  with pytest.raises(ValueError, match='Unhandled statistic'):
    resampling.resample_in_time_core(ds, 'resample', '1d', 'median', False)
  with pytest.raises(ValueError, match='did not evenly divide'):
    resampling.resample_in_time_core(ds, 'rolling', '7h', 'mean', False)
  with pytest.raises(ValueError,
                     match='Cannot specify both ALL and other variables'):
    resampling.resample_in_time(ds, mean_vars=['ALL', 'temperature'], **kw)
  with pytest.raises(ValueError, match='did not contain time'):
    resampling.resample_in_time(ds, max_vars=['orography'], **kw)
  with pytest.raises(ValueError, match='not in the chunk'):
    resampling.resample_in_time(ds, max_vars=['nowhere'], **kw)
  with pytest.raises(ValueError, match='is not <int><unit>'):
    resampling.resample_in_time(ds, method='resample', period='1M')
  x = np.zeros(4)
  for times, text in (
      (np.array(['2020-01-02', '2020-01-01', '2020-01-03', '2020-01-04'],
                dtype='datetime64[ns]'), 'must increase'),
      (np.array(['2020-01-01', '2020-01-01', '2020-01-03', '2020-01-04'],
                dtype='datetime64[ns]'), 'must increase'),
      (np.arange(4), 'datetime64 or timedelta64')):
    bad = xl.Dataset({'x': xl.DataArray(x, ('time',))}, {'time': times})
    with pytest.raises(ValueError, match=text):
      resampling.resample_in_time(bad, mean_vars=['x'], **kw)
  uneven = xl.Dataset({'x': xl.DataArray(x, ('time',))}, {'time': np.array(
      ['2020-01-01', '2020-01-02', '2020-01-04', '2020-01-05'],
      dtype='datetime64[ns]')})
  with pytest.raises(ValueError, match='constant spacing'):
    resampling.resample_in_time(uneven, method='rolling', period='2d',
                                mean_vars=['x'])
  with pytest.raises(ValueError, match='no coordinate'):
    resampling.resample_in_time(
        xl.Dataset({'x': xl.DataArray(x, ('time',))}), mean_vars=['x'], **kw)


# ---------------------------------------------------------------------------
# the C ABI without a GPU
# ---------------------------------------------------------------------------
def test_entry_points_validate_their_arguments(lib):
  h = lib.load()
  buf = ctypes.create_string_buffer(256)
  ptr = ctypes.addressof(buf)
  outs = (ctypes.c_void_p * 4)(ptr, ptr, ptr, ptr)

  def stats(mask=15, dtype=lib.WB2_F32, inp=ptr, n_outer=1, n_time=4,
            n_point=4, ranges=ptr, n_bin=2, group=1, out=outs):
    return h.wb2_time_bin_stats(mask, dtype, 0, inp, None, n_outer, n_time,
                                n_point, ranges, n_bin, group, out, None)

  assert stats(dtype=7) < 0 and b'unknown dtype' in h.wb2_last_error()
  for mask in (0, 16, -1):
    assert stats(mask=mask) < 0 and b'statistic mask' in h.wb2_last_error()
  for group in (0, -3):
    assert stats(group=group) < 0 and b'bins per group' in h.wb2_last_error()
  for null in ('inp', 'ranges', 'out'):
    assert stats(**{null: None}) < 0
    assert b'null pointer' in h.wb2_last_error()
  for s in range(4):
    some = (ctypes.c_void_p * 4)(*[None if k == s else ptr for k in range(4)])
    assert stats(mask=1 << s, out=some) < 0
    assert b'has no output' in h.wb2_last_error()
    assert stats(mask=15, out=some) < 0
  for count in ('n_outer', 'n_time', 'n_point', 'n_bin'):
    assert stats(**{count: 0}) == 0  # nothing to do, whatever the pointers
    assert stats(**{count: 0, 'inp': None, 'out': None}) == 0
    assert stats(**{count: -1}) < 0 and b'negative' in h.wb2_last_error()
  vals = [ctypes.c_int32() for _ in range(3)]
  refs = [ctypes.byref(v) for v in vals]
  assert h.wb2_time_window_geometry(9, 0, *refs) < 0
  assert b'unknown dtype' in h.wb2_last_error()
  assert h.wb2_time_window_geometry(lib.WB2_F32, 0, None, *refs[1:]) < 0
  assert b'null pointer' in h.wb2_last_error()


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_geometry_is_sane(lib, dtype, wide):
  import torch
  from weatherbench2_amd import engine
  geo = engine.time_window_geometry(getattr(torch, dtype), wide)
  vec = 16 // np.dtype(dtype).itemsize if wide else 1
  assert geo['tile_points'] % vec == 0
  assert geo['tile_points'] // vec in (64, 128, 256, 512, 1024)
  assert 2 <= geo['steps_ahead'] <= 16
  assert 1 <= geo['max_grid_outer'] <= 65535
