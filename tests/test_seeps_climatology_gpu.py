"""Window quantiles and SEEPS thresholds on the GPU (K15) against the NumPy
restatement, under the bounds derived in tests/seeps_climatology_np.py: the
dry fraction bit for bit, two runs bit-equal, across point tiles, position
blocks, LDS regimes, window shapes, input layouts and edge data; then the
hand-over to metrics.SEEPS."""
import numpy as np
import pytest

from tests import seeps_climatology_cases as sc
from tests import seeps_climatology_np as sn

pytestmark = pytest.mark.gpu

THR = sc.DRY_MM / 1000


@pytest.fixture(scope='module')
def torch():
  import torch as module
  return module


def _dev(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_launch(torch, x, begin, member, fill, n_cycle, n_pos, window, qs,
                  thr=None, n_year=None, x_dev=None, slab=None, what=''):
  """One K15 launch against the restatement on x [n_outer, n_time, n_point]
  (the series as the slab table presents them)."""
  from weatherbench2_amd import engine
  n_outer, n_time, n_point = x.shape
  x_dev = _dev(torch, x) if x_dev is None else x_dev
  args = (x_dev, None if slab is None else _dev(torch, slab), n_outer, n_time,
          n_point, begin, n_cycle, n_pos, _dev(torch, member),
          None if fill is None else _dev(torch, fill),
          sn.window_weights(window), qs, thr,
          None if thr is None else window * n_year)
  quant, dry = engine.window_quantile(*args)
  again_q, again_d = engine.window_quantile(*args)
  assert torch.equal(quant.view(torch.int64), again_q.view(torch.int64)), what
  want = sn.launch(x, begin, member, fill, n_cycle, n_pos, window, qs, thr,
                   n_year)
  sn.assert_within(quant.cpu().numpy(), want['quantile'],
                   sn.interval_bound(want['k'], want['xmax']), what)
  if thr is None:
    assert dry is None
  else:
    assert torch.equal(dry.view(torch.int64), again_d.view(torch.int64)), what
    assert np.array_equal(dry.cpu().numpy(), want['dry_fraction']), what
  return quant, dry, want


def _year_end(rng, dtype, n_outer, n_point, hour_interval=12, first='12-23',
              quantum=None):
  """The last days of 2019 - 2021 (2020 ends on day 366, which the others fill
  from their day 365): (times, x [n_outer, n_time, n_point])."""
  times = np.concatenate([
      sc.times_of(f'{y}-{first}', f'{y}-12-31', hour_interval)
      for y in (2019, 2020, 2021)])
  x = sc.precipitation(rng, (n_outer, times.size, n_point), dtype,
                       quantum=quantum)
  return times, x


def _plan(times, hour_interval):
  from weatherbench2_amd import climatology as cl
  hours = None if hour_interval == 24 else cl.hours_of(hour_interval)
  return cl.plan_groups(times, np.arange(times.size), 'explicit', hours)


def _lists(n_year, n_pos):
  """Every position with `n_year` members, time step y * n_pos + a."""
  member = (np.arange(n_year)[None, :] * n_pos
            + np.arange(n_pos)[:, None]).astype(np.int32).ravel()
  begin = (np.arange(n_pos + 1) * n_year).astype(np.int32)
  return begin, member


# ---------------------------------------------------------------------------
# the launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_point', [1, 5, 16, 20])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_basic_hourly_two_hours_two_outer(torch, dtype, n_point):
  rng = np.random.default_rng(n_point)
  times, x = _year_end(rng, dtype, 2, n_point)
  plan = _plan(times, 12)
  assert plan.n_cycle == 2 and plan.axis[-1] == 366 and plan.n_year == (3, 3)
  for qs, thr in (([2 / 3], THR), (sc.QUANTILES, None)):
    _, dry, want = _check_launch(
        torch, x, plan.group_begin, plan.member, plan.fill, 2, plan.n_pos, 5,
        qs, thr, 3, what=f'{dtype} n_point={n_point}')
    assert np.isfinite(want['quantile']).mean() > 0.9
    assert thr is None or 0.2 < dry.mean().item() < 0.7


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_edge_data(torch, dtype):
  rng = np.random.default_rng(3)
  times, x = _year_end(rng, dtype, 1, 6, 24)
  x[rng.uniform(size=x.shape) < 0.1] = np.nan
  x[:, :, 4] = rng.uniform(0, 0.2e-3, size=x.shape[:2]).astype(dtype)  # dry
  x[:, :, 5] = np.nan
  keep = np.ones(times.size, dtype=bool)
  keep[12] = False  # a gap day in 2020
  times, x = times[keep], x[:, keep]
  plan = _plan(times, 24)
  quant, dry, want = _check_launch(
      torch, x, plan.group_begin, plan.member, plan.fill, 1, plan.n_pos, 5,
      [2 / 3], THR, 3, what=dtype)
  quant, dry = quant.cpu().numpy(), dry.cpu().numpy()
  assert np.isnan(quant[0, 0, :, 4]).all() and (dry[0, :, 4] == 1).all()
  assert np.isnan(quant[0, 0, :, 5]).all() and (dry[0, :, 5] == 0).all()
  assert np.isfinite(quant[0, 0, :, :4]).mean() > 0.5
  _check_launch(torch, x, plan.group_begin, plan.member, plan.fill, 1,
                plan.n_pos, 5, sc.QUANTILES, what=dtype + ' quantiles')


@pytest.mark.parametrize('window, n_pos', [(3, 9), (21, 7)])
def test_window_shapes(torch, window, n_pos):
  """W = 3 (one day with a weight) and a window that wraps three times."""
  case = sc.december(n_pos=n_pos, window_size=window, n_point=5)
  plan = _plan(case['times'], 24)
  assert plan.n_pos == n_pos
  x = case['data'][None]
  for qs, thr in (([2 / 3], THR), (sc.QUANTILES, None)):
    _check_launch(torch, x, plan.group_begin, plan.member, plan.fill, 1, n_pos,
                  window, qs, thr, 3, what=f'W={window}')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_position_blocks(torch, dtype):
  from weatherbench2_amd import engine
  geo = engine.window_quantile_geometry(getattr(torch, dtype), 3, 5)
  d = geo['positions']
  assert d >= 2
  for n_pos in (d - 1, d, d + 1):
    case = sc.december(np.dtype(dtype).type, n_pos=n_pos, window_size=5,
                       n_point=3, seed=n_pos)
    plan = _plan(case['times'], 24)
    _check_launch(torch, case['data'][None], plan.group_begin, plan.member,
                  plan.fill, 1, n_pos, 5, [0.0, 2 / 3, 1.0], THR, 3,
                  what=f'{dtype} n_pos={n_pos}')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_regime_boundaries(torch, dtype):
  """The largest group of every tile width and one member more, for the
  script's window of 61; past the last regime the call refuses."""
  from weatherbench2_amd import _lib
  from weatherbench2_amd import engine
  window, n_pos, n_point = 61, 7, 3
  tdtype = getattr(torch, dtype)
  widths, last = {}, 0
  for n_year in range(1, 700):
    try:
      geo = engine.window_quantile_geometry(tdtype, n_year, window)
    except _lib.Wb2HipError:
      break
    assert geo['lds_bytes'] <= 160 * 1024
    widths[geo['tile_points']] = n_year
    last = n_year
  assert sorted(widths) == [1, 2, 4, 8, 16][:len(widths)] and len(widths) >= 4
  rng = np.random.default_rng(9)
  for n_year in sorted(set(widths.values()) | {v + 1 for v in widths.values()
                                               if v < last}):
    begin, member = _lists(n_year, n_pos)
    x = sc.precipitation(rng, (1, n_year * n_pos, n_point), dtype)
    _check_launch(torch, x, begin, member, None, 1, n_pos, window, [2 / 3],
                  THR, n_year, what=f'{dtype} n_year={n_year}')
  begin, member = _lists(last + 1, n_pos)
  x = np.zeros((1, (last + 1) * n_pos, n_point), dtype)
  with pytest.raises(_lib.Wb2HipError, match='does not fit'):
    engine.window_quantile(_dev(torch, x), None, 1, x.shape[1], n_point, begin,
                           1, n_pos, _dev(torch, member), None,
                           sn.window_weights(window), [0.5])


def test_ties_with_different_weights(torch):
  rng = np.random.default_rng(21)
  times, x = _year_end(rng, 'float32', 1, 5, 24, first='12-01',
                       quantum=1e-3)
  plan = _plan(times, 24)
  _, _, want = _check_launch(torch, x, plan.group_begin, plan.member,
                             plan.fill, 1, plan.n_pos, 9, sc.QUANTILES,
                             what='ties')
  assert np.unique(x).size < 120 < x.size
  _check_launch(torch, x, plan.group_begin, plan.member, plan.fill, 1,
                plan.n_pos, 9, [2 / 3], THR, 3, what='ties seeps')


def test_slab_table_and_validation(torch):
  from weatherbench2_amd import _lib
  from weatherbench2_amd import engine
  rng = np.random.default_rng(4)
  n_year, n_pos, n_point = 3, 6, 5
  begin, member = _lists(n_year, n_pos)
  base = sc.precipitation(rng, (40, n_point), np.float32)
  table = rng.permutation(40)[:2 * n_year * n_pos].reshape(2, -1).astype(
      np.int64)
  _check_launch(torch, base[table], begin, member, None, 1, n_pos, 5,
                [0.3, 2 / 3], THR, n_year, x_dev=_dev(torch, base),
                slab=table.ravel(), what='slab')
  x = _dev(torch, base[table])
  call = lambda **k: engine.window_quantile(**{**dict(
      x=x, slab=None, n_outer=2, n_time=n_year * n_pos, n_point=n_point,
      group_begin=begin, n_cycle=1, n_pos=n_pos, member=_dev(torch, member),
      fill=None, weights=[0, 1, 2, 1, 0], quantiles=[0.5]), **k})
  with pytest.raises(_lib.Wb2HipError, match='odd'):
    call(weights=[1, 2, 1, 0])
  with pytest.raises(_lib.Wb2HipError, match='negative'):
    call(weights=[0, 1, -2, 1, 0])
  with pytest.raises(_lib.Wb2HipError, match='counters'):
    call(weights=[0, 2**30, 2**30, 2**30, 0])
  with pytest.raises(_lib.Wb2HipError, match='not in'):
    call(quantiles=[1.5])
  bad = begin.copy()
  bad[2] = bad[1] - 1
  with pytest.raises(_lib.Wb2HipError, match='decreases'):
    call(group_begin=bad)
  quant, dry = call(quantiles=[])
  assert quant.shape == (0, 2, n_pos, n_point) and dry is None


# ---------------------------------------------------------------------------
# the public API on the device
# ---------------------------------------------------------------------------
def _dataset(case, data):
  from weatherbench2_amd import xarray_lite as xl
  return xl.Dataset({sc.VAR: xl.DataArray(data, case['dims'])},
                    coords={'time': case['times']})


def _seeps(case, data):
  from weatherbench2_amd import climatology as cl
  out = cl.compute_seeps_chunk(
      _dataset(case, data), frequency=case['frequency'],
      window_size=case['window_size'], clim_years=case['clim_years'],
      hour_interval=case['hour_interval'],
      seeps_threshold_mm={sc.VAR: sc.DRY_MM})
  return (out[sc.VAR + '_seeps_threshold'],
          out[sc.VAR + '_seeps_dry_fraction'])


@pytest.fixture(scope='module')
def hourly_case():
  case = sc.hourly(n_point=5)
  want = sn.restate_hourly(case['times'], case['data'], [0, 12], 5,
                           [2 / 3], THR)
  return case, want


def _assert_seeps(thr, dry, want, what):
  """(hour, dayofyear, row, point), in any order of the last three."""
  order = [thr.dims.index(d) for d in ('hour', 'dayofyear', 'row', 'point')]
  tv = np.transpose(thr.values, order)[:, :, 0]
  dv = np.transpose(dry.values, order)[:, :, 0]
  sn.assert_within(tv, want['quantile'][:, 0],
                   sn.interval_bound(want['k'][:, 0], want['xmax'][:, 0]),
                   what)
  assert np.array_equal(dv, want['dry_fraction']), what


def test_input_layouts_are_read_in_place(torch, hourly_case, monkeypatch):
  from weatherbench2_amd import engine
  from weatherbench2_amd import xarray_lite as xl
  case, want = hourly_case
  case = dict(case, dims=('time', 'row', 'point'))
  data = case['data'][:, None, :]  # (slabs of one row)
  n_time = data.shape[0]
  pad = np.full((3,) + data.shape[1:], 7.0, dtype=data.dtype)
  big = _dev(torch, np.concatenate([pad, data, pad]))
  seen = []
  real = engine.window_quantile
  monkeypatch.setattr(engine, 'window_quantile', lambda x, slab, *a, **k: (
      seen.append((x.data_ptr(), slab is not None)), real(x, slab, *a, **k))[1])
  view = big[3:3 + n_time]
  gather = xl.SlabGather(big, 3 + np.arange(n_time))
  before = big.clone()
  for label, source in (('view', view), ('gather', gather)):
    thr, dry = _seeps(case, source)
    assert thr.data.is_cuda and thr.data.dtype == torch.float64
    assert thr.dims == ('hour', 'dayofyear', 'row', 'point')
    _assert_seeps(thr, dry, want, label)
  assert seen[0] == (view.data_ptr(), False)  # (a view of whole slabs)
  assert seen[1] == (big.data_ptr(), True)
  assert torch.equal(before.view(torch.int32), big.view(torch.int32))
  inner = dict(case, dims=('row', 'point', 'time'))
  thr, dry = _seeps(inner, _dev(torch, np.ascontiguousarray(
      np.moveaxis(data, 0, -1))))
  assert thr.dims == ('hour', 'row', 'point', 'dayofyear')
  _assert_seeps(thr, dry, want, 'time innermost')


def test_daily_frequency_and_quantile_chunk(torch):
  from weatherbench2_amd import climatology as cl
  case = sc.daily(n_point=3)
  thr, dry = _seeps(case, _dev(torch, case['data']))
  host_thr, host_dry = _seeps(case, case['data'])
  assert thr.dims == ('dayofyear', 'point') and thr.data.is_cuda
  # (the daily means of K13 have the host path's bits: the same samples)
  days = case['data'].reshape(-1, 2, 3).mean(axis=1)
  want = sn.restate_hourly(case['times'][::2], days, None, 5,
                           list(sc.QUANTILES) + [2 / 3], THR)
  bound = sn.interval_bound(want['k'][0], want['xmax'][0])
  sn.assert_within(thr.values, want['quantile'][0, 5], bound[5], 'daily')
  assert np.array_equal(dry.values, want['dry_fraction'][0])
  assert np.array_equal(dry.values, host_dry.values)
  sn.assert_within(host_thr.values, want['quantile'][0, 5], bound[5], 'host')
  out = cl.compute_stat_chunk(
      _dataset(case, _dev(torch, case['data'])), frequency='daily',
      window_size=5, clim_years=case['clim_years'], statistic='quantile',
      quantiles=sc.QUANTILES)
  da = out[sc.VAR + '_quantile']
  assert da.dims == ('quantile', 'dayofyear', 'point') and da.data.is_cuda
  assert out.coords['quantile'].tolist() == list(sc.QUANTILES)
  free = sn.restate_hourly(case['times'][::2], days, None, 5, sc.QUANTILES)
  sn.assert_within(da.values, free['quantile'][0],
                   sn.interval_bound(free['k'][0], free['xmax'][0]),
                   'quantile chunk')


def test_device_climatology_feeds_seeps(torch):
  from weatherbench2_amd import climatology as cl
  from weatherbench2_amd import metrics as gm
  from weatherbench2_amd import xarray_lite as xl
  rng = np.random.default_rng(12)
  n_lat, n_lon = 8, 4
  lat = np.linspace(-87.5, 87.5, n_lat)
  lon = np.linspace(0, 360, n_lon, endpoint=False)
  obs_times = sc.times_of('2019-01-01', '2021-12-31', 6)
  obs = sc.precipitation(rng, (len(obs_times), n_lat, n_lon), np.float32,
                         dry=0.3)
  grid = {'latitude': lat, 'longitude': lon}
  dims = ('time', 'latitude', 'longitude')
  kw = dict(frequency='hourly', hour_interval=6, window_size=5,
            start_year=2019, end_year=2021, statistics=['seeps'],
            seeps_dry_threshold_mm={sc.VAR: 0.25})
  on_device = cl.compute_climatology(
      xl.Dataset({sc.VAR: xl.DataArray(_dev(torch, obs), dims)},
                 {'time': obs_times, **grid}), **kw)
  on_host = cl.compute_climatology(
      xl.Dataset({sc.VAR: xl.DataArray(obs, dims)},
                 {'time': obs_times, **grid}), **kw)
  names = [sc.VAR + '_seeps_threshold', sc.VAR + '_seeps_dry_fraction']
  assert list(on_device.data_vars) == names == list(on_host.data_vars)
  for name in names:
    assert on_device[name].data.is_cuda
    assert on_device[name].dims == ('hour', 'dayofyear', 'latitude',
                                    'longitude')
  assert np.array_equal(on_device[names[1]].values, on_host[names[1]].values)
  times = sc.times_of('2020-02-27', '2020-03-02', 6)
  coords = {'time': times, **grid}
  f = sc.precipitation(rng, (len(times), n_lat, n_lon), np.float32)
  t = sc.precipitation(rng, (len(times), n_lat, n_lon), np.float32)
  fds = xl.Dataset({sc.VAR: xl.DataArray(_dev(torch, f), dims)}, coords)
  tds = xl.Dataset({sc.VAR: xl.DataArray(_dev(torch, t), dims)}, coords)
  got = gm.SEEPS(climatology=on_device).compute_chunk(fds, tds)[sc.VAR].values
  host_clim = xl.Dataset(
      {n: xl.DataArray(_dev(torch, on_host[n].values), on_host[n].dims)
       for n in names}, dict(on_host.coords))
  want = gm.SEEPS(climatology=host_clim).compute_chunk(fds, tds)[sc.VAR].values
  assert np.isfinite(want).all()
  np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
