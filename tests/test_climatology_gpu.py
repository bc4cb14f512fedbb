"""Climatology by day of year on the GPU (K14): every fixture case through the
public API against the NumPy restatement, bit for bit; the moments kernel
across vector, tile, group-length, fill, grid and slab-table edges; the
smoothing kernel across axis and window lengths; the hand-over to ACC."""
import numpy as np
import pytest

from tests import climatology_cases as cc
from tests import climatology_np as cn
from tests.test_climatology_cpu import CASES, dataset_of, run_public

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
  import torch as module
  return module


def _dev(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# every fixture case, device and host inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('method', cc.METHODS)
@pytest.mark.parametrize('name', list(CASES))
def test_public_api_has_the_restatements_bits(torch, name, method):
  case = CASES[name]
  r = cc.restate(name, method)
  hourly = case['frequency'] == 'hourly'
  device_input = _dev(torch, case['data'])
  before = device_input.clone()
  for where, data in (('device', device_input), ('host', None)):
    for stat, da in zip(cc.STATS, run_public(case, method, data)):
      if where == 'device':
        assert da.data.is_cuda and da.data.dtype == torch.float64
      got = cc.in_restated_layout(da.values, da.dims, hourly, r['other_dims'])
      cn.assert_same(got, r[stat], f'{name} {method} {stat} {where}')
  assert torch.equal(before.view(torch.uint8), device_input.view(torch.uint8))


def test_one_moments_launch_serves_both_statistics_of_all_hours(torch):
  from weatherbench2_amd import climatology as cl
  from weatherbench2_amd import engine
  case = CASES['hourly6']
  launches = []
  old = engine.set_launch_hook(
      lambda when, what: launches.append(what) if when == 'begin' else None)
  try:
    out = cl.compute_climatology(
        dataset_of(case, _dev(torch, case['data'])), frequency='hourly',
        hour_interval=6, window_size=61, start_year=2019, end_year=2021,
        statistics=('mean', 'std'))
  finally:
    engine.set_launch_hook(old)
  assert launches.count('group_moments') == 1
  assert launches.count('first_finite') == 1
  assert launches.count('cycle_smooth') == 1
  r = cc.restate('hourly6', 'explicit')
  cn.assert_same(out['x'].values, r['mean'])
  cn.assert_same(out['x_std'].values, r['std'])


# ---------------------------------------------------------------------------
# wb2_group_moments and wb2_first_finite
# ---------------------------------------------------------------------------
def _groups(rs, lengths, n_time, absent=True):
  begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
  member = rs.randint(0, n_time, size=begin[-1]).astype(np.int32)
  if absent and member.size > 3:
    member[rs.choice(member.size, size=2, replace=False)] = -1
  return begin, member


def _check_moments(torch, x_host, x_dev, begin, member, fill, slab=None,
                   what=''):
  """Device pivot and moments against the restatement on `x_host`
  [n_outer, n_time, n_point] (the series as the slab table presents them)."""
  from weatherbench2_amd import engine
  n_outer, n_time, n_point = x_host.shape
  member_dev = _dev(torch, member)
  fill_dev = None if fill is None else _dev(torch, fill)
  slab_dev = None if slab is None else _dev(torch, slab)
  pivot = engine.first_finite(x_dev, slab_dev, n_outer, n_time, n_point,
                              member_dev)
  want_pivot = cn.first_finite(x_host, member)
  cn.assert_same(pivot.cpu().numpy(), want_pivot, what + ' pivot')
  got = engine.group_moments(x_dev, slab_dev, n_outer, n_time, n_point, begin,
                             member_dev, fill_dev, pivot)
  want = cn.group_moments(x_host, begin, member, fill, want_pivot)
  for name, g, w in zip(('count', 'sum', 'sumsq'), got, want):
    cn.assert_same(g.cpu().numpy(), w, f'{what} {name}')
  return got


def _series(rs, dtype, n_outer, n_time, n_point):
  x = (3.0 + rs.normal(size=(n_outer, n_time, n_point))).astype(dtype)
  x[rs.uniform(size=x.shape) < 0.1] = np.nan
  x[:, 0, :1] = np.nan  # (the pivot is not always the first member's sample)
  return x


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_moments_across_vector_tile_group_and_fill_edges(torch, dtype, wide):
  from weatherbench2_amd import engine
  geo = engine.climatology_geometry(getattr(torch, dtype), wide)
  tile, ahead = geo['tile_points'], geo['members_ahead']
  vec = 16 // np.dtype(dtype).itemsize
  lengths = [0, 1, ahead - 1, ahead, ahead + 1, 25, 0]
  n_time = 19
  rs = np.random.RandomState(7 + wide)
  for n_point in (1, 3, tile - 1, tile, tile + 1, tile + vec, 2 * tile + 5):
    x = _series(rs, dtype, 2, n_time, n_point)
    begin, member = _groups(rs, lengths, n_time)
    # wide: an aligned base (16-byte loads where n_point allows); narrow: a
    # base one element past a 16-byte boundary (scalar loads whatever n_point)
    flat = torch.empty(x.size + vec, dtype=getattr(torch, dtype),
                       device='cuda')
    off = 0 if wide else 1
    assert flat.data_ptr() % 16 == 0
    x_dev = flat[off:off + x.size].view(x.shape)
    x_dev.copy_(torch.from_numpy(x))
    nan_step = int(np.argmax(np.isnan(x[0]).any(axis=1)))
    fills = {'absent': None,
             'none': np.full(member.size, -1, np.int32),
             'random': rs.randint(-1, n_time, size=member.size).astype(
                 np.int32),
             'at_nan': np.full(member.size, nan_step, np.int32)}
    for label, fill in fills.items():
      _check_moments(torch, x, x_dev, begin, member, fill,
                     what=f'{dtype} wide={wide} n_point={n_point} fill={label}')


@pytest.mark.parametrize('n_outer', [5, 'grid_row_plus_one'])
def test_moments_across_outer_indices_and_grid_rows(torch, n_outer):
  from weatherbench2_amd import engine
  rs = np.random.RandomState(9)
  if n_outer == 'grid_row_plus_one':
    n_outer = engine.climatology_geometry(torch.float32)['max_grid_outer'] + 1
    n_time, n_point = 2, 1
  else:
    n_time, n_point = 11, 8
  x = _series(rs, np.float32, n_outer, n_time, n_point)
  begin, member = _groups(rs, [2, 0, 3], n_time, absent=False)
  got = _check_moments(torch, x, _dev(torch, x), begin, member, None,
                       what=f'n_outer={n_outer}')
  assert got[0].shape == (n_outer, 3, n_point)


def test_moments_read_through_a_slab_table(torch):
  """A time-sliced view, a permuted time order and a gather over a base differ
  in the table alone."""
  rs = np.random.RandomState(10)
  n_slab, n_outer, n_time, n_point = 40, 2, 9, 24
  base = _series(rs, np.float64, 1, n_slab, n_point)[0]
  base_dev = _dev(torch, base)
  begin, member = _groups(rs, [4, 1, 6], n_time)
  fill = rs.randint(-1, n_time, size=member.size).astype(np.int32)
  tables = {
      'sliced': np.stack([3 + np.arange(n_time), 20 + np.arange(n_time)]),
      'permuted': np.stack([rs.permutation(n_time),
                            20 + rs.permutation(n_time)]),
      'gather': rs.randint(0, n_slab, size=(n_outer, n_time)),
  }
  for label, table in tables.items():
    table = table.astype(np.int64)
    _check_moments(torch, base[table], base_dev, begin, member, fill,
                   slab=table.ravel(), what=label)


def test_views_and_gathers_are_read_in_place(torch, monkeypatch):
  from weatherbench2_amd import climatology as cl
  from weatherbench2_amd import engine
  from weatherbench2_amd import xarray_lite as xl
  case = CASES['common_years']
  r = cc.restate('common_years', 'explicit')
  data = case['data']
  n_time = data.shape[0]
  pad = np.full((3,) + data.shape[1:], 7.0)
  big = _dev(torch, np.concatenate([pad, data, pad]))
  seen = []
  real = engine.group_moments
  monkeypatch.setattr(engine, 'group_moments', lambda x, slab, *a, **k: (
      seen.append((x.data_ptr(), slab is not None)), real(x, slab, *a, **k))[1])
  view = big[3:3 + n_time]
  gather = xl.SlabGather(big, 3 + np.arange(n_time))
  for label, source in (('view', view), ('gather', gather)):
    ds = xl.Dataset({'x': xl.DataArray(source, case['dims'])},
                    coords={'time': case['times']})
    out = cl.compute_hourly_stat(ds, case['window_size'], case['clim_years'],
                                 24, 'mean')
    cn.assert_same(out['x'].values, r['mean'], label)
  assert seen[0] == (view.data_ptr(), False)  # (a view of whole slabs)
  assert seen[1] == (big.data_ptr(), True)


def test_a_nan_or_inf_stays_in_its_point(torch):
  rs = np.random.RandomState(11)
  n_time, n_point = 12, 1030
  x = (1.0 + rs.normal(size=(1, n_time, n_point))).astype(np.float32)
  clean = x.copy()
  x[0, 2, 5] = np.nan
  x[0, 3, 700] = np.inf
  x[0, 7, 1029] = -np.inf
  begin = np.array([0, 4, 8, 12], np.int32)
  member = np.arange(12, dtype=np.int32)
  got = _check_moments(torch, x, _dev(torch, x), begin, member, None)
  ref = _check_moments(torch, clean, _dev(torch, clean), begin, member, None)
  touched = np.zeros(n_point, dtype=bool)
  touched[[5, 700, 1029]] = True
  for g, w in zip(got, ref):
    g, w = g.cpu().numpy()[0], w.cpu().numpy()[0]
    assert np.array_equal(g[:, ~touched], w[:, ~touched])
  count = got[0].cpu().numpy()[0]
  assert count[0, 5] == 3 and count[1, 5] == 4  # only the group of step 2
  assert np.isinf(got[1].cpu().numpy()[0][0, 700])
  assert np.isfinite(got[1].cpu().numpy()[0][[1, 2], 700]).all()


# ---------------------------------------------------------------------------
# wb2_cycle_smooth
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_w', [1, 3, 7, 61])
@pytest.mark.parametrize('n_pos', [1, 5, 365, 366])
def test_smoothing_across_axis_and_window_lengths(torch, n_pos, n_w):
  from weatherbench2_amd import engine
  rs = np.random.RandomState(n_pos * 100 + n_w)
  n_outer, n_cycle, n_point = 2, 2, 5
  shape = (n_outer, n_cycle * n_pos, n_point)
  count = rs.randint(0, 4, size=shape).astype(np.float64)  # (some C = 0)
  mean = rs.normal(size=shape)
  total = np.where(count > 0, count * mean, 0.0)
  sumsq = np.where(count > 0, count * (mean ** 2 + rs.uniform(size=shape)),
                   0.0)
  # the two cycles must not mix: the second is far from the first
  total[:, n_pos:] += 1000.0 * count[:, n_pos:]
  sumsq[:, n_pos:] += 1e6 * count[:, n_pos:]
  pivot = rs.normal(size=(n_outer, n_point))
  # (a window of one has the weight 1 here; the reference's is 0 / 0)
  half = n_w // 2
  w = np.concatenate([np.linspace(0, 1, half + 1),
                      np.linspace(1, 0, half + 1)[1:]]) if n_w > 1 else \
      np.ones(1)
  w = w / w.mean()
  moments = tuple(_dev(torch, a) for a in (count, total, sumsq))
  for mode in ('explicit', 'fast'):
    want = dict(zip(('mean', 'std'), cn.cycle_smooth(
        mode, (count, total, sumsq), pivot, n_cycle, n_pos, w)))
    for asked in (('mean', 'std'), ('mean',), ('std',)):
      got = engine.cycle_smooth(mode, moments, _dev(torch, pivot), n_cycle,
                                n_pos, _dev(torch, w), asked)
      assert sorted(got) == sorted(asked)
      for s in asked:
        cn.assert_same(got[s].cpu().numpy(), want[s],
                       f'{mode} {s} n_pos={n_pos} n_w={n_w} of {asked}')
    # each cycle is what it would be alone
    for c in range(n_cycle):
      part = slice(c * n_pos, (c + 1) * n_pos)
      alone = cn.cycle_smooth(mode, tuple(a[:, part] for a in (
          count, total, sumsq)), pivot, 1, n_pos, w)
      cn.assert_same(want['mean'][:, part], alone[0])
      cn.assert_same(want['std'][:, part], alone[1])


# ---------------------------------------------------------------------------
# the hand-over
# ---------------------------------------------------------------------------
def test_device_climatology_feeds_acc(torch):
  from weatherbench2_amd import climatology as cl
  from weatherbench2_amd import metrics as gm
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(12)
  n_lat, n_lon = 9, 16
  lat = np.linspace(-90, 90, n_lat)
  lon = np.linspace(0, 360, n_lon, endpoint=False)
  obs_times = cc.times_of('2019-01-01', '2021-01-01', 12)
  obs = (280 + 5 * rs.normal(size=(len(obs_times), n_lat, n_lon))).astype(
      np.float32)
  grid = {'latitude': lat, 'longitude': lon}
  dims = ('time', 'latitude', 'longitude')
  kw = dict(frequency='hourly', hour_interval=12, window_size=7,
            start_year=2019, end_year=2020)
  on_device = cl.compute_climatology(
      xl.Dataset({'z': xl.DataArray(_dev(torch, obs), dims)},
                 {'time': obs_times, **grid}), **kw)
  assert on_device['z'].data.is_cuda
  assert on_device['z'].dims == ('hour', 'dayofyear', 'latitude', 'longitude')
  host_copy = xl.Dataset({'z': xl.DataArray(on_device['z'].values,
                                            on_device['z'].dims)},
                         {k: on_device.coords[k] for k in
                          ('hour', 'dayofyear', 'latitude', 'longitude')})
  times = cc.times_of('2020-02-27', '2020-03-02', 12)
  coords = {'time': times, **grid}
  f = 280 + 5 * rs.normal(size=(len(times), n_lat, n_lon))
  t = 280 + 5 * rs.normal(size=(len(times), n_lat, n_lon))
  fds = xl.Dataset({'z': xl.DataArray(f, dims)}, coords)
  tds = xl.Dataset({'z': xl.DataArray(t, dims)}, coords)
  got = gm.ACC(climatology=on_device).compute_chunk(fds, tds)['z'].values
  want = gm.ACC(climatology=host_copy).compute_chunk(fds, tds)['z'].values
  assert np.isfinite(want).all() and (np.abs(want) <= 1).all()
  cn.assert_same(got, want)
