"""Resampling in time on the GPU: every fixture case through the public API
on device and host inputs, the K13 entry point across tile, vector, look-ahead
and grid edges, unaligned bases, mask consistency, odd ranges, slab tables
read in place, NaN/inf isolation, rolling windows and the hand-over to
`quantiles.quantile`.  The expected values are those of the NumPy restatement
(tests/resample_np.py), which tests/test_resampling_cpu.py pins to the
reference fixtures and to pandas."""
import numpy as np
import pytest

from tests import resample_cases as rc
from tests import resample_np as rn
from tests.test_resampling_cpu import (GOLDEN_DIR, check_product, run_product,
                                       to_lite)

pytestmark = pytest.mark.gpu

CASES = sorted(rc.all_cases())
MODES = sorted(rc.MODES)
STATS = ('sum', 'mean', 'min', 'max')  # the order of the mask bits


@pytest.fixture(scope='module')
def golden():
  return rc.load_golden(GOLDEN_DIR)


def _torch_dtype(dtype):
  import torch
  return {'float32': torch.float32, 'float64': torch.float64}[
      np.dtype(dtype).name]


def _stats(x, ranges, statistics=STATS, skipna=False, slab=None, shape=None,
           bins_per_group=1):
  """engine.time_bin_stats on a device tensor -> {statistic: host array}."""
  import torch
  from weatherbench2_amd import engine
  n_outer, n_time, n_point = shape or x.shape
  table = None if slab is None else torch.from_numpy(
      np.ascontiguousarray(slab, dtype=np.int64)).cuda()
  bins = torch.from_numpy(np.ascontiguousarray(
      np.asarray(ranges, dtype=np.int32).reshape(-1, 2))).cuda()
  out = engine.time_bin_stats(x, table, n_outer, n_time, n_point, bins,
                              list(statistics), skipna, bins_per_group)
  assert list(out) == list(statistics)
  for a in out.values():
    assert a.dtype == x.dtype and a.is_cuda
    assert tuple(a.shape) == (n_outer, len(bins), n_point)
  return {s: a.cpu().numpy() for s, a in out.items()}


def _series(rs, shape, dtype, nan=0.1):
  x = (rs.standard_normal(shape) * 7).astype(dtype)
  x[rs.random_sample(shape) < nan] = np.nan
  return x


def _check(got: dict, host, ranges, skipna, what=''):
  want = rn.bin_stats(host, 1, [tuple(r) for r in ranges], skipna)
  for s, a in got.items():
    rn.assert_same(a, want[s], f'{what}/{s}')


# ---------------------------------------------------------------------------
# the public API on every fixture case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_fixture_cases_on_device_and_host_inputs(golden, cname, mode):
  case = rc.all_cases()[cname]()
  for device in (True, False):
    res = run_product(case, to_lite(case, device=device), rc.MODES[mode])
    check_product(res, case, cname, mode, golden, device=device)


# ---------------------------------------------------------------------------
# the C ABI across its edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_sizes_across_tile_lookahead_and_group_edges(dtype, skipna):
  import torch
  from weatherbench2_amd import engine
  rs = np.random.RandomState(11)
  geo = engine.time_window_geometry(_torch_dtype(dtype), True)
  narrow = engine.time_window_geometry(_torch_dtype(dtype), False)
  tile, ahead = geo['tile_points'], geo['steps_ahead']
  assert narrow['steps_ahead'] == ahead
  lengths = [1, ahead - 1, ahead, ahead + 1, 25]
  # consecutive bins of every length, then one over everything
  edges = np.concatenate([[0], np.cumsum(lengths)])
  n_time = int(edges[-1])
  ranges = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])] + [
      (0, n_time), (2, 20)]
  n_bin = len(ranges)
  assert n_bin % 3 and n_bin % 2
  vec = 16 // np.dtype(dtype).itemsize
  points = sorted({1, 3, narrow['tile_points'] - 1, narrow['tile_points'],
                   narrow['tile_points'] + 1, tile - 1, tile, tile + 1,
                   tile + vec, 2 * tile, 2 * tile + 5})
  for n_point in points:
    for n_outer in (1, 5):
      if n_outer == 5 and n_point not in (3, tile, 2 * tile + 5):
        continue
      host = _series(rs, (n_outer, n_time, n_point), dtype)
      x = torch.from_numpy(host).cuda()
      groups = (1, 3, n_bin, n_bin + 2) if n_point in (3, tile + 1) else (
          1 + n_point % 3,)
      for group in groups:
        got = _stats(x, ranges, skipna=skipna, bins_per_group=group)
        _check(got, host, ranges, skipna, f'{n_point}/{n_outer}/{group}')


def test_more_outer_indices_than_one_grid_row():
  import torch
  from weatherbench2_amd import engine
  geo = engine.time_window_geometry(torch.float32, False)
  n_outer = geo['max_grid_outer'] + 1
  rs = np.random.RandomState(12)
  host = _series(rs, (n_outer, 2, 1), np.float32)
  ranges = [(0, 2), (1, 2), (0, 1)]
  got = _stats(torch.from_numpy(host).cuda(), ranges, skipna=True,
               bins_per_group=2)
  _check(got, host, ranges, True, 'grid')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_unaligned_base_takes_the_scalar_path(dtype):
  """A base one element past a 16-byte boundary: the same bits as aligned."""
  import torch
  rs = np.random.RandomState(13)
  vec = 16 // np.dtype(dtype).itemsize
  host = _series(rs, (2, 9, 8 * vec), dtype)
  ranges = [(0, 5), (5, 9), (2, 7)]
  buf = torch.empty(host.size + 1, dtype=_torch_dtype(dtype), device='cuda')
  assert buf.data_ptr() % 16 == 0
  buf[1:] = torch.from_numpy(host).cuda().reshape(-1)
  view = buf[1:].view(host.shape)
  assert view.data_ptr() % 16 != 0 and view.is_contiguous()
  for skipna in (False, True):
    offset = _stats(view, ranges, skipna=skipna)
    aligned = _stats(torch.from_numpy(host).cuda(), ranges, skipna=skipna)
    _check(offset, host, ranges, skipna, 'offset')
    for s in STATS:
      assert offset[s].tobytes() == aligned[s].tobytes(), s


@pytest.mark.parametrize('skipna', [False, True])
def test_every_mask_gives_each_statistic_the_bits_it_has_alone(skipna):
  import torch
  rs = np.random.RandomState(14)
  host = _series(rs, (2, 13, 24), np.float32, nan=0.2)
  host[:, :, 5] = np.nan
  host[0, 3, 7], host[0, 4, 7] = np.inf, -np.inf
  x = torch.from_numpy(host).cuda()
  ranges = [(0, 6), (6, 13), (3, 4), (0, 13)]
  alone = {s: _stats(x, ranges, [s], skipna)[s] for s in STATS}
  _check(alone, host, ranges, skipna, 'alone')
  for mask in range(1, 16):
    names = [s for k, s in enumerate(STATS) if mask >> k & 1]
    got = _stats(x, ranges, names, skipna)
    for s in names:
      assert got[s].tobytes() == alone[s].tobytes(), (mask, s)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_overlapping_empty_and_negative_ranges(dtype):
  import torch
  rs = np.random.RandomState(15)
  host = _series(rs, (3, 10, 12), dtype)
  x = torch.from_numpy(host).cuda()
  ranges = [(0, 4), (2, 6), (2, 6), (5, 5), (7, 3), (-1, 3), (-5, -2),
            (8, 10), (0, 10), (9, 11), (10, 12), (4, 5)]
  for skipna in (False, True):
    for group in (1, 5, 32):
      got = _stats(x, ranges, skipna=skipna, bins_per_group=group)
      _check(got, host, ranges, skipna, f'ranges/{group}')
      for s in STATS:  # sum included, skipna included
        for b in (3, 4, 5, 6, 9, 10):
          assert np.isnan(got[s][:, b]).all(), (s, b)


# ---------------------------------------------------------------------------
# the slab table
# ---------------------------------------------------------------------------
def test_views_gathers_and_permuted_times_are_read_in_place(monkeypatch):
  """A time-sliced view, a SlabGather and a permuted time order reach the
  kernel as the resident tensor's own pointer with a slab table: no copy of
  the input is made.  Time innermost costs exactly one."""
  import torch
  from weatherbench2_amd import engine, resampling
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(16)
  dims = ('member', 'time', 'latitude', 'longitude')
  sizes = {'member': 2, 'time': 23, 'latitude': 3, 'longitude': 8}
  host = (rs.standard_normal(tuple(sizes.values())) * 5).astype(np.float32)
  full = torch.from_numpy(host).cuda()
  times = rc.time_axis('2020-01-01T00', 6, 23)
  calls = []
  real = engine.time_bin_stats

  def spy(x, slab, *a, **k):
    calls.append((x.data_ptr(), None if slab is None
                  else slab.cpu().numpy().copy()))
    return real(x, slab, *a, **k)
  monkeypatch.setattr(engine, 'time_bin_stats', spy)
  copies = []
  real_c = torch.Tensor.contiguous
  monkeypatch.setattr(torch.Tensor, 'contiguous',
                      lambda self, *a, **k: (copies.append(self.is_contiguous()),
                                             real_c(self, *a, **k))[1])

  def run(data, time_values, the_dims=dims):
    ds = xl.Dataset({'t': xl.DataArray(data, the_dims)}, {'time': time_values})
    return resampling.resample_in_time(
        ds, method='resample', period='1d', mean_vars=['t'], max_vars=['t'],
        sum_vars=['t'])

  def want(values, time_values, axis=1):
    _, ranges = rn.resample_bins(time_values, rn.NS['d'], 'left')
    return rn.bin_stats(values, axis, ranges, False)

  # the contiguous tensor: no table at all, one launch for three statistics
  got = run(full, times)
  assert calls == [(full.data_ptr(), None)]
  for name, s in (('t', 'mean'), ('t_max', 'max'), ('t_sum', 'sum')):
    assert got[name].data.is_cuda
    rn.assert_same(got[name].values, want(host, times)[s], 'whole')
  # every other time, from the second one
  view = full[:, 1::2]
  assert not view.is_contiguous()
  got = run(view, times[1::2])
  assert all(copies)  # .contiguous() only ever met contiguous tensors
  ptr, table = calls[-1]
  assert ptr == view.data_ptr() != full.data_ptr()
  assert np.array_equal(table, (np.arange(2)[:, None] * 23
                                + np.arange(view.shape[1])[None, :] * 2).ravel())
  rn.assert_same(got['t_sum'].values, want(host[:, 1::2], times[1::2])['sum'],
                 'sliced view')
  # a gather: the slabs of a resident base in a permuted time order, put back
  # in order by the table
  base = full.reshape(-1, sizes['latitude'], sizes['longitude'])
  index = np.stack([rs.permutation(23) + m * 23 for m in (1, 0)])
  shuffled = host.reshape((-1,) + host.shape[2:])[index]
  materialized = []
  real_m = xl.SlabGather.materialize
  monkeypatch.setattr(xl.SlabGather, 'materialize',
                      lambda self, *a, **k: (materialized.append(1),
                                             real_m(self, *a, **k))[1])
  got = run(xl.SlabGather(base, index), times)
  assert not materialized and all(copies)
  ptr, table = calls[-1]
  assert ptr == base.data_ptr()
  assert np.array_equal(table, index.ravel())
  assert got['t'].data.is_cuda
  rn.assert_same(got['t'].values, want(shuffled, times)['mean'], 'gather')
  # a permuted time order as a strided-index view of the resident tensor
  order = rs.permutation(23)
  got = run(xl.SlabGather(base, np.stack([order, order + 23])), times)
  assert not materialized and all(copies)
  rn.assert_same(got['t_max'].values, want(host[:, order], times)['max'],
                 'permuted')
  # time innermost: exactly one transposing copy, dims kept
  n_calls = len(copies)
  inner = full.permute(0, 2, 3, 1).contiguous()
  assert len(copies) == n_calls + 1
  got = run(inner, times, ('member', 'latitude', 'longitude', 'time'))
  assert copies[n_calls + 1:].count(False) == 1
  assert got['t'].dims == ('member', 'latitude', 'longitude', 'time')
  rn.assert_same(got['t'].values,
                 want(np.ascontiguousarray(host.transpose(0, 2, 3, 1)), times,
                      axis=3)['mean'], 'innermost')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_a_nan_or_inf_stays_in_its_own_point(dtype):
  """One special value changes no neighbouring point of its 16-byte vector."""
  import torch
  rs = np.random.RandomState(17)
  vec = 16 // np.dtype(dtype).itemsize
  clean = (rs.standard_normal((1, 9, 4 * vec)) * 3).astype(dtype)
  ranges = [(0, 4), (4, 9)]
  for skipna in (False, True):
    base = _stats(torch.from_numpy(clean).cuda(), ranges, skipna=skipna)
    for special in (np.nan, np.inf, -np.inf):
      for lane in range(vec):
        host = clean.copy()
        host[0, 2, vec + lane] = special
        got = _stats(torch.from_numpy(host).cuda(), ranges, skipna=skipna)
        _check(got, host, ranges, skipna, f'{special}/{lane}')
        others = np.arange(4 * vec) != vec + lane
        for s in STATS:
          assert (got[s][..., others].tobytes()
                  == base[s][..., others].tobytes()), (special, lane, s)
          assert got[s][0, 1].tobytes() == base[s][0, 1].tobytes()


# ---------------------------------------------------------------------------
# rolling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('label_side', ['left', 'right'])
def test_rolling_windows_and_the_label_shift(label_side):
  import torch
  from weatherbench2_amd import resampling
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(18)
  n_time = 14
  host = _series(rs, (n_time, 2, 37), np.float32, nan=0.02)
  times = rc.time_axis('2020-01-01T00', 6, n_time)
  ds = xl.Dataset({'x': xl.DataArray(torch.from_numpy(host).cuda(),
                                     ('time', 'level', 'point'))},
                  {'time': times})
  step = np.timedelta64(6 * 3600 * 10**9, 'ns')
  for w in (1, 4, 7, n_time, n_time + 1):
    for skipna in (False, True):
      res = resampling.resample_in_time(
          ds, method='rolling', period=f'{6 * w}h', mean_vars=['x'],
          min_vars=['x'], max_vars=['x'], sum_vars=['x'], skipna=skipna,
          label_side=label_side)
      want = rn.bin_stats(host, 0, rn.rolling_bins(n_time, w), False)
      for name, s in (('x', 'mean'), ('x_min', 'min'), ('x_max', 'max'),
                      ('x_sum', 'sum')):
        assert res[name].data.is_cuda
        rn.assert_same(res[name].values, want[s], f'{w}/{s}')
      assert np.isnan(res['x_sum'].values[:min(w - 1, n_time)]).all()
      shift = step - w * step if label_side == 'left' else step
      np.testing.assert_array_equal(np.asarray(res.coords['time']),
                                    times + shift)


# ---------------------------------------------------------------------------
# the hand-over
# ---------------------------------------------------------------------------
def test_resampled_result_goes_into_quantile_on_the_device(monkeypatch):
  import torch
  from weatherbench2_amd import feeder, quantiles, resampling
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(19)
  host = (rs.standard_normal((40, 4, 6)) * 5 + 280).astype(np.float32)
  times = rc.time_axis('2020-01-01T00', 6, 40)
  ds = xl.Dataset({'t': xl.DataArray(torch.from_numpy(host).cuda(),
                                     ('time', 'latitude', 'longitude'))},
                  {'time': times})
  downloads = []
  real = feeder.download
  monkeypatch.setattr(feeder, 'download',
                      lambda *a, **k: (downloads.append(1), real(*a, **k))[1])
  daily = resampling.resample_in_time(ds, method='resample', period='1d',
                                      mean_vars=['t'])
  q = quantiles.quantile(daily, [0.1, 0.5, 0.9], 'time', skipna=False)
  assert not downloads
  assert q['t'].data.is_cuda
  monkeypatch.undo()
  _, ranges = rn.resample_bins(times, rn.NS['d'], 'left')
  means = rn.bin_stats(host, 0, ranges, False)['mean']
  np.testing.assert_array_equal(
      q['t'].values, np.quantile(means, [0.1, 0.5, 0.9], axis=0))
