"""CRPS decomposition on the device (-m gpu): K20 (csrc/crps_bins.hip) against
the host path of weatherbench2_amd/crps_decomposition.py, bit for bit, at the
smallest shapes at which the kernel can go wrong."""
import numpy as np
import pytest
import torch

from tests import crps_decomposition_cases as cases
from tests import helpers
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import xarray_lite as xl

pytestmark = pytest.mark.gpu

g = helpers.to_gpu_dataset
NAME = cases.NAME
_ID = lambda v: getattr(v, '__name__', None) or str(v)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_dataset(ds: xl.Dataset) -> xl.Dataset:
  """The same Dataset with its variables in HBM."""
  return xl.Dataset({k: xl.DataArray(_dev(v.values), v.dims)
                     for k, v in ds.items()}, ds.coords, ds.attrs)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64) if a.dtype == np.float64 else a


def _both(ens, truth, cls, n_class):
  """((device sums, counts), (host sums, counts)) of contiguous [M, O, R, C]
  members and [O, R, C] truth."""
  n_member, n_outer, n_row, n_col = ens.shape
  stride = n_outer * n_row * n_col
  host = cd.host_sums(ens, stride, n_member, None, truth, None, n_outer, n_row,
                      n_col, cls, n_class)
  dev = engine.crps_bin_sums(_dev(ens), stride, n_member, None, _dev(truth),
                             None, n_outer, n_row, n_col, cls, n_class)
  assert dev[0].dtype == torch.float64 and dev[1].dtype == torch.int32
  assert tuple(dev[0].shape) == host[0].shape
  assert tuple(dev[1].shape) == host[1].shape
  return tuple(x.cpu().numpy() for x in dev), host


def _assert_same(dev, host, msg=''):
  np.testing.assert_array_equal(_bits(dev[0]), _bits(host[0]), err_msg=msg)
  np.testing.assert_array_equal(dev[1], host[1], err_msg=msg)


# below, at and above one wave and the column tile (one, two and four tiles of
# a row, with and without a partial last one); one row and several (a wave, a
# workgroup of its own, per row)
COLS = (1, 63, 64, 65, 72, 129, 240)
ROWS = (1, 2, 5, 19)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', cases.MEMBERS)
def test_device_sums_equal_the_host_path(n_member, dtype):
  for a, n_col in enumerate(COLS):
    for b, n_row in enumerate(ROWS):
      ens, truth = cases.arrays(n_member, 2, n_row, n_col, dtype,
                                cases.NANS[(a + b) % 4], seed=n_col)
      # runs of columns with a wrapped first class, and one class left empty
      n_class = min(5, n_col) + 1
      cls = cases.classes(n_col, n_class - 1)
      dev, host = _both(ens, truth, cls, n_class)
      _assert_same(dev, host, str((n_col, n_row)))
      assert (host[1][..., 2].sum(-1) <= n_col).all()
      assert not host[0][:, :, n_class - 1].any()


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_a_class_border_inside_a_wave_and_a_wrapped_class(dtype):
  # two waves of columns: the borders 20 | 70 | 100 fall inside both, class 0
  # holds the first and the last columns, class 2 is two separate runs
  n_col = 128
  cls = np.zeros(n_col, np.int32)
  cls[20:70] = 1
  cls[70:100] = 2
  cls[40:44] = 2
  assert cls[0] == cls[-1] == 0
  for n_member in (3, 50):
    ens, truth = cases.arrays(n_member, 1, 3, n_col, dtype, 'both')
    dev, host = _both(ens, truth, cls, 3)
    _assert_same(dev, host)
    again, _ = _both(ens, truth, cls, 3)
    _assert_same(again, dev)  # two runs of the same launch
  # ties: the planted cases, the counts by hand
  ens, truth, below, above = cases.tie_case(dtype)
  dev, host = _both(ens, truth, np.zeros(8, np.int32), 1)
  _assert_same(dev, host)
  np.testing.assert_array_equal(dev[1][0, :, 0, 0], below[0].sum(-1))
  np.testing.assert_array_equal(dev[1][0, :, 0, 1], above[0].sum(-1))


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_the_largest_member_count_at_two_rows_of_65(dtype):
  geo = engine.crps_bins_geometry(torch.from_numpy(np.empty(0, dtype)).dtype)
  assert (geo['min_member'], geo['max_member']) == (cd.MIN_MEMBERS,
                                                    cd.MAX_MEMBERS)
  ens, truth = cases.arrays(geo['max_member'], 1, 2, 65, dtype, 'both')
  dev, host = _both(ens, truth, cases.classes(65, 3), 3)
  _assert_same(dev, host)
  with pytest.raises(ValueError, match='members'):
    big = np.zeros((geo['max_member'] + 1, 1, 2, 65), dtype)
    engine.crps_bin_sums(_dev(big), 130, geo['max_member'] + 1, None,
                         _dev(truth), None, 1, 2, 65, np.zeros(65, np.int32),
                         1)


def test_outer_indices_beyond_one_grid_row():
  geo = engine.crps_bins_geometry(torch.float32, 2, 1)
  n_outer = geo['max_grid_outer'] + 1
  rs = np.random.RandomState(4)
  ens = (np.round(rs.normal(size=(2, n_outer, 1, 3)) * 4) / 4
         ).astype(np.float32)
  truth = (np.round(rs.normal(size=(n_outer, 1, 3)) * 4) / 4
           ).astype(np.float32)
  truth[-1, 0, 2] = np.nan  # the last point of the last outer index
  dev, host = _both(ens, truth, np.zeros(3, np.int32), 1)
  _assert_same(dev, host)
  assert host[1][-1, 0, 0, 2] == 2


def test_sums_walk_the_slab_tables():
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32,
                            'both', seed=5)
  cls = cases.classes(n_col, 2)
  want = cd.host_sums(ens, ens[0].size, n_member, None, truth, None, n_outer,
                      n_row, n_col, cls, 2)
  # members innermost, outer indices reversed; the truth reversed too
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  back = n_outer - 1 - np.arange(n_outer)
  got = engine.crps_bin_sums(_dev(moved), n_row * n_col, n_member, table,
                             _dev(truth[::-1]), back, n_outer, n_row, n_col,
                             cls, 2)
  _assert_same(tuple(x.cpu().numpy() for x in got), want)
  host = cd.host_sums(moved, n_row * n_col, n_member, table,
                      np.ascontiguousarray(truth[::-1]), back, n_outer, n_row,
                      n_col, cls, 2)
  _assert_same(host, want)
  # tables that leave the operands' storage are refused on the host
  with pytest.raises(IndexError, match='member slabs'):
    engine.crps_bin_sums(_dev(moved), n_row * n_col, n_member, table + 1,
                         _dev(truth), None, n_outer, n_row, n_col, cls, 2)
  with pytest.raises(IndexError, match='truth slabs'):
    engine.crps_bin_sums(_dev(ens), ens[0].size, n_member, None,
                         _dev(truth[:2]), None, n_outer, n_row, n_col, cls, 2)
  with pytest.raises(IndexError, match='col_class'):
    engine.crps_bin_sums(_dev(ens), ens[0].size, n_member, None, _dev(truth),
                         None, n_outer, n_row, n_col, cls + 1, 2)
  with pytest.raises(TypeError):
    engine.crps_bin_sums(_dev(ens), ens[0].size, n_member, None,
                         _dev(truth.astype(np.float64)), None, n_outer, n_row,
                         n_col, cls, 2)


def test_fold_equals_the_host_fold():
  rs = np.random.RandomState(2)
  sums = rs.rand(3, 19, 5, 2, 8) * rs.randint(0, 2, size=(3, 19, 5, 1, 1))
  cnt = rs.randint(0, 40, size=(3, 19, 5, 3)).astype(np.int32)
  cols = cnt[..., 2].max(axis=(0, 1)) + 2
  wrow = rs.rand(4, 19) * rs.randint(0, 3, size=(4, 19))  # 0, 1 and 2 times
  mult = rs.randint(0, 3, size=(4, 5)).astype(np.int32)
  assert (mult == 2).any() and (wrow == 0).any()
  got = engine.crps_bin_fold(_dev(sums), _dev(cnt), cols, wrow, mult)
  want = cd.host_fold(sums, cnt, cols, wrow, mult)
  assert tuple(got[0].shape) == (3, 4, 2, 8) == want[0].shape
  assert tuple(got[1].shape) == (3, 4, 4) == want[1].shape
  for a, b in zip(got, want):
    assert a.dtype == torch.float64
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b))
  # the fold written out for one element
  r, o, s = 2, 1, (1, 3)
  acc = 0.0
  for i in range(19):
    t = 0.0
    for c in range(5):
      t = t + float(mult[r, c]) * sums[o, i, c][s]
    acc = acc + wrow[r, i] * t
  assert want[0][o, r][s] == acc
  with pytest.raises(ValueError, match='wrow'):
    engine.crps_bin_fold(_dev(sums), _dev(cnt), cols, wrow[:, :5], mult)


# ---------------------------------------------------------------------------
# operand forms behind the metric
# ---------------------------------------------------------------------------
def _recorded(monkeypatch):
  seen = []
  real = engine.crps_bin_sums

  def spy(ens, *args):
    seen.append((ens, args[2]))
    return real(ens, *args)
  monkeypatch.setattr(engine, 'crps_bin_sums', spy)
  return seen


def test_views_gathers_and_layouts_differ_in_the_tables_alone(monkeypatch):
  rs = np.random.RandomState(0)
  lat, lon = cases.grid(5, 8)
  coords = {'realization': np.arange(3),
            'time': np.array(['2020-01-01', '2020-01-02'], 'datetime64[ns]'),
            'prediction_timedelta': np.arange(6) * np.timedelta64(1, 'D'),
            'latitude': lat, 'longitude': lon}
  full = (np.round(rs.normal(size=(3, 2, 6, 5, 8)) * 4) / 4).astype(np.float32)
  full[1, 0, 2, 3, 4] = full[0, 1, 4, 0, 0] = np.nan
  tru = (np.round(rs.normal(size=(2, 5, 8)) * 4) / 4).astype(np.float32)
  tru[1, 4, 7] = np.nan
  dims = ('realization', 'time', 'prediction_timedelta', 'latitude',
          'longitude')
  regions = {'global': None, 'north': helpers.to_gpu_region(
      helpers.predefined_regions()['northern-hemisphere'])}
  lead = slice(1, 5)
  sub = dict(coords, prediction_timedelta=coords['prediction_timedelta'][lead])
  truth = xl.Dataset({'x': xl.DataArray(_dev(tru), dims[1:2] + dims[3:])},
                     sub)
  metric = cd.CRPSTable()
  seen = _recorded(monkeypatch)

  def run(data, var_dims=dims, tr=truth):
    forecast = xl.Dataset({'x': xl.DataArray(data, var_dims)}, sub)
    return metric.compute_chunk(forecast, tr, skipna=True, regions=regions)

  # the reference: the host path on the same values (a truth without the
  # member and lead dims), then a contiguous device tensor
  host = metric.compute_chunk(
      xl.Dataset({'x': xl.DataArray(full[:, :, lead], dims)}, sub),
      xl.Dataset({'x': xl.DataArray(tru, dims[1:2] + dims[3:])}, sub),
      skipna=True, regions=regions)
  assert not seen
  want = run(_dev(full[:, :, lead]))
  assert seen[-1][0].is_contiguous() and seen[-1][1] is None
  cases.assert_same_dataset(want, host)
  assert want['x'].dims == ('region', 'time', 'prediction_timedelta', 'term',
                            'bin')
  assert np.isfinite(want['x'].values).all()

  # a lead-sliced VIEW of the resident forecast: read where it lies
  view = _dev(full)[:, :, lead]
  assert not view.is_contiguous()
  cases.assert_same_dataset(run(view), want)
  assert seen[-1][0] is view and seen[-1][1] is not None

  # a SlabGather over a shuffled base, members at one stride
  order = np.random.RandomState(1).permutation(2 * 4)
  index = (np.arange(3)[:, None, None] * 8 + order.reshape(2, 4)[None])
  base = np.zeros((24, 5, 8), np.float32)
  base[index.reshape(-1)] = full[:, :, lead].reshape(-1, 5, 8)
  base_dev = _dev(base)
  cases.assert_same_dataset(run(xl.SlabGather(base_dev, index)), want)
  assert seen[-1][0] is base_dev and seen[-1][1] is not None

  # (lon, lat) everywhere: one transposing copy, the same table
  turned = xl.Dataset({'x': xl.DataArray(
      _dev(np.swapaxes(tru, -1, -2)), ('time', 'longitude', 'latitude'))},
                      sub)
  got = run(_dev(np.swapaxes(full[:, :, lead], -1, -2)),
            dims[:3] + ('longitude', 'latitude'), turned)
  cases.assert_same_dataset(got, want)


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', [7, 50])
def test_metric_on_the_device_equals_the_host_path(n_member, dtype, skipna):
  ens, truth = cases.arrays(n_member, 2, 19, 72, dtype,
                            'both' if skipna else 'none')
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = cd.CRPSTable()
  host = metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                              regions=regions)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  dev = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
  cases.assert_same_dataset(dev, host)
  again = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
  cases.assert_same_dataset(again, dev)
  assert np.isfinite(dev[NAME].values).any()
  mean = metric.compute_regions(f_dev, t_dev, regions, skipna)
  cases.assert_same_dataset(
      mean, metric.compute_regions(g(forecast), g(tru), regions, skipna))
  parts = cd.decomposition(dev)[NAME]
  whole = cd.crps(dev)[NAME].values
  np.testing.assert_allclose(
      parts['reliability'].values + parts['potential'].values, whole,
      rtol=1e-12, equal_nan=True)


def test_device_backed_refusals_come_before_any_launch():
  """The refusals of the metric with the variables in HBM, where a launch
  would follow: every one is a ValueError and the launch hook, which sees
  every library call, sees none; a good call right after is seen."""
  from weatherbench2_amd import regions as greg
  ens, truth = cases.arrays(3, 1, 19, 72, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  lat, lon = cases.grid(19, 72)
  metric = cd.CRPSTable()
  lsm = xl.DataArray(np.ones((19, 72)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  many = {f'r{k}': greg.SliceRegion(lon_slice=slice(0, float(lon[k])))
          for k in range(70)}
  big = cases.datasets(*cases.arrays(cd.MAX_MEMBERS + 1, 1, 5, 8, np.float32))
  half = xl.Dataset({NAME: xl.DataArray(f_dev[NAME].data.half(),
                                        f_dev[NAME].dims)}, f_dev.coords)
  whole = xl.Dataset({NAME: xl.DataArray(t_dev[NAME].data.to(torch.int32),
                                         t_dev[NAME].dims)}, t_dev.coords)
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    for call, match in (
        (lambda: metric.compute_chunk(f_dev, t_dev, regions={
            'global': None, 'the-land': greg.LandRegion(lsm)}),
         'the-land.*LandRegion.*2-D'),
        (lambda: metric.compute_chunk(f_dev, t_dev, regions=many), 'classes'),
        (lambda: metric.compute_chunk(_device_dataset(g(big[0])),
                                      _device_dataset(g(big[1]))),
         f'{cd.MAX_MEMBERS + 1} members'),
        (lambda: metric.compute_chunk(half, t_dev), 'float32 and float64'),
        (lambda: metric.compute_chunk(f_dev, whole), 'float32 and float64')):
      with pytest.raises(ValueError, match=match):
        call()
      assert not calls, match
    metric.compute_chunk(f_dev, t_dev)
    assert [c for c in calls if c[1] == 'crps_bin_sums']
  finally:
    engine.set_launch_hook(old)


def test_crps_table_in_the_generic_evaluation_loop():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  regions = cases.product_regions(cases.oracle_regions())
  metric = cd.CRPSTable()
  cfg = config.Eval(metrics={'crps_table': metric}, regions=regions)
  res = xl.as_dataset(evaluation._metric_and_region_loop(
      f_dev, t_dev, cfg, False, compute_chunk=True))
  want = metric.compute_chunk(f_dev, t_dev, regions=regions)
  assert res[NAME].dims == ('metric',) + want[NAME].dims
  np.testing.assert_array_equal(np.asarray(res[NAME].values)[0],
                                want[NAME].values)
