"""Quantile and interval verification on the device (-m gpu): K28
(csrc/quantile_score.hip) against the host path of
weatherbench2_amd/quantile_scores.py, bit for bit, and the counts against the
dense restatement of tests/quantile_score_np.py, at the smallest shapes at
which the kernel can go wrong.  Every table handed to the kernel here is
valid."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import quantile_score_cases as cases
from tests import quantile_score_np as qnp
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import quantile_scores as qs
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
  return np.ascontiguousarray(a).view(np.uint64)


def _both(ens, truth, cls, n_class, levels, method='linear', direct=False,
          restated=True):
  """((device sums, counts, valid), (host ...)) of contiguous [M, O, R, C]
  members and [O, R, C] truth; the host counts are checked against the
  restatement."""
  n_member, n_outer, n_row, n_col = ens.shape
  stride = n_outer * n_row * n_col
  tables = engine.quantile_score_levels(levels, n_member, method, direct)
  args = (None, n_outer, n_row, n_col, cls, n_class, tables, direct)
  host = qs.host_sums(ens, stride, n_member, None, truth, *args)
  dev = engine.quantile_score_sums(_dev(ens), stride, n_member, None,
                                   _dev(truth), *args)
  n_level = len(levels)
  assert dev[0].dtype == torch.float64
  assert dev[1].dtype == dev[2].dtype == torch.int32
  shape = (n_outer, n_row, n_class)
  assert tuple(dev[0].shape) == host[0].shape == shape + (n_level, 2)
  assert tuple(dev[1].shape) == host[1].shape == shape + (n_level, 2)
  assert tuple(dev[2].shape) == host[2].shape == shape + (2,)
  if restated and not direct:
    cnt, valid = qnp.dense_counts(ens, truth, cls, n_class, levels, method)
    np.testing.assert_array_equal(host[1], cnt)
    np.testing.assert_array_equal(host[2], valid)
  return tuple(a.cpu().numpy() for a in dev), host


def _same(dev, host, msg=''):
  np.testing.assert_array_equal(dev[1], host[1], err_msg=msg)
  np.testing.assert_array_equal(dev[2], host[2], err_msg=msg)
  np.testing.assert_array_equal(_bits(dev[0]), _bits(host[0]), err_msg=msg)


def _fold_same(dev, host, n_row, n_class, rs, msg=''):
  wrow = rs.rand(3, n_row) * rs.randint(0, 3, size=(3, n_row))
  mult = rs.randint(0, 3, size=(3, n_class)).astype(np.int32)
  cols = np.zeros(n_class, np.int32)
  got = engine.quantile_score_fold(*[_dev(a) for a in dev], cols, wrow, mult)
  want = qs.host_fold(*host, cols, wrow, mult)
  for a, b in zip(got, want):
    assert a.dtype == torch.float64 and tuple(a.shape) == b.shape
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b),
                                  err_msg=msg)
  n_level = host[0].shape[3]
  assert want[0].shape == (host[0].shape[0], 3, n_level, 2)
  assert want[1].shape == (host[0].shape[0], 3, 2 * n_level + 2)


# a tile tail (7, 30), whole lanes (8, 64), a second and a third tile (68,
# 130); each padded network (2 .. 64) and its successor; each slot step (4, 8,
# 16) and its successor
COLS = (7, 30, 8, 64, 68, 130)
ROWS = (1, 2, 5)
OUTER = (1, 3)
MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
LEVEL_COUNTS = (1, 4, 5, 8, 9, 16)


def level_set(n_level):
  """`n_level` levels, the ends 0 and 1 (lo == hi or t = 0 for every member
  count) and the median among them from three on."""
  if n_level == 1:
    return (0.5,)
  if n_level < 4:
    return tuple(np.linspace(0.0, 1.0, n_level))
  inner = np.linspace(0.03, 0.97, n_level - 2)
  inner[(n_level - 2) // 2] = 0.5
  return (0.0,) + tuple(inner) + (1.0,)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', MEMBERS)
def test_device_sums_counts_and_folds_equal_the_host_path(n_member, dtype):
  b = MEMBERS.index(n_member)
  rs = np.random.RandomState(n_member)
  for a, n_col in enumerate(COLS):
    for s, method in enumerate(cases.METHODS):
      n_row = ROWS[(a + b + s) % 3]
      n_outer = OUTER[(a + b // 2 + s) % 2]
      n_level = LEVEL_COUNTS[(a + b + 2 * s) % 6]
      levels = level_set(n_level)
      # rotated classes (class = column mod n_class) or runs whose first class
      # wraps round the row end, and one more class that no column has
      n_class = min((1, 3)[(a + b) % 2], n_col)
      cls = (cases.rotated, cases.runs)[(a + s) % 2](n_col, n_class)
      n_class += 1
      ens, truth = cases.arrays(
          n_member, n_outer, n_row, n_col, dtype, seed=n_col,
          nan=('both', 'truth', 'member', 'none')[(a + b + s) % 4],
          kind=('normal', 'precip')[(b + s) % 2])
      msg = str((n_col, n_row, n_outer, n_level, method, n_class))
      dev, host = _both(ens, truth, cls, n_class, levels, method)
      _same(dev, host, msg)
      assert not host[2][:, :, n_class - 1].any()
      assert not host[1][:, :, n_class - 1].any()
      assert not dev[0][:, :, n_class - 1].any()
      assert not np.signbit(dev[0][dev[0] == 0]).any()
      assert host[2][..., 0].any()
      _fold_same(dev, host, n_row, n_class, rs, msg)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_every_level_count_in_both_modes(dtype):
  # direct mode: the quantile forecasts are the members, in storage order
  # (here NOT sorted: nothing may sort them); every slot step and successor
  for k, n_level in enumerate(LEVEL_COUNTS):
    for n_col in (34, 130):
      levels = level_set(n_level)
      q, truth = cases.arrays(n_level, 2, 5, n_col, dtype, seed=k,
                              nan=('both', 'none')[k % 2], kind='precip')
      cls = cases.runs(n_col, 3)
      dev, host = _both(q, truth, cls, 3, levels, direct=True)
      _same(dev, host, str((n_level, n_col)))
      assert host[2][..., 0].sum() > 0 and host[1][..., 1].sum() > 0
      # the forecast-quantile sums are the plain chains over the slabs
      if k % 2:
        want = np.zeros(host[0].shape[:-1])
        for j in range(n_col):
          want[:, :, cls[j]] += np.moveaxis(q[..., j].astype(np.float64), 0, -1)
        np.testing.assert_array_equal(_bits(host[0][..., 1]), _bits(want))
      # ensemble mode at the same level count
      ens, _ = cases.arrays(9, 2, 5, n_col, dtype, seed=k)
      both = _both(ens, truth, cls, 3, levels, 'hazen')
      _same(*both, str((n_level, n_col, 'ensemble')))
  # more than 16 levels: further launches, the same bits
  levels = tuple(np.linspace(0.01, 0.99, 37))
  ens, truth = cases.arrays(17, 1, 2, 68, dtype, nan='member', seed=3)
  _same(*_both(ens, truth, cases.runs(68, 3), 3, levels, 'weibull'))


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_classes_nan_cases_and_two_runs(dtype):
  levels = cases.LEVELS
  n_col = 130
  ens, truth = cases.arrays(7, 2, 3, n_col, dtype, nan='both', seed=1,
                            kind='precip')
  # a single class; runs; a class met again after another; a change on a tile
  # border (column 64) and on the second one (128)
  single = np.zeros(n_col, np.int32)
  border = (np.arange(n_col) // 64).astype(np.int32)
  again = ((np.arange(n_col) // 10) % 3).astype(np.int32)
  for cls, n_class in ((single, 1), (cases.runs(n_col, 4), 4), (border, 3),
                       (again, 3), (np.arange(n_col, dtype=np.int32) % 64, 64)):
    dev, host = _both(ens, truth, cls, n_class, levels)
    _same(dev, host, str(cls[:12]))
    rerun, _ = _both(ens, truth, cls, n_class, levels, restated=False)
    _same(rerun, dev)  # two runs of the same launch
  # a whole class without a valid point: sums +0.0, every count invalid
  cls = cases.runs(n_col, 4)
  blank = cases.blank_class(truth, cls, 2)
  dev, host = _both(ens, blank, cls, 4, levels)
  _same(dev, host)
  assert (_bits(dev[0][:, :, 2]) == 0).all() and not dev[1][:, :, 2].any()
  assert not dev[2][:, :, 2, 0].any()
  assert (dev[2][:, :, 2, 1] == (cls == 2).sum()).all()
  # NaN in the truth alone, in one member alone (the last: behind the sort)
  for where in ('truth', 'member'):
    e, y = cases.arrays(5, 1, 2, 68, dtype, seed=2)
    if where == 'truth':
      y[0, 1, 65] = np.nan
    else:
      e[4, 0, 1, 65] = np.nan
    dev, host = _both(e, y, cases.runs(68, 2), 2, levels)
    _same(dev, host)
    assert dev[2][..., 1].sum() == 1
  # the 13 evaluation regions' classes on 72 columns (`europe` wraps)
  lat, lon = cases.grid(19, 72)
  cls, mult, _ = events.column_classes(
      cases.product_regions(cases.oracle_regions()), lat, lon)
  ens, truth = cases.arrays(5, 1, 9, 72, dtype, nan='truth', seed=2)
  _same(*_both(ens, truth, cls, mult.shape[1], levels))
  assert mult.shape[1] > 3


def test_sums_walk_the_slab_tables_and_a_misaligned_base():
  n_member, n_outer, n_row, n_col = 3, 4, 5, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32,
                            nan='both', seed=5)
  cls = cases.rotated(n_col, 2)
  slab = n_row * n_col
  tables = engine.quantile_score_levels(cases.LEVELS, n_member)
  tail = (n_outer, n_row, n_col, cls, 2, tables)
  want = qs.host_sums(ens, ens[0].size, n_member, None, truth, None, *tail)

  def same(got):
    _same(tuple(a.cpu().numpy() for a in got), want)
  # members innermost (member_stride = one slab, not the members' extent),
  # outer indices reversed (a permuted slab table); the truth reversed too
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  back = n_outer - 1 - np.arange(n_outer)
  same(engine.quantile_score_sums(_dev(moved), slab, n_member, table,
                                  _dev(truth[::-1]), back, *tail))
  _same(qs.host_sums(moved, slab, n_member, table,
                     np.ascontiguousarray(truth[::-1]), back, *tail), want)
  # a base one element off a 16-byte border: the same bits
  for shift_ens, shift_truth in ((1, 0), (0, 1), (3, 3)):
    e = torch.zeros(ens.size + 4, dtype=torch.float32, device='cuda')
    y = torch.zeros(truth.size + 4, dtype=torch.float32, device='cuda')
    ev = e[shift_ens:shift_ens + ens.size]
    yv = y[shift_truth:shift_truth + truth.size]
    ev.copy_(_dev(ens).reshape(-1))
    yv.copy_(_dev(truth).reshape(-1))
    same(engine.quantile_score_sums(ev, ens[0].size, n_member, None, yv, None,
                                    *tail))


def test_geometry_and_the_out_of_range_calls_launch_nothing():
  """The limits as the engine reports them, and calls beyond them through the
  engine, with operands that are large enough for what each call names: a
  refusal that failed would run in bounds and fail the test, not fault.  (The
  C entry point's own refusals are tested without a device in
  tests/test_quantile_score_cpu.py.)"""
  from weatherbench2_amd import _lib
  geo = engine.quantile_score_geometry(torch.float32, 50, 13, 16)
  assert (geo['min_member'], geo['max_member'], geo['max_levels']) == (1, 64,
                                                                       16)
  assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
  assert geo['lds_bytes'] == max(50 * 64 * 4, 64 * 33 * 8) + 256
  for wrong in (dict(n_member=65), dict(n_class=65), dict(n_level=17),
                dict(n_member=0), dict(n_level=0)):
    with pytest.raises(_lib.Wb2HipError):
      engine.quantile_score_geometry(torch.float32, **wrong)
  n_member, n_row, n_col = 65, 2, 68
  ens, truth = cases.arrays(n_member, 1, n_row, n_col, np.float32)
  e, y = _dev(ens), _dev(truth)
  stride = n_row * n_col
  cls = np.zeros(n_col, np.int32)
  good = engine.quantile_score_levels((0.5,), 5)
  lo17 = np.arange(17, dtype=np.int32)
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def sums(n_member=5, n_class=1, tables=good, direct=False):
    return engine.quantile_score_sums(e, stride, n_member, None, y, None, 1,
                                      n_row, n_col, cls, n_class, tables,
                                      direct)
  try:
    for levels, members, direct in ((np.linspace(0, 1, 65), 5, False),
                                    (np.linspace(0, 1, 17), 17, True)):
      with pytest.raises(ValueError, match='levels'):
        engine.quantile_score_levels(levels, members, 'linear', direct)
    with pytest.raises(ValueError, match='65 members'):
      sums(n_member=65)
    with pytest.raises(ValueError, match='0 members'):
      sums(n_member=0)
    with pytest.raises(ValueError, match='17 levels.*1 to 16'):
      sums(n_member=17, direct=True,
           tables=(lo17, lo17, np.zeros(17), np.linspace(0, 1, 17),
                   1 - np.linspace(0, 1, 17)))
    with pytest.raises(ValueError, match='hi < n_member'):
      sums(tables=(np.array([4]), np.array([5]), np.zeros(1), np.array([0.5]),
                   np.array([0.5])))
    with pytest.raises(ValueError, match='lo == hi'):
      sums(direct=True)
    with pytest.raises(_lib.Wb2HipError, match='n_class='):
      sums(n_class=65)
    assert not calls
    sums()
    assert [c for c in calls if c[1] == 'quantile_score_sums']
  finally:
    engine.set_launch_hook(old)


# ---------------------------------------------------------------------------
# the metric on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('grid', cases.GRIDS,
                         ids=lambda v: 'x'.join(map(str, v)))
def test_device_table_equals_the_host_table(grid):
  """The full `compute_chunk` with the 13 evaluation regions (and two more)
  and without regions, both skipna, two runs."""
  a = cases.GRIDS.index(grid)
  regions = cases.product_regions(cases.oracle_regions())
  for b, n_member in enumerate((1, 2, 7)):
    dtype = cases.DTYPES[(a + b) % 2]
    method = cases.METHODS[(a + b) % 3]
    ens, truth = cases.arrays(n_member, 2, *grid, dtype,
                              nan=('both', 'none', 'truth')[b], seed=a,
                              kind=('precip', 'normal')[(a + b) % 2])
    forecast, tru = cases.datasets(ens, truth)
    metric = qs.QuantileScoreTable(cases.LEVELS, method=method)
    f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
    for skipna in (False, True):
      for kwargs in (dict(regions=regions), dict()):
        host = metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                    **kwargs)
        dev = metric.compute_chunk(f_dev, t_dev, skipna=skipna, **kwargs)
        cases.assert_same_dataset(dev, host)
        again = metric.compute_chunk(f_dev, t_dev, skipna=skipna, **kwargs)
        cases.assert_same_dataset(again, dev)  # two runs
      assert host[NAME].dims == ('time', cases.TERM, cases.LEVEL)
      assert dev.attrs == {'ensemble_size': n_member, 'method': method,
                           'levels': cases.LEVELS}
    assert np.isfinite(dev[NAME].values).any()
  # direct mode: quantile forecasts along their own dim
  levels = (0.1, 0.5, 0.9)
  q, truth = cases.arrays(3, 2, *grid, np.float32, nan='both', seed=a)
  q = np.sort(q, axis=0)  # (NaN last: the point is invalid all the same)
  qf, qt = cases.quantile_datasets(q, truth, levels)
  metric = qs.QuantileScoreTable(None, quantile_dim=cases.QDIM)
  host = metric.compute_chunk(g(qf), g(qt), skipna=True, regions=regions)
  dev = metric.compute_chunk(_device_dataset(g(qf)), _device_dataset(g(qt)),
                             skipna=True, regions=regions)
  cases.assert_same_dataset(dev, host)
  assert dev.attrs['levels'] == levels


def _recorded(monkeypatch):
  seen = []
  real = engine.quantile_score_sums

  def spy(ens, *args, **kwargs):
    seen.append((ens, args[2], args[4]))
    return real(ens, *args, **kwargs)
  monkeypatch.setattr(engine, 'quantile_score_sums', spy)
  return seen


def test_views_gathers_and_layouts_differ_in_the_tables_alone(monkeypatch):
  rs = np.random.RandomState(0)
  lat, lon = cases.grid(5, 8)
  coords = {'realization': np.arange(3),
            'time': np.array(['2020-01-01', '2020-01-02'], 'datetime64[ns]'),
            'prediction_timedelta': np.arange(6) * np.timedelta64(1, 'D'),
            'latitude': lat, 'longitude': lon}
  full = np.round(rs.normal(size=(3, 2, 6, 5, 8)) * 2, 1).astype(np.float32)
  full[1, 0, 2, 3, 4] = full[0, 1, 4, 0, 0] = np.nan
  tru = np.round(rs.normal(size=(2, 5, 8)) * 2, 1).astype(np.float32)
  tru[1, 4, 7] = np.nan
  dims = ('realization', 'time', 'prediction_timedelta', 'latitude',
          'longitude')
  regions = {'global': None, 'north': helpers.to_gpu_region(
      helpers.predefined_regions()['northern-hemisphere'])}
  lead = slice(1, 5)
  sub = dict(coords, prediction_timedelta=coords['prediction_timedelta'][lead])
  # a truth without the lead dim
  truth = xl.Dataset({'x': xl.DataArray(_dev(tru), dims[1:2] + dims[3:])},
                     sub)
  metric = qs.QuantileScoreTable(cases.LEVELS, method='hazen')
  seen = _recorded(monkeypatch)

  def run(data, var_dims=dims, tr=truth):
    forecast = xl.Dataset({'x': xl.DataArray(data, var_dims)}, sub)
    return metric.compute_chunk(forecast, tr, skipna=True, regions=regions)

  # the reference: the host path on the same values, then a contiguous device
  # tensor
  host = metric.compute_chunk(
      xl.Dataset({'x': xl.DataArray(full[:, :, lead], dims)}, sub),
      xl.Dataset({'x': xl.DataArray(tru, dims[1:2] + dims[3:])}, sub),
      skipna=True, regions=regions)
  assert not seen
  want = run(_dev(full[:, :, lead]))
  assert seen[-1][0].is_contiguous() and seen[-1][1] is None
  # the truth is one slab per time, read through a table
  assert seen[-1][2] is not None
  cases.assert_same_dataset(want, host)
  assert want['x'].dims == ('region', 'time', 'prediction_timedelta',
                            cases.TERM, cases.LEVEL)
  assert np.isfinite(want['x'].values).all()

  # a lead-sliced VIEW of the resident forecast: read where it lies
  view = _dev(full)[:, :, lead]
  assert not view.is_contiguous()
  cases.assert_same_dataset(run(view), want)
  assert seen[-1][0] is view and seen[-1][1] is not None

  # a permuted outer order (lead before time): the same table
  turned = _dev(np.ascontiguousarray(np.swapaxes(full[:, :, lead], 1, 2)))
  got = run(turned, (dims[0], dims[2], dims[1]) + dims[3:])
  cases.assert_same_dataset(got, want)

  # a SlabGather over a shuffled base, members at one stride
  order = np.random.RandomState(1).permutation(2 * 4)
  index = (np.arange(3)[:, None, None] * 8 + order.reshape(2, 4)[None])
  base = np.zeros((24, 5, 8), np.float32)
  base[index.reshape(-1)] = full[:, :, lead].reshape(-1, 5, 8)
  base_dev = _dev(base)
  cases.assert_same_dataset(run(xl.SlabGather(base_dev, index)), want)
  assert seen[-1][0] is base_dev and seen[-1][1] is not None

  # (lon, lat) everywhere: one transposing copy each, the same table
  turned = xl.Dataset({'x': xl.DataArray(
      _dev(np.swapaxes(tru, -1, -2)), ('time', 'longitude', 'latitude'))},
                      sub)
  got = run(_dev(np.swapaxes(full[:, :, lead], -1, -2)),
            dims[:3] + ('longitude', 'latitude'), turned)
  cases.assert_same_dataset(got, want)


def test_device_backed_refusals_come_before_any_launch():
  """The refusals of the metric with the variables in HBM, where a launch
  would follow: every one is a ValueError and the launch hook, which sees
  every library call, sees none; a good call right after is seen."""
  from weatherbench2_amd import regions as greg
  ens, truth = cases.arrays(3, 1, 19, 72, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  lat, lon = cases.grid(19, 72)
  metric = qs.QuantileScoreTable()
  lsm = xl.DataArray(np.ones((19, 72)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  many = {f'r{k}': greg.SliceRegion(lon_slice=slice(0, float(lon[k])))
          for k in range(70)}
  big = cases.datasets(*cases.arrays(qs.MAX_MEMBERS + 1, 1, 5, 72,
                                     np.float32))
  half = xl.Dataset({NAME: xl.DataArray(f_dev[NAME].data.half(),
                                        f_dev[NAME].dims)}, f_dev.coords)
  q17 = np.sort(cases.arrays(17, 1, 5, 72, np.float32)[0], axis=0)
  qf, qt = cases.quantile_datasets(q17, truth[:, :5], np.linspace(0.1, 0.9,
                                                                   17))
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
         f'{qs.MAX_MEMBERS + 1} members'),
        (lambda: metric.compute_chunk(half, t_dev), 'float32 and float64'),
        (lambda: qs.QuantileScoreTable(None, quantile_dim=cases.QDIM
                                       ).compute_chunk(
            _device_dataset(g(qf)), _device_dataset(g(qt))), '17 levels')):
      with pytest.raises(ValueError, match=match):
        call()
      assert not calls, match
    metric.compute_chunk(f_dev, t_dev)
    assert [c for c in calls if c[1] == 'quantile_score_sums']
    assert [c for c in calls if c[1] == 'crps_bin_fold']
    assert [c for c in calls if c[1] == 'event_fold']
  finally:
    engine.set_launch_hook(old)


def test_pooled_bootstrap_and_the_evaluation_loop_on_the_device():
  from weatherbench2_amd import config, evaluation, pooling
  ens, truth = cases.arrays(5, 6, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  regions = cases.product_regions(cases.oracle_regions())
  metric = qs.QuantileScoreTable(cases.LEVELS, method='weibull')
  cfg = config.Eval(metrics={'quantile_score': metric}, regions=regions)
  res = xl.as_dataset(evaluation._metric_and_region_loop(
      f_dev, t_dev, cfg, False, compute_chunk=True))
  want = metric.compute_chunk(f_dev, t_dev, regions=regions)
  assert res[NAME].dims == ('metric',) + want[NAME].dims
  np.testing.assert_array_equal(np.asarray(res[NAME].values)[0],
                                want[NAME].values)
  host = metric.compute_chunk(g(forecast), g(tru), regions=regions)
  cases.assert_same_dataset(want, host)
  mean = metric.compute_regions(f_dev, t_dev, regions, True)
  cases.assert_same_dataset(
      mean, metric.compute_regions(g(forecast), g(tru), regions, True))
  pooled = pooling.Pooled(metric, neighborhoods=(1, 3))
  dev = pooled.compute_chunk_regions(f_dev, t_dev, regions, True)
  assert dev[NAME].dims == ('neighborhood',) + want[NAME].dims
  cases.assert_same_dataset(
      dev, pooled.compute_chunk_regions(g(forecast), g(tru), regions, True))
  tables = metric.compute_chunk(f_dev, t_dev, skipna=True)
  kwargs = dict(n_replicate=25, block_length=2, seed=2)
  out = bs.bootstrap(_device_dataset(tables), qs.interval_score, **kwargs)
  cases.assert_same_dataset(
      out, bs.bootstrap(tables, qs.interval_score, **kwargs))
  assert np.isfinite(np.asarray(out[NAME].values)).all()
