"""Distributions-oriented verification on the device (-m gpu): K26
(csrc/joint_counts.hip) against the host path of
weatherbench2_amd/distribution.py, bit for bit, and against the dense
restatement of tests/joint_np.py for the counts, at the smallest shapes at
which the kernel can go wrong.  Every table handed to the kernel here is
valid."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import joint_cases as cases
from tests import joint_np as jnp_
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import distribution as dist
from weatherbench2_amd import engine
from weatherbench2_amd import events
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


def _both(ens, truth, cls, n_class, given, side, restated=True):
  """(device counts, host counts) of contiguous [M, O, R, C] members and [O,
  R, C] truth; the host counts are checked against the restatement."""
  n_member, n_outer, n_row, n_col = ens.shape
  stride = n_outer * n_row * n_col
  args = (None, n_outer, n_row, n_col, cls, n_class, given, side)
  host = dist.host_counts(ens, stride, n_member, None, truth, *args)
  dev = engine.joint_counts(_dev(ens), stride, n_member, None, _dev(truth),
                            *args)
  n_code = (len(given) + 1) ** 2 + 1
  assert dev.dtype == torch.int32
  assert tuple(dev.shape) == host.shape == (n_outer, n_row, n_class, n_code)
  if restated:
    np.testing.assert_array_equal(
        host, jnp_.dense_counts(ens, truth, cls, n_class, given, side))
  return dev.cpu().numpy(), host


# one element per access with tails (7, 30); whole 16-byte lanes of both
# dtypes (8, 64, 68); the row-group tail (rows_per_group is 4, 2 or 1); the
# tail of four members ahead (5), more than one round (8, 33)
COLS = (7, 30, 8, 64, 68)
ROWS = (1, 4, 5, 9)
OUTER = (1, 3)
MEMBERS = (1, 2, 5, 8, 33)
EDGES = (0, 1, 7, 8, 31)    # 7 | 8: the last of one instantiation, 8 | 12 ..
CLASSES = (1, 3)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', MEMBERS)
def test_device_counts_and_fold_equal_the_host_path(n_member, dtype):
  b = MEMBERS.index(n_member)
  rs = np.random.RandomState(n_member)
  some = False
  for a, n_col in enumerate(COLS):
    for side in cases.SIDES:
      s = cases.SIDES.index(side)
      n_row = ROWS[(a + b + s) % 4]
      n_outer = OUTER[(a + b // 2 + s) % 2]
      n_edge = EDGES[(a + b + 2 * s) % 5]
      given = cases.edges(n_edge)
      # rotated classes (class = column mod n_class) and one more that no
      # column has
      n_class = min(CLASSES[(a + b) % 2], n_col)
      cls = cases.rotated(n_col, n_class)
      n_class += 1
      ens, truth = cases.planted(n_member, n_outer, n_row, n_col, dtype, given,
                                 seed=n_col)
      msg = str((n_col, n_row, n_outer, n_edge, side, n_class))
      dev, host = _both(ens, truth, cls, n_class, given, side)
      np.testing.assert_array_equal(dev, host, err_msg=msg)
      assert not host[:, :, n_class - 1].any()
      assert host[..., -1].any() and host[..., :-1].any()
      some = some or (n_edge > 0 and host[..., 1:-1].any())
      # the fold: wb2_event_fold with n_code = B * B + 1
      wrow = rs.rand(3, n_row) * rs.randint(0, 3, size=(3, n_row))
      mult = rs.randint(0, 3, size=(3, n_class)).astype(np.int32)
      got = engine.joint_fold(_dev(dev), wrow, mult)
      want = dist.host_fold(host, wrow, mult)
      assert got.dtype == torch.float64
      assert tuple(got.shape) == want.shape == (n_outer, 3, host.shape[-1])
      np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64),
                                    want.view(np.uint64), err_msg=msg)
  assert some


@pytest.mark.parametrize('side', cases.SIDES)
def test_every_edge_count_on_both_dtypes_and_lane_widths(side):
  # the (E, dtype, width) triples the walk above does not meet with this side
  for k, n_edge in enumerate(EDGES + (12, 16, 24)):
    given = cases.edges(n_edge)
    for dtype in cases.DTYPES:
      for n_col in (30, 68):
        n_member = (2, 5, 8)[(k + (dtype is np.float64)) % 3]
        ens, truth = cases.planted(n_member, 1, 5, n_col, dtype, given, seed=k)
        dev, host = _both(ens, truth, cases.rotated(n_col, 3), 3, given, side)
        np.testing.assert_array_equal(dev, host,
                                      err_msg=str((n_edge, dtype, n_col)))
        assert host[..., :-1].sum() > 0


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_saturated_counter_many_classes_and_two_runs(dtype):
  # 128 members, every one in ONE category per point: a packed counter holds
  # 128 = 0x80 for every edge below that category
  n_col = 68
  given = cases.edges(8)
  rs = np.random.RandomState(0)
  truth = (np.round(rs.normal(size=(1, 5, n_col)) * 4) / 4).astype(dtype)
  level = (np.round(rs.normal(size=(1, 5, n_col)) * 4) / 4).astype(dtype)
  ens = np.broadcast_to(level, (128,) + level.shape).copy()
  ens[:, 0, 0, :9] = np.array(given + (9.0,), dtype)   # each category once
  ens[:, 0, 1, 0] = np.inf
  ens[:, 0, 1, 1] = -np.inf
  truth[0, 2, 5] = np.nan
  ens[127, 0, 3, 67] = np.nan                          # the LAST member
  for side in cases.SIDES:
    dev, host = _both(ens, truth, cases.rotated(n_col, 3), 3, given, side)
    np.testing.assert_array_equal(dev, host)
    assert (host[..., :-1] % 128 == 0).all() and host[..., :-1].any()
    assert host[..., -1].sum() == 2
    again, _ = _both(ens, truth, cases.rotated(n_col, 3), 3, given, side,
                     restated=False)
    np.testing.assert_array_equal(again, dev)  # two runs of the same launch
  # 64 classes with one edge (every column of 64 a class of its own), the 13
  # evaluation regions' classes on 72 columns
  ens, truth = cases.planted(5, 2, 5, 64, dtype, (0.0,), seed=1)
  dev, host = _both(ens, truth, np.arange(64, dtype=np.int32), 64, (0.0,),
                    'right')
  np.testing.assert_array_equal(dev, host)
  lat, lon = cases.grid(19, 72)
  cls, mult, _ = events.column_classes(
      cases.product_regions(cases.oracle_regions()), lat, lon)
  ens, truth = cases.planted(5, 1, 9, 72, dtype, given, seed=2)
  dev, host = _both(ens, truth, cls, mult.shape[1], given, 'left')
  np.testing.assert_array_equal(dev, host)
  assert mult.shape[1] > 3


def test_counts_walk_the_slab_tables_and_a_misaligned_base():
  n_member, n_outer, n_row, n_col = 3, 4, 5, 8
  given = cases.edges(7)
  ens, truth = cases.planted(n_member, n_outer, n_row, n_col, np.float32,
                             given, seed=5)
  cls = cases.rotated(n_col, 2)
  slab = n_row * n_col
  tail = (n_outer, n_row, n_col, cls, 2, given, 'right')
  want = dist.host_counts(ens, ens[0].size, n_member, None, truth, None, *tail)
  # members innermost (member_stride = one slab, not the members' extent),
  # outer indices reversed (a permuted slab table); the truth reversed too
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  back = n_outer - 1 - np.arange(n_outer)
  got = engine.joint_counts(_dev(moved), slab, n_member, table,
                            _dev(truth[::-1]), back, *tail)
  np.testing.assert_array_equal(got.cpu().numpy(), want)
  host = dist.host_counts(moved, slab, n_member, table,
                          np.ascontiguousarray(truth[::-1]), back, *tail)
  np.testing.assert_array_equal(host, want)
  # one truth slab for every outer index, through a table of zeros
  zero = np.zeros(n_outer, np.int64)
  want1 = dist.host_counts(ens, ens[0].size, n_member, None,
                           np.broadcast_to(truth[1], truth.shape).copy(), None,
                           *tail)
  got = engine.joint_counts(_dev(ens), ens[0].size, n_member, None,
                            _dev(truth[1]), zero, *tail)
  np.testing.assert_array_equal(got.cpu().numpy(), want1)
  # a base one element off a 16-byte border: whole lanes by n_col and
  # member_stride, yet one element per access; the same integers
  for shift_ens, shift_truth in ((1, 0), (0, 1), (3, 3)):
    e = torch.zeros(ens.size + 4, dtype=torch.float32, device='cuda')
    y = torch.zeros(truth.size + 4, dtype=torch.float32, device='cuda')
    ev = e[shift_ens:shift_ens + ens.size]
    yv = y[shift_truth:shift_truth + truth.size]
    ev.copy_(_dev(ens).reshape(-1))
    yv.copy_(_dev(truth).reshape(-1))
    assert (ev.data_ptr() % 16 != 0) or (yv.data_ptr() % 16 != 0)
    got = engine.joint_counts(ev, ens[0].size, n_member, None, yv, None, *tail)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
  # tables that leave the operands' storage are refused on the host
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    with pytest.raises(IndexError, match='member slabs'):
      engine.joint_counts(_dev(moved), slab, n_member, table + 1, _dev(truth),
                          None, *tail)
    with pytest.raises(IndexError, match='truth slabs'):
      engine.joint_counts(_dev(ens), ens[0].size, n_member, None,
                          _dev(truth[:2]), None, *tail)
    with pytest.raises(IndexError, match='col_class'):
      engine.joint_counts(_dev(ens), ens[0].size, n_member, None, _dev(truth),
                          None, n_outer, n_row, n_col, cls + 1, 2, given,
                          'right')
    assert not calls
  finally:
    engine.set_launch_hook(old)


def test_the_out_of_range_calls_launch_nothing():
  from weatherbench2_amd import _lib
  ens, truth = cases.arrays(5, 1, 2, 68, np.float32, 'both')
  h = _lib.load()
  out = torch.full((2, 64, 5), 7, dtype=torch.int32, device='cuda')
  e, y = _dev(ens), _dev(truth)
  col = _dev(np.zeros(68, np.int32))
  edge = _dev(np.zeros(1))
  for n_member, n_class, n_edge, side, words in (
      (129, 1, 1, 0, b'n_member='), (0, 1, 1, 0, b'n_member='),
      (3, 65, 1, 0, b'n_class='), (3, 0, 1, 0, b'n_class='),
      (3, 1, 32, 0, b'n_edge='), (3, 1, -1, 0, b'n_edge='),
      (3, 1, 1, 2, b'side='), (3, 64, 31, 0, b'LDS budget')):
    rc = h.wb2_joint_counts(
        _lib.WB2_F32, _lib.ptr(e), None, _lib.ptr(y), None, n_member, 136, 1,
        2, 68, _lib.ptr(col), n_class, _lib.ptr(edge), n_edge, side,
        _lib.ptr(out), None)
    assert rc < 0 and words in h.wb2_last_error()
  torch.cuda.synchronize()
  assert (out == 7).all()


# ---------------------------------------------------------------------------
# the metric on the device
# ---------------------------------------------------------------------------
GRIDS = ((2, 7), (5, 30), (4, 64), (9, 68), (19, 72))


@pytest.mark.parametrize('grid', GRIDS, ids=lambda v: 'x'.join(map(str, v)))
def test_device_table_equals_the_host_table(grid):
  """The full `compute_chunk` with the 13 evaluation regions (and two more),
  both skipna, two runs."""
  a = GRIDS.index(grid)
  regions = cases.product_regions(cases.oracle_regions())
  for b, n_member in enumerate((1, 2, 5, 8, 33, 128)[a % 2::2]):
    dtype = cases.DTYPES[(a + b) % 2]
    nan = cases.NANS[(a + b) % 4]
    side = cases.SIDES[(a + b) % 2]
    n_edge = EDGES[(a + 2 * b) % 5]
    given = cases.edges(n_edge)
    ens, truth = cases.planted(n_member, 2, *grid, dtype, given,
                               nan=nan != 'none', seed=a)
    forecast, tru = cases.datasets(ens, truth)
    metric = dist.JointTable(given, side=side)
    f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
    for skipna in (False, True):
      host = metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                  regions=regions)
      dev = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
      cases.assert_same_dataset(dev, host)
      again = metric.compute_chunk(f_dev, t_dev, skipna=skipna,
                                   regions=regions)
      cases.assert_same_dataset(again, dev)  # two runs
      assert dev[NAME].dims == ('region', 'time', cases.TRUTH_BIN,
                                cases.FORECAST_BIN)
      assert dev.attrs == {'ensemble_size': n_member, 'bin_edges': given,
                           'side': side}
    assert np.isfinite(dev[NAME].values).any()


def _recorded(monkeypatch):
  seen = []
  real = engine.joint_counts

  def spy(ens, *args, **kwargs):
    seen.append((ens, args[2], args[4]))
    return real(ens, *args, **kwargs)
  monkeypatch.setattr(engine, 'joint_counts', spy)
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
  # a truth without the lead dim
  truth = xl.Dataset({'x': xl.DataArray(_dev(tru), dims[1:2] + dims[3:])},
                     sub)
  metric = dist.JointTable((-0.5, 0.0, 0.5), side='left')
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
                            cases.TRUTH_BIN, cases.FORECAST_BIN)
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
  metric = dist.JointTable((-0.5, 0.5))
  lsm = xl.DataArray(np.ones((19, 72)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  many = {f'r{k}': greg.SliceRegion(lon_slice=slice(0, float(lon[k])))
          for k in range(70)}
  big = cases.datasets(*cases.arrays(dist.MAX_MEMBERS + 1, 1, 5, 8,
                                     np.float32))
  half = xl.Dataset({NAME: xl.DataArray(f_dev[NAME].data.half(),
                                        f_dev[NAME].dims)}, f_dev.coords)
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
         f'{dist.MAX_MEMBERS + 1} members'),
        (lambda: dist.JointTable({'other': (1.0,)}).compute_chunk(
            f_dev, t_dev), 'no entry'),
        (lambda: metric.compute_chunk(half, t_dev), 'float32 and float64')):
      with pytest.raises(ValueError, match=match):
        call()
      assert not calls, match
    metric.compute_chunk(f_dev, t_dev)
    assert [c for c in calls if c[1] == 'joint_counts']
    assert [c for c in calls if c[1] == 'event_fold']
  finally:
    engine.set_launch_hook(old)


def test_pooled_bootstrap_and_the_evaluation_loop_on_the_device():
  from weatherbench2_amd import config, evaluation, pooling
  ens, truth = cases.arrays(5, 6, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  regions = cases.product_regions(cases.oracle_regions())
  metric = dist.JointTable(cases.edges(7))
  # config.Eval with regions=
  cfg = config.Eval(metrics={'joint': metric}, regions=regions)
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
  # Pooled at windows (1, 3): window 1 is the plain table, both equal the host
  pooled = pooling.Pooled(metric, neighborhoods=(1, 3))
  dev = pooled.compute_chunk_regions(f_dev, t_dev, regions, True)
  assert dev[NAME].dims == ('neighborhood',) + want[NAME].dims
  cases.assert_same_dataset(
      dev, pooled.compute_chunk_regions(g(forecast), g(tru), regions, True))
  plain = metric.compute_chunk_regions(f_dev, t_dev, regions, True)
  np.testing.assert_array_equal(
      np.asarray(dev[NAME].values)[0].view(np.uint64),
      np.asarray(plain[NAME].values).view(np.uint64))
  # bootstrap with a device table
  tables = metric.compute_chunk(f_dev, t_dev, skipna=True)
  kwargs = dict(n_replicate=25, block_length=2, seed=2)
  out = bs.bootstrap(_device_dataset(tables), dist.heidke, **kwargs)
  cases.assert_same_dataset(out, bs.bootstrap(tables, dist.heidke, **kwargs))
  assert np.isfinite(np.asarray(out[NAME].values)).all()
