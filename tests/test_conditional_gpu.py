"""Conditional verification on the device (-m gpu): K24
(csrc/conditional_sums.hip) against the host path of
weatherbench2_amd/conditional.py, bit for bit, at the smallest shapes at which
the kernel can go wrong.  Every table handed to the kernel here is valid."""
import numpy as np
import pytest
import torch

from tests import conditional_cases as cases
from tests import helpers
from weatherbench2_amd import conditional as cond
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


def _both(ens, truth, cls, n_class, by, n_bin):
  """((device sums, counts), (host sums, counts)) of contiguous [M, O, R, C]
  members and [O, R, C] truth."""
  n_member, n_outer, n_row, n_col = ens.shape
  stride = n_outer * n_row * n_col
  edges = cases.kernel_edges(by, n_bin)
  args = (None, n_outer, n_row, n_col, cls, n_class, by, edges)
  host = cond.host_sums(ens, stride, n_member, None, truth, *args)
  dev = engine.conditional_sums(_dev(ens), stride, n_member, None, _dev(truth),
                                *args)
  assert dev[0].dtype == torch.float64 and dev[1].dtype == torch.int32
  assert tuple(dev[0].shape) == host[0].shape == (
      n_outer, n_row, n_class, n_bin, 4)
  assert tuple(dev[1].shape) == host[1].shape == (
      n_outer, n_row, n_class, n_bin)
  return tuple(x.cpu().numpy() for x in dev), host


def _assert_same(dev, host, msg=''):
  np.testing.assert_array_equal(_bits(dev[0]), _bits(host[0]), err_msg=msg)
  np.testing.assert_array_equal(dev[1], host[1], err_msg=msg)


# below, at and above one wave = the column tile (one, two and three tiles of
# a row, with and without a partial last one); one row and several (a wave, a
# workgroup of its own, per row); one outer index and several
COLS = (1, 63, 64, 65, 129)
ROWS = (1, 3)
OUTER = (1, 3)
# every padded register count (2, 4, 8, 16, 32, 64) but 8 from its upper end,
# 32 and 64 from inside too
MEMBERS = (1, 2, 3, 17, 50, 64)
CLASSES = (1, 3, 10, 64)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', MEMBERS)
def test_device_sums_and_fold_equal_the_host_path(n_member, dtype):
  b = MEMBERS.index(n_member)
  rs = np.random.RandomState(n_member)
  some = False
  for a, n_col in enumerate(COLS):
    n_row = ROWS[(a + b) % 2]
    n_outer = OUTER[(a + b // 2) % 2]
    n_bin = cases.BINS[(a + b) % 5]
    nan = cases.NANS[(a + 2 * b) % 4]
    by = cases.BYS[(a + b) % 3]
    if n_member == 1 and by == 'spread':
      by = 'truth'  # (the kernel would take it: s2 = +0.0 for every point)
    # runs of columns with a wrapped first class, borders inside a tile, and
    # one class more that no column has
    n_class = min(CLASSES[(a + b) % 4], n_col)
    cls = cases.classes(n_col, n_class)
    n_class = min(n_class + 1, 64)
    ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, dtype, nan,
                              seed=n_col)
    msg = str((n_col, n_row, n_outer, n_bin, nan, by, n_class))
    dev, host = _both(ens, truth, cls, n_class, by, n_bin)
    _assert_same(dev, host, msg)
    assert (host[1].sum(axis=(2, 3)) <= n_col).all()
    if n_class > cls.max() + 1:
      assert not host[0][:, :, n_class - 1].any()
    some = some or host[0].any()
    # the fold: wb2_crps_bin_fold (n_slot = 4 B) and wb2_event_fold
    cols = np.bincount(cls, minlength=n_class)
    wrow = rs.rand(3, n_row) * rs.randint(0, 3, size=(3, n_row))
    mult = rs.randint(0, 3, size=(3, n_class)).astype(np.int32)
    got = engine.conditional_fold(_dev(dev[0]), _dev(dev[1]), cols, wrow, mult)
    want = cond.host_fold(host[0], host[1], cols, wrow, mult)
    for x, y, shape in zip(got, want, ((n_outer, 3, n_bin, 4),
                                       (n_outer, 3, n_bin + 1))):
      assert x.dtype == torch.float64
      assert tuple(x.shape) == y.shape == shape
      np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(y),
                                    err_msg=msg)
  assert some


@pytest.mark.parametrize('by', cases.BYS)
def test_every_bin_count_and_mode_on_both_dtypes(by):
  # the (M, B) pairs the walk above does not meet in this mode, on two tiles
  # and a partial third
  for k, n_bin in enumerate(cases.BINS):
    for dtype in cases.DTYPES:
      n_member = (2, 3, 17, 50, 64)[(k + (dtype is np.float64)) % 5]
      ens, truth = cases.arrays(n_member, 1, 3, 129, dtype, 'both', seed=k)
      dev, host = _both(ens, truth, cases.classes(129, 3), 3, by, n_bin)
      _assert_same(dev, host, str((n_bin, dtype, n_member)))
      assert host[1].sum() > 0


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_class_borders_nan_placement_and_two_runs(dtype):
  # two tiles of columns: the borders 20 | 70 | 100 fall inside both, class 0
  # holds the first and the last columns, class 2 is two separate runs
  n_col = 128
  cls = np.zeros(n_col, np.int32)
  cls[20:70] = 1
  cls[70:100] = 2
  cls[40:44] = 2
  assert cls[0] == cls[-1] == 0
  for n_member, by in ((3, 'spread'), (50, 'forecast')):
    ens, truth = cases.arrays(n_member, 1, 3, n_col, dtype, 'both')
    # NaN truth and NaN member at the tile edges
    truth[0, :, [0, 63, 64, 127]] = np.nan
    ens[n_member - 1, 0, :, [1, 62, 65, 126]] = np.nan
    # all points of a (row, class) invalid; another row's class all in one bin
    truth[0, 1, cls == 1] = np.nan
    ens[:, 0, 2, cls == 2] = 40.0
    truth[0, 2, cls == 2] = 40.0
    dev, host = _both(ens, truth, cls, 3, by, 5)
    _assert_same(dev, host)
    again, _ = _both(ens, truth, cls, 3, by, 5)
    _assert_same(again, dev)  # two runs of the same launch
    assert not host[1][0, 1, 1].any() and not host[0][0, 1, 1].any()
    if by == 'forecast':
      assert (host[1][0, 2, 2] == [0, 0, 0, 0, (cls == 2).sum()]).all()
  # a hand-made interleaved table: every class recurs within a tile and across
  # every tile border; then 1, 3, 10 and 64 classes in runs (with 64 classes
  # every other column changes)
  ens, truth = cases.arrays(7, 2, 3, 129, dtype, 'both')
  for by in cases.BYS:
    dev, host = _both(ens, truth, cases.interleaved(129), 3, by, 5)
    _assert_same(dev, host, by)
    assert (host[1].sum(axis=3) > 0).all()
  for n_class in CLASSES:
    cls = cases.classes(129, n_class)
    assert cls[0] == cls[-1] == 0 or n_class == 1
    dev, host = _both(ens, truth, cls, n_class, 'truth', 17)
    _assert_same(dev, host, str(n_class))
  # the planted point: members (-2, 0, 2) have s2 = 4 exactly and lie in the
  # upper bin of the edge 2.0; mu = 0 and y = 1 on their edges
  ens = np.empty((3, 1, 1, 2), dtype)
  ens[:, 0, 0, :] = np.array([[-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype).T
  truth = np.array([[[1.0, 0.5]]], dtype)
  for by, edge, bins in (('spread', 4.0, (1, 0)), ('forecast', 0.0, (1, 1)),
                         ('truth', 1.0, (1, 0))):
    sums, cnt = engine.conditional_sums(
        _dev(ens), 2, 3, None, _dev(truth), None, 1, 1, 2, np.arange(2), 2,
        by, [edge])
    sums, cnt = sums.cpu().numpy(), cnt.cpu().numpy()
    for j, b in enumerate(bins):
      assert cnt[0, 0, j, b] == 1 and cnt[0, 0, j, 1 - b] == 0, (by, j)
    np.testing.assert_array_equal(sums[0, 0, 0, bins[0]], [0.0, 1.0, 4.0, 1.0])
    np.testing.assert_array_equal(sums[0, 0, 1, bins[1]],
                                  [0.0, 0.5, 1.0, 0.25])


def test_outer_indices_beyond_one_grid_row():
  geo = engine.conditional_geometry(torch.float32, 2, 1, 1)
  n_outer = geo['max_grid_outer'] + 1
  rs = np.random.RandomState(4)
  ens = (np.round(rs.normal(size=(2, n_outer, 1, 3)) * 4) / 4
         ).astype(np.float32)
  truth = (np.round(rs.normal(size=(n_outer, 1, 3)) * 4) / 4
           ).astype(np.float32)
  truth[-1, 0, 2] = np.nan  # the last point of the last outer index
  cls = np.zeros(3, np.int32)
  stride = n_outer * 3
  # (the host path vectorised over the outer indices: one row, one class)
  mu, s2, se, bad = cond.host_point_terms(ens.reshape(2, -1),
                                          truth.reshape(-1))
  which = cond.host_bins(truth.reshape(-1).astype(np.float64), [0.0])
  sums = np.zeros((n_outer, 1, 1, 2, 4))
  cnt = np.zeros((n_outer, 1, 1, 2), np.int32)
  v = np.stack([mu, truth.reshape(-1).astype(np.float64), s2, se], axis=-1
               ).reshape(n_outer, 3, 4)
  which, ok = which.reshape(n_outer, 3), ~bad.reshape(n_outer, 3)
  rows = np.arange(n_outer)
  for j in range(3):
    add = np.zeros((n_outer, 2, 4))
    live = ok[:, j]
    add[rows[live], which[live, j]] = v[live, j]
    sums[:, 0, 0] = sums[:, 0, 0] + add
    cnt[rows[live], 0, 0, which[live, j]] += 1
  dev = engine.conditional_sums(_dev(ens), stride, 2, None, _dev(truth), None,
                                n_outer, 1, 3, cls, 1, 'truth', [0.0])
  _assert_same(tuple(x.cpu().numpy() for x in dev), (sums, cnt))
  assert cnt[-1].sum() == 2 and cnt[0].sum() == 3
  # ... and the first outer indices through host_sums itself
  few = cond.host_sums(ens[:, :4].copy(), 12, 2, None, truth[:4].copy(), None,
                       4, 1, 3, cls, 1, 'truth', [0.0])
  _assert_same((sums[:4], cnt[:4]), few)


def test_sums_walk_the_slab_tables():
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32,
                            'both', seed=5)
  cls = cases.classes(n_col, 2)
  slab = n_row * n_col
  tail = (n_outer, n_row, n_col, cls, 2, 'spread',
          cases.kernel_edges('spread', 5))
  want = cond.host_sums(ens, ens[0].size, n_member, None, truth, None, *tail)
  # members innermost (member_stride = one slab, not the members' extent),
  # outer indices reversed (a permuted slab table); the truth reversed too
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  back = n_outer - 1 - np.arange(n_outer)
  got = engine.conditional_sums(_dev(moved), slab, n_member, table,
                                _dev(truth[::-1]), back, *tail)
  _assert_same(tuple(x.cpu().numpy() for x in got), want)
  host = cond.host_sums(moved, slab, n_member, table,
                        np.ascontiguousarray(truth[::-1]), back, *tail)
  _assert_same(host, want)
  # one truth slab for every outer index, through a table of zeros
  zero = np.zeros(n_outer, np.int64)
  want = cond.host_sums(ens, ens[0].size, n_member, None,
                        np.broadcast_to(truth[1], truth.shape).copy(), None,
                        *tail)
  got = engine.conditional_sums(_dev(ens), ens[0].size, n_member, None,
                                _dev(truth[1]), zero, *tail)
  _assert_same(tuple(x.cpu().numpy() for x in got), want)
  # tables that leave the operands' storage are refused on the host
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    with pytest.raises(IndexError, match='member slabs'):
      engine.conditional_sums(_dev(moved), slab, n_member, table + 1,
                              _dev(truth), None, *tail)
    with pytest.raises(IndexError, match='truth slabs'):
      engine.conditional_sums(_dev(ens), ens[0].size, n_member, None,
                              _dev(truth[:2]), None, *tail)
    with pytest.raises(IndexError, match='col_class'):
      engine.conditional_sums(_dev(ens), ens[0].size, n_member, None,
                              _dev(truth), None, n_outer, n_row, n_col,
                              cls + 1, 2, 'spread', [1.0])
    with pytest.raises(ValueError, match='strictly increasing'):
      engine.conditional_sums(_dev(ens), ens[0].size, n_member, None,
                              _dev(truth), None, n_outer, n_row, n_col, cls,
                              2, 'spread', [1.0, 1.0])
    with pytest.raises(TypeError):
      engine.conditional_sums(_dev(ens), ens[0].size, n_member, None,
                              _dev(truth.astype(np.float64)), None, *tail)
    assert not calls
  finally:
    engine.set_launch_hook(old)


def test_the_out_of_range_calls_launch_nothing():
  from weatherbench2_amd import _lib
  ens, truth = cases.arrays(64, 1, 2, 65, np.float32, 'both')
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    big = _dev(np.zeros((65, 1, 2, 65), np.float32))
    with pytest.raises(ValueError, match='65 members'):
      engine.conditional_sums(big, 130, 65, None, _dev(truth), None, 1, 2, 65,
                              np.zeros(65, np.int32), 1, 'truth', [0.0])
    with pytest.raises(ValueError, match='64 bin edges'):
      engine.conditional_sums(_dev(ens), 130, 64, None, _dev(truth), None, 1,
                              2, 65, np.zeros(65, np.int32), 1, 'truth',
                              np.arange(64.0))
    assert not calls
  finally:
    engine.set_launch_hook(old)
  # the C ABI with device pointers: refused, nothing launched, the outputs
  # untouched
  h = _lib.load()
  out = torch.full((2, 65, 2, 4), 7.0, dtype=torch.float64, device='cuda')
  cnt = torch.full((2, 65, 2), 7, dtype=torch.int32, device='cuda')
  e, y = _dev(ens), _dev(truth)
  col = _dev(np.zeros(65, np.int32))
  edge = _dev(np.zeros(1))
  for n_member, n_class, n_edge, mode, words in (
      (65, 1, 1, 0, b'n_member='), (0, 1, 1, 0, b'n_member='),
      (3, 65, 1, 0, b'n_class='), (3, 0, 1, 0, b'n_class='),
      (3, 1, 64, 0, b'n_edge='), (3, 1, -1, 0, b'n_edge='),
      (3, 1, 1, 3, b'mode=')):
    rc = h.wb2_conditional_sums(
        _lib.WB2_F32, _lib.ptr(e), None, _lib.ptr(y), None, n_member, 130, 1,
        2, 65, _lib.ptr(col), n_class, mode, _lib.ptr(edge), n_edge,
        _lib.ptr(out), _lib.ptr(cnt), None)
    assert rc < 0 and words in h.wb2_last_error()
  torch.cuda.synchronize()
  assert (out == 7.0).all() and (cnt == 7).all()


# ---------------------------------------------------------------------------
# the metric on the device
# ---------------------------------------------------------------------------
GRIDS = ((2, 1), (3, 63), (5, 64), (1, 65), (4, 129), (3, 240))


@pytest.mark.parametrize('grid', GRIDS, ids=lambda v: 'x'.join(map(str, v)))
def test_device_table_equals_the_host_table(grid):
  """The full `compute_chunk` with the 13 evaluation regions (and two more):
  their column classes on 64 and 240 columns among others."""
  a = GRIDS.index(grid)
  regions = cases.product_regions(cases.oracle_regions())
  for b, n_member in enumerate((1, 2, 3, 17, 50, 64)[a % 2::2]):
    dtype = cases.DTYPES[(a + b) % 2]
    nan = cases.NANS[(a + b) % 4]
    by = cases.BYS[(a + b) % 3]
    if n_member == 1 and by == 'spread':
      by = 'forecast'
    n_bin = cases.BINS[(a + 2 * b) % 5]
    ens, truth = cases.arrays(n_member, 2, *grid, dtype, nan)
    forecast, tru = cases.datasets(ens, truth)
    metric = cond.ConditionalTable(cases.edges(by, n_bin), by=by)
    f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
    for skipna in (False, True):
      host = metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                  regions=regions)
      dev = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
      cases.assert_same_dataset(dev, host)
      again = metric.compute_chunk(f_dev, t_dev, skipna=skipna,
                                   regions=regions)
      cases.assert_same_dataset(again, dev)  # two runs
      assert dev[NAME].dims == ('region', 'time', 'term', 'bin')
      assert dev.attrs == {'ensemble_size': n_member, 'by': by,
                           'bin_edges': cases.edges(by, n_bin)}
    assert np.isfinite(dev[NAME].values).any()


def _recorded(monkeypatch):
  seen = []
  real = engine.conditional_sums

  def spy(ens, *args, **kwargs):
    seen.append((ens, args[2], args[4]))
    return real(ens, *args, **kwargs)
  monkeypatch.setattr(engine, 'conditional_sums', spy)
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
  metric = cond.ConditionalTable((0.5, 1.0, 1.5), by='spread')
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
  metric = cond.ConditionalTable((0.5, 1.0), by='spread')
  lsm = xl.DataArray(np.ones((19, 72)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  many = {f'r{k}': greg.SliceRegion(lon_slice=slice(0, float(lon[k])))
          for k in range(70)}
  big = cases.datasets(*cases.arrays(cond.MAX_MEMBERS + 1, 1, 5, 8,
                                     np.float32))
  half = xl.Dataset({NAME: xl.DataArray(f_dev[NAME].data.half(),
                                        f_dev[NAME].dims)}, f_dev.coords)
  one = f_dev.isel(realization=0)
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
         f'{cond.MAX_MEMBERS + 1} members'),
        (lambda: metric.compute_chunk(one, t_dev), 'one member'),
        (lambda: cond.ConditionalTable({'other': (1.0,)}).compute_chunk(
            f_dev, t_dev), 'no entry'),
        (lambda: metric.compute_chunk(half, t_dev), 'float32 and float64')):
      with pytest.raises(ValueError, match=match):
        call()
      assert not calls, match
    metric.compute_chunk(f_dev, t_dev)
    assert [c for c in calls if c[1] == 'conditional_sums']
    assert [c for c in calls if c[1] == 'conditional_fold']
    assert [c for c in calls if c[1] == 'event_fold']
  finally:
    engine.set_launch_hook(old)


def test_conditional_table_in_the_generic_evaluation_loop():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  regions = cases.product_regions(cases.oracle_regions())
  metric = cond.ConditionalTable(cases.edges('spread', 5), by='spread')
  cfg = config.Eval(metrics={'conditional': metric}, regions=regions)
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
