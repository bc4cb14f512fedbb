"""Neighbourhood fractions on the device (-m gpu): K19 (csrc/neighborhood.hip)
against the host path of weatherbench2_amd/neighborhood.py, bit for bit, at
the smallest shapes at which the kernels can go wrong."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import neighborhood_cases as cases
from tests import neighborhood_np as nnp
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import neighborhood as nb
from weatherbench2_amd import xarray_lite as xl

pytestmark = pytest.mark.gpu

g = helpers.to_gpu_dataset
NAME = cases.NAME
DTYPES = {np.float32: torch.float32, np.float64: torch.float64}


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_dataset(ds: xl.Dataset) -> xl.Dataset:
  """The same Dataset with its variables in HBM."""
  return xl.Dataset({k: xl.DataArray(_dev(v.values), v.dims)
                     for k, v in ds.items()}, ds.coords, ds.attrs)


# ---------------------------------------------------------------------------
# 1. wb2_event_codes
# ---------------------------------------------------------------------------
def _both_codes(ens, truth, thrs, ens_dev=None):
  """(device codes, host codes) of contiguous [M, O, R, C] operands."""
  n_member, n_outer, n_row, n_col = ens.shape
  stride = n_outer * n_row * n_col
  host = nb.host_codes(ens, stride, n_member, None, truth, None, thrs, None,
                       n_outer, n_row, n_col)
  dev = engine.event_codes(
      _dev(ens) if ens_dev is None else ens_dev, stride, n_member, None,
      _dev(truth), None, [_dev(t) for t in thrs], None, n_outer, n_row, n_col)
  assert dev.dtype == torch.uint16 and tuple(dev.shape) == host.shape
  return dev.cpu().numpy(), host


# (members, thresholds): one member; an odd count; the members' tail of the
# four-at-a-time loop with 4 thresholds in one launch; 5 = a second launch;
# 128 members
COMBOS = [(1, 1), (2, 3), (7, 4), (50, 5), (128, 1)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n_col', [3, 7, 8, 1028, 1031])
def test_device_codes_equal_the_host_path(n_col, dtype):
  # 3 rows of n_col: below one lane group, odd, exact lanes, and past one
  # workgroup of 256 lanes with (1031) and without (1028) a tail
  for n_member, n_thr in COMBOS:
    ens, truth, thrs = cases.edge_case(n_member, n_thr, 2, 3, n_col, dtype,
                                       seed=n_member + n_col)
    dev, host = _both_codes(ens, truth, thrs)
    np.testing.assert_array_equal(dev, host, err_msg=str((n_member, n_thr)))
    assert (host == 0x200).any() and (host & 0x100).any()
  # a base offset by one element: the one-element path on aligned shapes
  ens, truth, thrs = cases.edge_case(7, 3, 2, 3, n_col, dtype, seed=1)
  flat = torch.empty(ens.size + 1, dtype=DTYPES[dtype], device='cuda')
  flat[1:] = _dev(ens).reshape(-1)
  shifted = flat[1:].reshape(ens.shape)
  assert shifted.data_ptr() % 16 != 0
  dev, host = _both_codes(ens, truth, thrs, ens_dev=shifted)
  np.testing.assert_array_equal(dev, host)


def test_codes_walk_the_slab_tables():
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth, thrs = cases.edge_case(n_member, 2, n_outer, n_row, n_col,
                                     np.float32, seed=5)
  want = nnp.codes_loop(ens, truth, thrs)
  # members innermost, outer indices reversed; thresholds of one / all slabs
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  got = engine.event_codes(
      _dev(moved), n_row * n_col, n_member, table, _dev(truth), None,
      [_dev(thrs[0]), _dev(thrs[1][::-1])],
      [None, n_outer - 1 - np.arange(n_outer)], n_outer, n_row, n_col)
  np.testing.assert_array_equal(got.cpu().numpy(), want)
  # tables that leave the operands' storage are refused on the host
  with pytest.raises(IndexError, match='member slabs'):
    engine.event_codes(_dev(moved), n_row * n_col, n_member, table + 1,
                       _dev(truth), None, [_dev(thrs[0])], None, n_outer,
                       n_row, n_col)
  with pytest.raises(TypeError):
    engine.event_codes(_dev(ens), ens[0].size, n_member, None,
                       _dev(truth.astype(np.float64)), None, [_dev(thrs[0])],
                       None, n_outer, n_row, n_col)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n_col', [7, 8])
def test_device_codes_recount_to_the_device_counts(n_col, dtype):
  # what K19's front end and K18 do with (k, obs, bad), held to each other: the
  # codes, recoded and counted per (row, column class), are the event counts.
  # (Both kernels call the one exceed_points(); that is held to the host path
  # by the tests above and by tests/test_events_gpu.py.)
  from tests import events_cases
  from tests import events_np
  n_member, n_outer, n_row, n_class = 7, 2, 3, 4
  ens, truth, thrs = events_cases.edge_case(n_member, 5, n_outer, n_row,
                                            n_col, dtype)
  cls = events_cases.classes(n_col, n_class)
  flat = torch.empty(ens.size + 1, dtype=DTYPES[dtype], device='cuda')
  flat[1:] = _dev(ens).reshape(-1)
  shifted = flat[1:].reshape(ens.shape)
  assert shifted.data_ptr() % 16 != 0
  # (the members as they are, and with their base off by one element)
  for ens_dev in (_dev(ens), shifted):
    front = (ens_dev, n_outer * n_row * n_col, n_member, None, _dev(truth),
             None, [_dev(t) for t in thrs], None, n_outer, n_row, n_col)
    plane = engine.event_codes(*front).cpu().numpy()
    counts = engine.event_counts(*front, cls, n_class).cpu().numpy()
    np.testing.assert_array_equal(
        events_np.counts_of_code_planes(plane, n_member, cls, n_class), counts)
    assert counts[..., -1].sum() > 0  # the NaN placements are inside


# ---------------------------------------------------------------------------
# 2. wb2_fss_sums on code planes made on the host
# ---------------------------------------------------------------------------
def _window_sets(n_col):
  top = min(n_col if n_col % 2 else n_col - 1, 255)
  sets = [(1,), (3,), (1, 3, 5, 9), (1, 3, 5, 7, 9), (top,)]
  out = []
  for s in sets:
    s = tuple(n for n in s if n <= n_col)
    if s and s not in out:
      out.append(s)
  return out


@pytest.mark.parametrize('n_col', [3, 7, 8, 260, 263])
def test_device_sums_equal_the_host_path(n_col):
  # n_col: below one lane group, odd, one column per thread, and two columns
  # per thread with (263) and without (260) threads that own none
  geo = engine.fss_sums_geometry(n_col, 10, 5)
  per = geo['rows_per_group']
  assert geo['windows_per_launch'] == 4  # five windows: a second launch
  members, class_counts = (1, 50, 128), (1, 4, 10)
  seen = set()
  for ri, n_row in enumerate((1, 2, 5, per + 1, 2 * per + 1)):
    for wi, windows in enumerate(_window_sets(n_col)):
      for ci, n_class in enumerate(class_counts):
        n_member = members[(ri + wi + ci) % 3]
        n_class = min(n_class, n_col)
        seen.add((n_member, n_class))
        code = cases.code_plane(3, n_row, n_col, n_member,
                                seed=n_row + n_col + wi)
        cls = cases.classes(n_col, n_class)  # classes are not contiguous
        want = nb.host_sums(code, windows, n_member, cls, n_class)
        got = engine.fss_sums(_dev(code), windows, n_member, cls, n_class)
        assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
        np.testing.assert_array_equal(
            got.cpu().numpy(), want,
            err_msg=str((n_row, windows, n_class, n_member)))
  assert {m for m, _ in seen} == set(members)


def test_sums_of_contiguous_classes_and_the_definition():
  # classes that are runs of columns: whole waves of one class (the wave
  # reduction), a wave with a class border, and the loop from the definition
  n_row, n_col, n_member, windows = 4, 700, 5, (1, 5, 33)
  code = cases.code_plane(2, n_row, n_col, n_member, seed=3)
  cls = np.repeat(np.arange(4), [200, 290, 10, 200]).astype(np.int32)
  got = engine.fss_sums(_dev(code), windows, n_member, cls, 4).cpu().numpy()
  np.testing.assert_array_equal(
      got, nb.host_sums(code, windows, n_member, cls, 4))
  small = code[:, :, :40]
  np.testing.assert_array_equal(
      engine.fss_sums(_dev(small), windows, n_member, cls[:40] * 0, 1
                      ).cpu().numpy(),
      nnp.sums_loop(small, windows, n_member, cls[:40] * 0, 1))
  # two runs are bit-equal; a 4-D plane [threshold, outer, row, column]
  again = engine.fss_sums(_dev(code.reshape(2, 1, n_row, n_col)), windows,
                          n_member, cls, 4).cpu().numpy()
  np.testing.assert_array_equal(again, got)
  with pytest.raises(IndexError, match='col_class'):
    engine.fss_sums(_dev(code), windows, n_member, cls + 1, 4)


# ---------------------------------------------------------------------------
# 3. wb2_fss_fold
# ---------------------------------------------------------------------------
# n_row: less than one block of 64 rows per wave; exactly one; one row into a
# second block; two blocks and a tail of 2 (the accumulators are carried from
# block to block, the tail adds fewer than 64 lanes)
@pytest.mark.parametrize('n_row', [19, 64, 65, 130])
def test_fold_is_the_ordered_restatement(n_row):
  rs = np.random.RandomState(2 + n_row)
  n_region = 13  # twelve regions and the pseudo-region
  sums = rs.randint(0, 10 ** 9, size=(3, 3, n_row, 5, 6)).astype(np.int64)
  # the conversion to float64 rounds; in a row of the last block
  big_row = {19: 7, 64: 63, 65: 64, 130: 129}[n_row]
  sums[2, 1, big_row, 3, 0] = 2 ** 53 + 1
  wrow = rs.rand(n_region, n_row) * rs.randint(0, 3, size=(n_region, n_row))
  wrow[-1] = 1.0
  mult = rs.randint(0, 3, size=(n_region, 5)).astype(np.int32)
  mult[-1] = 1
  mult[:, 3] = np.maximum(mult[:, 3], 1)  # the large sum counts everywhere
  w = nb.window_weights(wrow, 7, (1, 5, 9))
  got = engine.fss_fold(_dev(sums), w, mult)
  assert got.dtype == torch.float64 and tuple(got.shape) == (3, 3, 13, 6)
  want = nnp.fold(sums, w, mult)
  np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64),
                                want.view(np.uint64))
  np.testing.assert_array_equal(nb.host_fold(sums, w, mult).view(np.uint64),
                                want.view(np.uint64))
  # the order matters at these sizes: the reversed row order differs
  back = nnp.fold(sums[:, :, ::-1], w[..., ::-1], mult)
  assert not np.array_equal(back, want)
  with pytest.raises(ValueError, match='n_region'):
    engine.fss_fold(_dev(sums), w[..., :5], mult)


def test_sums_with_more_than_64_kib_of_lds():
  # 1440 columns and four windows: 71 168 bytes of dynamic LDS, which a
  # kernel gets only after the entry point has raised its limit
  n_row, n_col, n_member, windows = 3, 1440, 50, (1, 5, 9, 17)
  geo = engine.fss_sums_geometry(n_col, 10, len(windows))
  assert geo['windows_per_launch'] == 4 and geo['lds_bytes'] > 64 * 1024
  code = cases.code_plane(2, n_row, n_col, n_member, seed=11)
  cls = cases.classes(n_col, 10)
  got = engine.fss_sums(_dev(code), windows, n_member, cls, 10)
  np.testing.assert_array_equal(
      got.cpu().numpy(), nb.host_sums(code, windows, n_member, cls, 10))


# ---------------------------------------------------------------------------
# 4. the metric end to end
# ---------------------------------------------------------------------------
WINDOWS = (1, 3, 5)


def _small_case(seed=0):
  """Forecast (realization 3, time 2, prediction_timedelta 6, latitude 5,
  longitude 8), truth (time, latitude, longitude) and two threshold fields,
  one without the lead dim and one with it."""
  rs = np.random.RandomState(seed)
  lat, lon = cases.axes(5, 8)
  coords = {'realization': np.arange(3),
            'time': np.array(['2020-01-01', '2020-01-02'], 'datetime64[ns]'),
            'prediction_timedelta': np.arange(6) * np.timedelta64(1, 'D'),
            'latitude': lat, 'longitude': lon}
  full = np.round(rs.normal(size=(3, 2, 6, 5, 8)), 1).astype(np.float32)
  full[1, 0, 2, 3, 4] = full[0, 1, 4, 0, 0] = np.nan
  tru = np.round(rs.normal(size=(2, 5, 8)), 1).astype(np.float32)
  tru[1, 4, 7] = np.nan
  thr_a = np.round(rs.normal(size=(2, 5, 8)) * 0.5, 1).astype(np.float32)
  thr_b = np.round(rs.normal(size=(6, 2, 5, 8)) * 0.5, 1).astype(np.float32)
  return coords, full, tru, thr_a, thr_b


def _small_metric(coords, thr_a, thr_b, lead, put, transpose=False):
  sub = dict(coords, prediction_timedelta=coords['prediction_timedelta'][lead])
  tail = ('longitude', 'latitude') if transpose else ('latitude', 'longitude')
  turn = (lambda a: np.swapaxes(a, -1, -2)) if transpose else (lambda a: a)
  fields = [
      xl.Dataset({'x': xl.DataArray(put(turn(thr_a)), ('time',) + tail)}, sub),
      xl.Dataset({'x': xl.DataArray(put(turn(thr_b[lead])),
                                    ('prediction_timedelta', 'time') + tail)},
                 sub)]
  return nb.FractionsTable(
      thresholds=[cases.FieldThreshold(climatology=f, quantile=q)
                  for f, q in zip(fields, (0.5, 0.9))], neighborhoods=WINDOWS)


def test_views_gathers_and_layouts_equal_the_host_path(monkeypatch):
  coords, full, tru, thr_a, thr_b = _small_case()
  dims = ('realization', 'time', 'prediction_timedelta', 'latitude',
          'longitude')
  regions = {'global': None, 'north': helpers.to_gpu_region(
      helpers.predefined_regions()['northern-hemisphere'])}
  lead = slice(1, 5)
  sub = dict(coords, prediction_timedelta=coords['prediction_timedelta'][lead])
  host = np.ascontiguousarray

  def run(data, put, var_dims=dims, transpose=False):
    tdims = dims[1:2] + (var_dims[3:])
    truth = xl.Dataset({'x': xl.DataArray(
        put(np.swapaxes(tru, -1, -2) if transpose else tru), tdims)}, sub)
    forecast = xl.Dataset({'x': xl.DataArray(data, var_dims)}, sub)
    metric = _small_metric(coords, thr_a, thr_b, lead, put, transpose)
    return metric.compute_chunk(forecast, truth, skipna=True, regions=regions)

  want = run(host(full[:, :, lead]), host)
  assert want['x'].dims == ('region', 'quantile', 'neighborhood', 'time',
                            'prediction_timedelta', 'component')
  assert np.isfinite(want['x'].values).all()

  seen = []
  real = engine.event_codes

  def spy(ens, *args):
    seen.append((ens, args[2]))
    return real(ens, *args)
  monkeypatch.setattr(engine, 'event_codes', spy)

  # materialised contiguous (lat, lon) copies in HBM
  cases.assert_same_dataset(run(_dev(full[:, :, lead]), _dev), want)
  assert seen[-1][0].is_contiguous() and seen[-1][1] is None
  # a lead-sliced VIEW of the resident forecast: read where it lies
  view = _dev(full)[:, :, lead]
  assert not view.is_contiguous()
  cases.assert_same_dataset(run(view, _dev), want)
  assert seen[-1][0] is view and seen[-1][1] is not None
  # a SlabGather over a shuffled base: read through its index
  rs = np.random.RandomState(1)
  order = rs.permutation(2 * 4)
  index = (np.arange(3)[:, None, None] * 8 + order.reshape(2, 4)[None])
  base = np.zeros((24, 5, 8), np.float32)
  base[index.reshape(-1)] = full[:, :, lead].reshape(-1, 5, 8)
  base_dev = _dev(base)
  cases.assert_same_dataset(run(xl.SlabGather(base_dev, index), _dev), want)
  assert seen[-1][0] is base_dev and seen[-1][1] is not None
  # (lon, lat) everywhere: one transposing copy, the same table
  got = run(_dev(np.swapaxes(full[:, :, lead], -1, -2)), _dev,
            dims[:3] + ('longitude', 'latitude'), transpose=True)
  cases.assert_same_dataset(got, want)
  # skipna=False: the slabs with a NaN are void, on both paths alike
  metric = _small_metric(coords, thr_a, thr_b, lead, _dev)
  truth = xl.Dataset({'x': xl.DataArray(_dev(tru), dims[1:2] + dims[3:])}, sub)
  forecast = xl.Dataset({'x': xl.DataArray(view, dims)}, sub)
  void = metric.compute_chunk(forecast, truth, regions=regions)['x'].values
  assert np.isnan(void[:, :, :, 1]).all()  # the truth's NaN, time 1
  assert np.isfinite(void[:, :, :, 0, 0]).all()


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('ensemble_size', [None, 7])
def test_metric_on_the_device_equals_the_host_path(ensemble_size, skipna):
  truth, forecast, clim = cases.random_case(
      ensemble_size, nan_frac=0.05 if skipna else 0.0)
  regions = cases.product_regions(cases.oracle_regions())
  metric = nb.FractionsTable(thresholds=cases.product_thresholds(clim),
                             neighborhoods=(1, 3, 5, 9, 17))
  host = metric.compute_chunk(g(forecast), g(truth), skipna=skipna,
                              regions=regions)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(truth))
  dev = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
  cases.assert_same_dataset(dev, host)
  assert np.isfinite(dev[NAME].values).any()
  mean = metric.compute_regions(f_dev, t_dev, regions, skipna)
  cases.assert_same_dataset(
      mean, metric.compute_regions(g(forecast), g(truth), regions, skipna))
  score = nb.fss(mean)[NAME]
  assert score.dims == mean[NAME].dims[:-1]
  finite = score.values[np.isfinite(score.values)]
  assert finite.size and (finite <= 1.0).all() and (finite >= 0.0).all()


def test_constant_threshold_on_the_device():
  forecast, truth, _ = cases.small_case(3, 5, 8)
  th = [nb.ConstantThreshold(0.3), nb.ConstantThreshold(-0.4)]
  f_dev, t_dev = _device_dataset(forecast), _device_dataset(truth)
  field = th[0].compute(t_dev)['x'].data
  assert field.device == t_dev['x'].data.device and field.dtype == torch.float32
  assert tuple(field.shape) == (5, 8)
  metric = nb.FractionsTable(thresholds=th, neighborhoods=(1, 3))
  cases.assert_same_dataset(
      metric.compute_chunk(f_dev, t_dev, skipna=True),
      metric.compute_chunk(forecast, truth, skipna=True))
  table = events.EventTable(thresholds=th)
  cases.assert_same_dataset(table.compute_chunk(f_dev, t_dev, skipna=True),
                            table.compute_chunk(forecast, truth, skipna=True))


def test_fractions_table_in_the_generic_evaluation_loop():
  from weatherbench2_amd import config, evaluation
  truth, forecast, clim = cases.random_case(7)
  f_dev = _device_dataset(g(forecast)).isel(time=slice(0, 2))
  t_dev = _device_dataset(g(truth)).isel(time=slice(0, 2))
  regions = cases.product_regions(cases.oracle_regions())
  metric = nb.FractionsTable(thresholds=cases.product_thresholds(clim),
                             neighborhoods=(1, 5))
  cfg = config.Eval(metrics={'fractions': metric}, regions=regions)
  res = xl.as_dataset(evaluation._metric_and_region_loop(
      f_dev, t_dev, cfg, False, compute_chunk=True))
  want = metric.compute_chunk(f_dev, t_dev, regions=regions)
  da = res[NAME]
  assert da.dims == ('metric',) + want[NAME].dims
  np.testing.assert_array_equal(np.asarray(da.values)[0], want[NAME].values)
  assert want[NAME].sizes['time'] == 2
  # ... and with the time mean
  res = xl.as_dataset(evaluation._metric_and_region_loop(
      f_dev, t_dev, cfg, False))
  mean = metric.compute_regions(f_dev, t_dev, regions)
  np.testing.assert_array_equal(np.asarray(res[NAME].values)[0],
                                mean[NAME].values)


# ---------------------------------------------------------------------------
# 5. wb2_fss_sums where the LDS budget splits the launches
# ---------------------------------------------------------------------------
FSS_THREADS = 256  # the workgroup of fss_sums_kernel: one row, all columns


def _widest_row(n_class, n_window=1):
  """The largest n_col that `engine.fss_sums_geometry` admits: bisection over
  the geometry call (the LDS bytes grow with n_col)."""
  from weatherbench2_amd import _lib

  def fits(n_col):
    try:
      engine.fss_sums_geometry(n_col, n_class, n_window)
      return True
    except _lib.Wb2HipError as e:
      assert 'LDS budget' in str(e)
      return False
  lo, hi = 1, 1 << 20
  assert fits(lo) and not fits(hi)
  while hi - lo > 1:
    mid = (lo + hi) // 2
    lo, hi = (mid, hi) if fits(mid) else (lo, mid)
  return lo


def _sums_both(code, windows, n_member, cls, n_class):
  got = engine.fss_sums(_dev(code), windows, n_member, cls, n_class)
  want = nb.host_sums(code, windows, n_member, cls, n_class)
  assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
  return got.cpu().numpy(), want


def test_window_batches_that_the_budget_splits():
  # five windows at two per launch: fss_sums_kernel<2>, <2> and <1>, each with
  # its own offset into the sums of the call
  n_row, n_col, n_member, n_class = 3, 5000, 50, 10
  windows = (1, 3, 9, 33, 255)
  geo = engine.fss_sums_geometry(n_col, n_class, len(windows))
  assert geo['windows_per_launch'] == 2
  code = cases.code_plane(2, n_row, n_col, n_member, seed=21)
  cls = cases.classes(n_col, n_class)
  got, want = _sums_both(code, windows, n_member, cls, n_class)
  for wi, n in enumerate(windows):
    np.testing.assert_array_equal(got[:, wi], want[:, wi], err_msg=str(n))
  assert all(want[:, wi].any() for wi in range(len(windows)))
  # the first 64 columns of the same plane as a call of their own (the
  # windows that such a row takes), against the loop from the definition
  small = np.ascontiguousarray(code[:, :, :64])
  fit = tuple(n for n in windows if n <= 64)
  assert fit == windows[:4]
  np.testing.assert_array_equal(
      engine.fss_sums(_dev(small), fit, n_member, cls[:64], n_class
                      ).cpu().numpy(),
      nnp.sums_loop(small, fit, n_member, cls[:64], n_class))


def test_more_than_32_columns_per_thread():
  # 33 columns per thread: the mask of a thread's invalid centres is shifted
  # by up to 32
  n_row, n_col, n_member, n_class = 3, 8200, 50, 10
  windows = (3, 17)
  per = -(-n_col // FSS_THREADS)
  assert per == 33
  geo = engine.fss_sums_geometry(n_col, n_class, len(windows))
  assert geo['windows_per_launch'] == 1
  code = cases.code_plane(2, n_row, n_col, n_member, seed=22, invalid=1 / 3)
  # columns 32 and 33 counted from the start of several threads' runs
  for t in (0, 1, 63, 64, 127, 200, 247):
    for j in (per * t + 32, per * t + 33):
      assert j < n_col
      code[:, :, j] = 0x200
  # ... and a thread whose only invalid centre is its column 32
  t = 100
  keep = code[0, 1, per * t:per * (t + 1)]
  keep[keep == 0x200] = 3
  keep[32] = 0x200
  cls = cases.classes(n_col, n_class)
  got, want = _sums_both(code, windows, n_member, cls, n_class)
  np.testing.assert_array_equal(got, want)
  share = (code == 0x200).mean()
  assert 0.3 < share < 0.4
  # (the valid centres counted, per row: what the mask decides)
  np.testing.assert_array_equal(got[..., 5].sum(axis=-1)[:, 0],
                                (code != 0x200).sum(axis=-1))


def test_the_widest_row_that_fits_and_the_refusal_one_column_later():
  from weatherbench2_amd import _lib
  n_row, n_member = 2, 7
  widest = _widest_row(1)
  assert widest == 13638
  geo = engine.fss_sums_geometry(widest, 1, 1)
  assert geo['lds_bytes'] == 163832 and -(-widest // FSS_THREADS) == 54
  wide10 = _widest_row(10)
  assert wide10 < widest
  for n_col, n_class in ((widest, 1), (wide10, 10)):
    code = cases.code_plane(1, n_row, n_col, n_member, seed=n_class)
    cls = cases.classes(n_col, n_class)  # (10 classes: not contiguous)
    for windows in ((1,), (255,)):
      got, want = _sums_both(code, windows, n_member, cls, n_class)
      np.testing.assert_array_equal(got, want,
                                    err_msg=str((n_col, n_class, windows)))
    # one column more: refused by the entry point, before any launch (the
    # hook's bracket stays open: no 'end')
    over = _dev(np.zeros((1, n_row, n_col + 1), np.uint16))
    calls = []
    old = engine.set_launch_hook(lambda *a: calls.append(a))
    try:
      with pytest.raises(_lib.Wb2HipError, match='LDS budget'):
        engine.fss_sums(over, (1,), n_member, np.zeros(n_col + 1, np.int32),
                        n_class)
    finally:
      engine.set_launch_hook(old)
    assert calls == [('begin', 'fss_sums')]


def _assert_cells(got, want, n_cell, axis):
  for cell in (0, 32767, 32768, n_cell - 1):
    np.testing.assert_array_equal(np.take(got, cell, axis=axis),
                                  np.take(want, cell, axis=axis),
                                  err_msg=f'cell {cell}')
  np.testing.assert_array_equal(got, want)


def test_cells_beyond_one_grid_row():
  geo = engine.fss_sums_geometry(3, 1, 1)
  n_cell = geo['max_grid_outer'] + 1
  assert n_cell > 32768
  # wb2_fss_sums: every cell its own codes
  n_member = 5
  code = cases.code_plane(n_cell, 1, 3, n_member, seed=23, invalid=0.2)
  code[:, 0, 0] = np.arange(n_cell) % (n_member + 1)  # (valid, cell by cell)
  code[-1, 0, 2] = 0x200
  cls = np.array([0, 1, 0], np.int32)
  got, want = _sums_both(code, (1, 3), n_member, cls, 2)
  _assert_cells(got, want, n_cell, 0)
  assert (want[-1] != want[0]).any() and (want[32768] != want[32767]).any()
  # wb2_event_codes: one member, one threshold, the same outer count
  rs = np.random.RandomState(24)
  ens = np.round(rs.normal(size=(1, n_cell, 1, 3)), 1).astype(np.float32)
  truth = np.round(rs.normal(size=(n_cell, 1, 3)), 1).astype(np.float32)
  thr = np.round(rs.normal(size=(n_cell, 1, 3)) * 0.5, 1).astype(np.float32)
  truth[-1, 0, 2] = ens[0, 32768, 0, 0] = np.nan
  dev, host = _both_codes(ens, truth, [thr])
  _assert_cells(dev, host, n_cell, 1)
  assert host[0, -1, 0, 2] == 0x200 and host[0, 32768, 0, 0] == 0x200
