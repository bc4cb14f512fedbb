"""Neighbourhood fractions without a device: the host path of
weatherbench2_amd/neighborhood.py against the restatement
(tests/neighborhood_np.py), known answers of the fractions skill score, the
point-wise event table at window 1, the refusals and the C ABI's checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers
from tests import neighborhood_cases as cases
from tests import neighborhood_np as nnp
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import metrics as gm
from weatherbench2_amd import neighborhood as nb
from weatherbench2_amd import regions as greg
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = 2.0 ** -53
WINDOWS = (1, 3, 5, 13)


# ---------------------------------------------------------------------------
# 1. the three host entry points vs loops from the definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n_member', [1, 2, 7])
def test_host_codes_equal_a_per_point_loop(n_member, dtype):
  n_outer, n_row, n_col = 2, 5, 7
  ens, truth, thrs = cases.edge_case(n_member, 2, n_outer, n_row, n_col, dtype)
  got = nb.host_codes(ens, n_outer * n_row * n_col, n_member, None, truth,
                      None, thrs, None, n_outer, n_row, n_col)
  want = nnp.codes_loop(ens, truth, thrs)
  assert got.dtype == np.uint16 and got.shape == want.shape
  np.testing.assert_array_equal(got, want)
  assert (got == 0x200).any() and ((got >> 8) == 1).any()
  assert not (got[got >= 0x200] != 0x200).any()  # k = o = 0 where invalid
  # through slab tables: members innermost, outer indices reversed
  moved = np.ascontiguousarray(np.moveaxis(ens[:, ::-1], 0, 1))
  table = (n_outer - 1 - np.arange(n_outer)) * n_member
  again = nb.host_codes(moved, n_row * n_col, n_member, table, truth, None,
                        thrs, [np.arange(n_outer)] * 2, n_outer, n_row, n_col)
  np.testing.assert_array_equal(again, want)


@pytest.mark.parametrize('n_row,n_col,windows', [
    (5, 7, (1, 3, 5, 7)),      # a window equal to n_col
    (2, 9, (5, 1)),            # taller than the grid: clipped at both ends
    (1, 3, (3,)),
    (6, 12, (9, 11, 3)),
])
@pytest.mark.parametrize('n_member', [1, 7, 128])
def test_host_sums_equal_the_definition(n_row, n_col, windows, n_member):
  code = cases.code_plane(3, n_row, n_col, n_member, seed=n_row + n_member)
  n_class = min(4, n_col)
  cls = cases.classes(n_col, n_class)
  got = nb.host_sums(code, windows, n_member, cls, n_class)
  want = nnp.sums_loop(code, windows, n_member, cls, n_class)
  assert got.dtype == np.int64 and got.shape == want.shape
  np.testing.assert_array_equal(got, want)
  # every centre is counted once, the invalid ones left out
  np.testing.assert_array_equal(
      got[..., 5].sum(axis=(-2, -1)),
      np.broadcast_to((code != 0x200).sum(axis=(-2, -1))[:, None],
                      got.shape[:2]))
  assert got[..., 5].sum() < code.size * len(windows)


@pytest.mark.parametrize('n_row', [19, 130])
def test_host_fold_is_the_ordered_restatement(n_row):
  rs = np.random.RandomState(2)
  sums = rs.randint(0, 10 ** 9, size=(3, 2, n_row, 5, 6)).astype(np.int64)
  # not a float64: the conversion rounds
  sums[1, 1, n_row - 1, 2, 0] = 2 ** 53 + 1
  w = rs.rand(2, 3, 4, n_row) * rs.randint(0, 3, size=(2, 3, 4, n_row))
  mult = rs.randint(0, 3, size=(4, 5)).astype(np.int32)
  got = nb.host_fold(sums, w, mult)
  want = nnp.fold(sums, w, mult)
  assert got.dtype == np.float64 and got.shape == (3, 2, 4, 6)
  np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def test_window_weights_follow_the_rule():
  wrow = np.array([[0.3, 0.7, 1.1, 0.0, 2.0]])
  w = nb.window_weights(wrow, 7, (1, 3, 9))
  for wi, (n, rows) in enumerate([(1, [1] * 5), (3, [2, 3, 3, 3, 2]),
                                  (9, [5] * 5)]):
    for i in range(5):
      d = float(7 * n * rows[i])
      assert w[wi, 0, 0, i] == wrow[0, i] / (d * d)
      assert w[wi, 1, 0, i] == wrow[0, i] / d
      assert w[wi, 2, 0, i] == wrow[0, i]


# ---------------------------------------------------------------------------
# 2. the metric's host path vs the restatement, over the region sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('ensemble_size', [None, 2, 7])
def test_table_equals_the_restatement(ensemble_size, skipna):
  truth, forecast, clim = cases.random_case(
      ensemble_size, nan_frac=0.05 if skipna else 0.0)
  oregions = cases.oracle_regions()
  metric = nb.FractionsTable(thresholds=cases.product_thresholds(clim),
                             neighborhoods=WINDOWS)
  got = metric.compute_chunk(g(forecast), g(truth), skipna=skipna,
                             regions=cases.product_regions(oregions))
  n_member = ensemble_size or 1
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  rtol = nnp.bound(len(lat), len(lon), n_member, WINDOWS)
  da = got[NAME]
  outer = None
  for q, th in enumerate(cases.oracle_thresholds(clim)):
    outer, ens, tru, thr = cases.dense_operands(
        forecast[NAME], truth[NAME], th.compute(truth)[NAME])
    for r, (name, region) in enumerate(oregions.items()):
      weights = _oracle_region_weights(region, lat, lon)
      want = nnp.dense_components(ens, tru, thr, weights, WINDOWS, skipna)
      # [outer..., window, 4] -> [window, outer..., 4]
      want = np.moveaxis(want, -2, 0)
      np.testing.assert_allclose(da.values[r, q], want, rtol=rtol, atol=0,
                                 equal_nan=True, err_msg=f'{name} q={q}')
      spec = greg.decompose_region(helpers.to_gpu_region(region), lat, lon)
      wrow = gm.plan_lib.get_lat_weights(lat) * spec.lat_mult
      same = np.moveaxis(nnp.ordered_components(
          ens, tru, thr, wrow, spec.lon_mult, WINDOWS, skipna), -2, 0)
      np.testing.assert_array_equal(
          da.values[r, q].view(np.uint64),
          np.ascontiguousarray(same).view(np.uint64),
          err_msg=f'{name} q={q}')
  assert da.dims == ('region', 'quantile', 'neighborhood') + outer + (
      'component',)
  assert da.dtype == np.float64
  np.testing.assert_array_equal(got['quantile'].values, cases.QUANTILES)
  assert got['neighborhood'].values.dtype == np.int64
  np.testing.assert_array_equal(got['neighborhood'].values, WINDOWS)
  assert list(got['component'].values) == list(nnp.COMPONENTS)
  assert list(got['region'].values) == list(oregions)
  assert got.attrs == {'threshold_method': 'GaussianQuantileThreshold',
                       'ensemble_size': n_member}
  assert np.isfinite(da.values).any()
  if not skipna:
    assert np.isfinite(da.values).all()


@pytest.mark.parametrize('skipna', [False, True])
def test_two_rows_clip_every_window_at_both_ends(skipna):
  # 2 rows x 9 columns: window 5 is taller than the grid, so the row range
  # of every centre is clipped at both ends (N_i = 2 n), and window 9 equals
  # n_col; the row weights of `window_weights` against the dense form
  n_member, n_row, n_col, windows = 3, 2, 9, (1, 5, 9)
  forecast, truth, field = cases.small_case(
      n_member, n_row, n_col, n_time=3, nan_frac=0.2 if skipna else 0.0,
      seed=4)
  metric = nb.FractionsTable(
      thresholds=[cases.FieldThreshold(climatology=field, quantile=0.5)],
      neighborhoods=windows)
  got = metric.compute_chunk(forecast, truth, skipna=skipna)['x']
  assert got.dims == ('quantile', 'neighborhood', 'time', 'component')
  lat = truth['latitude'].values
  wrow = gm.plan_lib.get_lat_weights(lat)
  ens, tru, thr = (np.asarray(ds['x'].values, dtype=np.float64)
                   for ds in (forecast, truth, field))
  dense = nnp.dense_components(
      ens, tru, thr, np.broadcast_to(wrow[:, None], (n_row, n_col)), windows,
      skipna)
  np.testing.assert_allclose(
      got.values[0], np.moveaxis(dense, -2, 0), atol=0, equal_nan=True,
      rtol=nnp.bound(n_row, n_col, n_member, windows))
  same = nnp.ordered_components(ens, tru, thr, wrow, np.ones(n_col, np.int64),
                                windows, skipna)
  np.testing.assert_array_equal(
      got.values[0].view(np.uint64),
      np.ascontiguousarray(np.moveaxis(same, -2, 0)).view(np.uint64))
  assert np.isfinite(got.values).any()
  w = nb.window_weights(wrow[None], n_member, windows)
  np.testing.assert_array_equal(w[1, 1, 0], wrow / float(n_member * 5 * 2))


def test_single_region_is_a_slice_of_the_region_set():
  truth, forecast, clim = cases.random_case(2, nan_frac=0.05)
  metric = nb.FractionsTable(thresholds=cases.product_thresholds(clim),
                             neighborhoods=(1, 5))
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(truth), skipna=True,
                               regions=regions)
  for r, (name, region) in enumerate(regions.items()):
    one = metric.compute_chunk(g(forecast), g(truth), region=region,
                               skipna=True)
    assert one[NAME].dims == every[NAME].dims[1:]
    np.testing.assert_array_equal(one[NAME].values, every[NAME].values[r],
                                  err_msg=name)
  # without skipna 5 % NaN void every slab, whatever the region
  void = metric.compute_chunk(g(forecast), g(truth), regions=regions)
  assert np.isnan(void[NAME].values).all()
  # `compute` is the time mean of the components
  mean = metric.compute_regions(g(forecast), g(truth), regions, True)
  axis = every[NAME].dims.index('time')
  np.testing.assert_allclose(mean[NAME].values,
                             np.nanmean(every[NAME].values, axis=axis),
                             rtol=1e-13)
  assert mean.attrs['ensemble_size'] == 2


def test_one_nan_outside_every_region_voids_all_of_them():
  forecast, truth, field = cases.small_case(3, 9, 12, nan_frac=0.0)
  truth['x'].values[0, 0, 5] = np.nan  # the southernmost row, time 0
  lat = truth['latitude'].values
  assert lat[0] < -30
  regions = {'tropics': greg.SliceRegion(lat_slice=slice(-30, 30)),
             'north': greg.SliceRegion(lat_slice=slice(30, 90))}
  metric = nb.FractionsTable(
      thresholds=[cases.FieldThreshold(climatology=field, quantile=0.5)],
      neighborhoods=(1, 3))
  got = metric.compute_chunk(forecast, truth, regions=regions)['x']
  assert got.dims == ('region', 'quantile', 'neighborhood', 'time',
                      'component')
  assert np.isnan(got.values[..., 0, :]).all()
  assert np.isfinite(got.values[..., 1, :]).all()
  kept = metric.compute_chunk(forecast, truth, regions=regions,
                              skipna=True)['x']
  assert np.isfinite(kept.values).all()
  np.testing.assert_array_equal(kept.values[..., 1, :], got.values[..., 1, :])


# ---------------------------------------------------------------------------
# 3. known answers
# ---------------------------------------------------------------------------
def _fss_of(forecast, truth, windows, value=0.5, **kwargs):
  metric = nb.FractionsTable(thresholds=[nb.ConstantThreshold(value)],
                             neighborhoods=windows, ensemble_dim=None)
  table = metric.compute_chunk(forecast, truth, **kwargs)
  return table, nb.fss(table)['x']


@pytest.mark.parametrize('jf,jo', [(3, 5), (11, 1), (4, 4), (0, 3), (7, 6),
                                   (10, 2)])
def test_fss_of_one_displaced_event(jf, jo):
  n_row, n_col, windows = 5, 12, (1, 3, 5, 7)
  d = min((jf - jo) % n_col, (jo - jf) % n_col)
  for row in (0, 2):  # a row whose windows are clipped, and one inside
    forecast, truth = cases.single_events(n_row, n_col, row, jf, jo)
    table, score = _fss_of(forecast, truth, windows)
    assert score.dims == ('quantile', 'neighborhood', 'time')
    checked = 0
    for wi, n in enumerate(windows):
      if n + d <= n_col:
        assert abs(score.values[0, wi, 0] - max(0, n - d) / n) <= 4 * U, (n, d)
        checked += 1
    assert checked >= 3
    np.testing.assert_array_equal(table['quantile'].values, [0.5])


def test_fss_extremes():
  n_row, n_col, windows = 5, 12, (1, 3, 5, 7)
  rs = np.random.RandomState(0)
  lat, lon = cases.axes(n_row, n_col)
  coords = {'time': np.array(['2020-01-01'], 'datetime64[ns]'),
            'latitude': lat, 'longitude': lon}
  dims = ('time', 'latitude', 'longitude')
  ds = lambda a: xl.Dataset({'x': xl.DataArray(a, dims)}, coords)
  field = np.round(rs.normal(size=(1, n_row, n_col)), 1)
  # a perfect forecast
  _, score = _fss_of(ds(field), ds(field.copy()), windows, value=0.0)
  np.testing.assert_array_equal(score.values, 1.0)
  # no event in either field
  table, score = _fss_of(ds(field), ds(field.copy()), windows, value=99.0)
  assert np.isnan(score.values).all()
  np.testing.assert_array_equal(table['x'].values, 0.0)
  # events everywhere in the forecast, none observed
  table, score = _fss_of(ds(field + 200.0), ds(field), windows, value=99.0)
  np.testing.assert_array_equal(score.values, 0.0)
  # (T3 / T5: two ordered sums over the 5 rows and a division)
  np.testing.assert_allclose(table['x'].values[..., 2], 1.0, rtol=2 * 7 * U)
  np.testing.assert_array_equal(table['x'].values[..., 3], 0.0)
  np.testing.assert_array_equal(nb.fss_uniform(table)['x'].values, 0.5)
  assert np.isnan(nb.useful_scale(table)['x'].values).all()


def test_scores_take_tables_and_datasets():
  comp = np.zeros((3, 2, 4))
  # windows 1, 5, 9: fss 0.2, 0.6, 0.9 and fss_uniform 0.55 -> scale 5;
  # second column: never useful
  comp[:, 0, 0], comp[:, 0, 1], comp[:, 0, 3] = [0.8, 0.4, 0.1], 1.0, 0.1
  comp[:, 1, 0], comp[:, 1, 1], comp[:, 1, 3] = [0.9, 0.8, 0.7], 1.0, 0.2
  coords = {'neighborhood': np.array([1, 5, 9], np.int64),
            'lead': np.array([0, 1]),
            'component': np.array(nb.COMPONENTS, dtype=object)}
  da = xl.DataArray(comp, ('neighborhood', 'lead', 'component'), coords, 'x')
  np.testing.assert_allclose(nb.fss(da).values[:, 0], [0.2, 0.6, 0.9],
                             rtol=1e-15)
  np.testing.assert_array_equal(nb.fss_uniform(da).values[:, 0], 0.55)
  scale = nb.useful_scale(da)
  assert scale.dims == ('lead',)
  np.testing.assert_array_equal(scale.values, [5.0, np.nan])
  both = nb.useful_scale(xl.Dataset({'x': da}, coords))
  np.testing.assert_array_equal(both['x'].values, [5.0, np.nan])
  with pytest.raises(ValueError, match='not a fractions table'):
    nb.fss(xl.DataArray(comp[..., :3], ('neighborhood', 'lead', 'k')))


# ---------------------------------------------------------------------------
# 4. window 1 is the point-wise event table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ensemble_size', [None, 2, 7, 33])
def test_window_one_equals_the_event_table(ensemble_size):
  truth, forecast, clim = cases.random_case(ensemble_size, nan_frac=0.05)
  ths = cases.product_thresholds(clim)
  regions = cases.product_regions(cases.oracle_regions())
  frac = nb.FractionsTable(thresholds=ths, neighborhoods=(1,)).compute_chunk(
      g(forecast), g(truth), skipna=True, regions=regions)[NAME]
  table = events.EventTable(thresholds=ths).compute_chunk(
      g(forecast), g(truth), skipna=True, regions=regions)
  n_member = ensemble_size or 1
  n_row, n_col = forecast.sizes['latitude'], forecast.sizes['longitude']
  rtol = 4 * (n_row * n_col + n_member) * U + nnp.bound(n_row, n_col,
                                                        n_member, (1,))
  fbs = frac.values[:, :, 0, ..., 0]
  if ensemble_size is None:
    p = table[NAME].values
    want = p[..., 0, 1] + p[..., 1, 0]
  else:
    want = events.brier_score(table)[NAME].values
  assert fbs.shape == want.shape and np.isfinite(want).any()
  np.testing.assert_allclose(fbs, want, rtol=rtol, atol=0, equal_nan=True)


# ---------------------------------------------------------------------------
# 5. what is refused, before any launch
# ---------------------------------------------------------------------------
def _metric(windows=(1, 3), **kwargs):
  forecast, truth, field = cases.small_case(2, 5, 8, **kwargs)
  return (lambda w=windows: nb.FractionsTable(
      thresholds=[cases.FieldThreshold(climatology=field, quantile=0.5)],
      neighborhoods=w), forecast, truth)


@pytest.mark.parametrize('windows', [(2,), (0,), (-1,), (257,), (9,), (3, 3),
                                     (1, 4), ()])
def test_bad_windows_are_refused(windows):
  make, forecast, truth = _metric()
  with pytest.raises(ValueError, match='window'):
    make(windows).compute_chunk(forecast, truth)


def test_other_refusals():
  make, forecast, truth = _metric()
  assert make().compute_chunk(forecast, truth)['x'].shape == (1, 2, 2, 4)
  # a regional longitude axis, and a non-uniform one
  for lon in (np.arange(8) * 10.0, np.array([0, 45, 90, 135, 180, 225, 270,
                                             300.0])):
    f2, t2 = (xl.Dataset({'x': ds['x']}, dict(ds.coords, longitude=lon))
              for ds in (forecast, truth))
    with pytest.raises(ValueError, match='not cyclic'):
      make().compute_chunk(f2, t2)
  # members outside 1..128
  lat, lon = cases.axes(2, 3)
  coords = {'realization': np.arange(129), 'latitude': lat, 'longitude': lon}
  big = xl.Dataset({'x': xl.DataArray(np.zeros((129, 2, 3)), (
      'realization', 'latitude', 'longitude'))}, coords)
  one = xl.Dataset({'x': xl.DataArray(np.zeros((2, 3)), (
      'latitude', 'longitude'))}, {'latitude': lat, 'longitude': lon})
  with pytest.raises(ValueError, match='129 members'):
    nb.FractionsTable(thresholds=[nb.ConstantThreshold(0.0)],
                      neighborhoods=(1,)).compute_chunk(big, one)
  with pytest.raises(ValueError, match='at least one threshold'):
    nb.FractionsTable(neighborhoods=(1,)).compute_chunk(forecast, truth)
  # more than 64 column classes; a region with a 2-D field
  lat, lon = cases.axes(3, 130)
  coords = {'latitude': lat, 'longitude': lon}
  wide = xl.Dataset({'x': xl.DataArray(np.zeros((3, 130)), (
      'latitude', 'longitude'))}, coords)
  stripes = {str(j): greg.SliceRegion(lon_slice=slice(lon[2 * j],
                                                      lon[2 * j]))
             for j in range(65)}
  metric = nb.FractionsTable(thresholds=[nb.ConstantThreshold(0.0)],
                             neighborhoods=(1,), ensemble_dim=None)
  with pytest.raises(ValueError, match='classes'):
    metric.compute_chunk(wide, wide, regions=stripes)
  lsm = xl.DataArray(np.ones((3, 130)), ('latitude', 'longitude'), coords)
  with pytest.raises(ValueError, match='2-D weight field'):
    metric.compute_chunk(wide, wide, region=greg.LandRegion(lsm))
  # (M n^2)^2 n_col max(mult) >= 2^63
  with pytest.raises(ValueError, match='overflow'):
    nb._check_range(128, (255,), 2 ** 20, np.array([[2 ** 5]]))
  nb._check_range(128, (255,), 1440, np.array([[2]]))


# ---------------------------------------------------------------------------
# 6. absolute thresholds; the class
# ---------------------------------------------------------------------------
def test_constant_threshold():
  forecast, truth, _ = cases.small_case(3, 5, 8)
  th = nb.ConstantThreshold(0.3)
  assert th.quantile == 0.3 and th.value == 0.3
  field = th.compute(truth)
  assert field['x'].dims == ('latitude', 'longitude')
  assert field['x'].values.dtype == np.float32
  np.testing.assert_array_equal(field['x'].values, np.float32(0.3))
  both = xl.Dataset({'x': truth['x'], 'y': xl.DataArray(
      truth['x'].values.astype(np.float64), truth['x'].dims)}, truth.coords)
  th2 = nb.ConstantThreshold({'x': 1.0, 'y': -2.0}, quantile=0.9)
  field = th2.compute(both)
  assert th2.quantile == 0.9
  assert field['y'].values.dtype == np.float64
  np.testing.assert_array_equal(field['x'].values, 1.0)
  np.testing.assert_array_equal(field['y'].values, -2.0)
  with pytest.raises(ValueError, match='quantile'):
    nb.ConstantThreshold({'x': 1.0})
  with pytest.raises(KeyError):
    nb.ConstantThreshold({'z': 1.0}, quantile=0.5).compute(truth)
  # with the event table: the same p as a field of the constant
  as_field = cases.FieldThreshold(climatology=xl.Dataset(
      {'x': xl.DataArray(np.full((2, 5, 8), 0.3, np.float32),
                         ('time', 'latitude', 'longitude'))}, truth.coords),
                                  quantile=0.3)
  got = events.EventTable(thresholds=[th]).compute_chunk(forecast, truth,
                                                         skipna=True)
  want = events.EventTable(thresholds=[as_field]).compute_chunk(
      forecast, truth, skipna=True)
  assert got['x'].dims == want['x'].dims
  np.testing.assert_array_equal(got['x'].values, want['x'].values)
  np.testing.assert_array_equal(got['quantile'].values, [0.3])
  assert got.attrs['threshold_method'] == 'ConstantThreshold'
  frac = nb.FractionsTable(thresholds=[th, nb.ConstantThreshold(-0.4)],
                           neighborhoods=(1, 3)).compute_chunk(
                               forecast, truth, skipna=True)
  np.testing.assert_array_equal(frac['quantile'].values, [0.3, -0.4])
  assert frac['x'].dims == ('quantile', 'neighborhood', 'time', 'component')


def test_class_facts():
  assert issubclass(nb.FractionsTable, gm.ThresholdMetric)
  assert nb.FractionsTable._fused_regions is True
  assert nb.FractionsTable._reads_slabs_in_place is False
  assert nb.FractionsTable().neighborhoods == (1, 3, 5, 9, 17)
  assert nb.FractionsTable().ensemble_dim == 'realization'
  assert not any(getattr(gm, k, None) in (nb.FractionsTable, nb)
                 for k in dir(gm))
  from weatherbench2_amd import thresholds
  assert issubclass(nb.ConstantThreshold, thresholds.Threshold)
  assert not hasattr(thresholds, 'ConstantThreshold')


# ---------------------------------------------------------------------------
# 7. the entry points without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def _words(h, rc, words):
  assert rc < 0 and words in h.wb2_last_error(), h.wb2_last_error()


def test_event_codes_validates_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data
  thr = lib.ptr_array([b])
  call = lambda dtype=lib.WB2_F32, ens=b, n_thr=1, m=5, stride=8, n_outer=2, \
      n_row=2, n_col=4, code=b, t=thr: h.wb2_event_codes(
          dtype, ens, None, b, None, t, None, n_thr, m, stride, n_outer,
          n_row, n_col, code, None)
  _words(h, call(dtype=7), b'unknown dtype')
  _words(h, call(m=0), b'n_member=')
  _words(h, call(m=129), b'n_member=')
  _words(h, call(n_thr=0), b'n_threshold=')
  _words(h, call(stride=-1), b'member_stride=')
  for empty in ('n_outer', 'n_row', 'n_col'):
    assert call(ens=None, code=None, t=None, **{empty: 0}) == 0
  assert call(n_outer=-1) < 0
  _words(h, call(ens=None), b'null pointer')
  _words(h, call(code=None), b'null pointer')
  _words(h, call(t=lib.ptr_array([None])), b'null pointer')


def test_fss_entry_points_validate_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data

  def sums(windows=(1, 3), code=b, n_cell=2, n_row=3, n_col=8, m=5, cls=b,
           n_class=2, out=b, n_window=None):
    win = (ctypes.c_int32 * max(len(windows), 1))(*windows)
    return h.wb2_fss_sums(code, n_cell, n_row, n_col, m,
                          win if windows else None,
                          len(windows) if n_window is None else n_window,
                          cls, n_class, out, None)
  _words(h, sums(m=0), b'n_member=')
  _words(h, sums(m=129), b'n_member=')
  _words(h, sums(n_class=0), b'n_class=')
  _words(h, sums(n_class=65), b'n_class=')
  _words(h, sums(n_window=0), b'n_window=')
  _words(h, sums(n_col=20000), b'LDS budget')
  for empty in ('n_cell', 'n_row', 'n_col'):
    assert sums(code=None, cls=None, out=None, windows=(), n_window=1,
                **{empty: 0}) == 0
  assert sums(n_cell=-1) < 0
  for null in ('code', 'cls', 'out'):
    _words(h, sums(**{null: None}), b'null pointer')
  _words(h, sums(windows=(), n_window=1), b'null pointer')
  for bad in (2, 0, -3, 257, 9):
    _words(h, sums(windows=(1, bad)), b'window=')
  # the geometry: every accepted window count fits 160 KiB
  rows, per, lds, outer = (ctypes.c_int32(), ctypes.c_int32(),
                           ctypes.c_int64(), ctypes.c_int32())
  ref = ctypes.byref
  for n_col in (0, 3, 1440, 3000, 5000, 13000):
    for n_class in (1, 10, 64):
      for n_window in (1, 2, 3, 4, 5, 9):
        assert h.wb2_fss_sums_geometry(n_col, n_class, n_window, ref(rows),
                                       ref(per), ref(lds), ref(outer)) == 0
        assert 1 <= per.value <= min(n_window, 4) and rows.value >= 1
        # the formula of include/wb2hip.h
        assert lds.value == per.value * (n_class * 48 + n_col * 12) + 128
        assert lds.value <= 163840
        assert outer.value >= 1
        geo = engine.fss_sums_geometry(n_col, n_class, n_window)
        assert geo == {'rows_per_group': rows.value,
                       'windows_per_launch': per.value,
                       'lds_bytes': lds.value, 'max_grid_outer': outer.value}
  assert engine.fss_sums_geometry(1440, 10, 6)['windows_per_launch'] == 4
  assert engine.fss_sums_geometry(5000, 10, 6)['windows_per_launch'] == 2
  _words(h, h.wb2_fss_sums_geometry(14000, 1, 1, ref(rows), ref(per),
                                    ref(lds), ref(outer)), b'LDS budget')
  _words(h, h.wb2_fss_sums_geometry(8, 0, 1, ref(rows), ref(per), ref(lds),
                                    ref(outer)), b'n_class=')
  _words(h, h.wb2_fss_sums_geometry(8, 1, 1, None, None, None, None),
         b'null pointer')
  # the fold
  fold = lambda sums=b, n_cell=2, n_window=2, n_row=3, n_class=2, w=b, \
      mult=b, n_region=2, table=b: h.wb2_fss_fold(
          sums, n_cell, n_window, n_row, n_class, w, mult, n_region, table,
          None)
  for empty in ('n_cell', 'n_window', 'n_region'):
    assert fold(sums=None, w=None, mult=None, table=None, **{empty: 0}) == 0
  _words(h, fold(n_class=0), b'n_class=')
  for null in ('sums', 'w', 'mult', 'table'):
    _words(h, fold(**{null: None}), b'null pointer')


def test_engine_checks_its_tables_on_the_host():
  n_member, n_outer, n_row, n_col = 3, 4, 2, 5
  ens, truth, thrs = cases.edge_case(n_member, 1, n_outer, n_row, n_col,
                                     np.float32)
  t_ = torch.from_numpy
  stride = n_outer * n_row * n_col
  with pytest.raises(IndexError, match='member slabs'):
    engine.event_codes(t_(ens), stride, n_member, np.arange(n_outer) + 1,
                       t_(truth), None, [t_(thrs[0])], None, n_outer, n_row,
                       n_col)
  with pytest.raises(IndexError, match='threshold slabs'):
    engine.event_codes(t_(ens), stride, n_member, None, t_(truth), None,
                       [t_(thrs[0][:2])], None, n_outer, n_row, n_col)
  with pytest.raises(TypeError):
    engine.event_codes(t_(ens), stride, n_member, None,
                       t_(truth.astype(np.float64)), None, [t_(thrs[0])],
                       None, n_outer, n_row, n_col)
  code = t_(cases.code_plane(2, n_row, n_col, n_member))
  with pytest.raises(IndexError, match='col_class'):
    engine.fss_sums(code, (1, 3), n_member, [0, 1, 2, 0, 1], 2)
  with pytest.raises(IndexError, match='col_class'):
    engine.fss_sums(code, (1, 3), n_member, [0, 1], 2)
  with pytest.raises(ValueError, match='uint16'):
    engine.fss_sums(code.to(torch.int32), (1,), n_member, [0] * 5, 1)
  with pytest.raises(ValueError, match='no windows'):
    engine.fss_sums(code, (), n_member, [0] * 5, 1)
  sums = torch.zeros((2, 2, n_row, 2, 6), dtype=torch.int64)
  with pytest.raises(ValueError, match='n_region'):
    engine.fss_fold(sums, np.zeros((2, 3, 4, n_row + 1)),
                    np.zeros((4, 2), np.int32))
  with pytest.raises(ValueError, match='int64'):
    engine.fss_fold(sums.to(torch.int32), np.zeros((2, 3, 4, n_row)),
                    np.zeros((4, 2), np.int32))
