"""Structure-function verification on the host: `structure.VariogramTable`
against the dense restatement of tests/variogram_np.py, its identities, the
scores, the metric protocol and the refusals of the engine and the C ABI (no
device needed: nothing is launched)."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import metrics_np as om
from tests import helpers
from tests import variogram_cases as cases
from tests import variogram_np as vnp
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import regions as greg
from weatherbench2_amd import structure
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = vnp.U
MEMBERS = (1, 2, 7)
# every grid, member count and order; dtype and NaNs cycle
CASES = [(grid, m, order, cases.DTYPES[(a + b + c) % 2], (a + b + c) % 3 != 0)
         for a, grid in enumerate(cases.GRIDS)
         for b, m in enumerate(MEMBERS)
         for c, order in enumerate(cases.ORDERS)]
_ID = lambda v: ('x'.join(map(str, v)) if isinstance(v, tuple) else
                 getattr(v, '__name__', None) or str(v))
WORST = {'fraction': 0.0}


def _lags(grid):
  """The named lags; on the wider grids the default ones and the largest
  offsets too (13 in all)."""
  top = min(grid[1] - 1, 32)
  return cases.LAGS if grid[1] < 30 else cases.LAGS + structure.DEFAULT_LAGS[
      2:] + ((3, top), (16, -top))


def _table(values):
  """A variogram table DataArray of a [.., 3, L] array (leading dims d0 ..)."""
  values = np.asarray(values, dtype=np.float64)
  lead = tuple(f'd{k}' for k in range(values.ndim - 2))
  return xl.DataArray(values, lead + (cases.TERM, cases.LAG))


def _oracle_regions():
  """The 13 evaluation regions, an overlapping slice list and the
  extra-tropics."""
  return cases.oracle_regions()


@functools.lru_cache(maxsize=None)
def _case(grid, n_member, order, dtype, nan):
  """The arrays, the oracle datasets and the product's tables (every region,
  both skipna) of one case: computed once, shared and left unchanged."""
  ens, truth = cases.planted(n_member, 1, *grid, dtype, nan=nan,
                             seed=grid[1] + n_member)
  forecast, tru = cases.datasets(ens, truth)
  oregions = _oracle_regions()
  metric = structure.VariogramTable(_lags(grid), order=order)
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, oregions, tables


# ---------------------------------------------------------------------------
# 1. the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('grid,n_member,order,dtype,nan', CASES, ids=_ID)
def test_host_path_equals_the_dense_restatement(grid, n_member, order, dtype,
                                                nan):
  ens, truth, forecast, tru, oregions, tables = _case(grid, n_member, order,
                                                      dtype, nan)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  lags = _lags(grid)
  n_lag = len(lags)
  col_class, mult, wrow = events.column_classes(
      cases.product_regions(oregions), lat, lon)
  n_class = mult.shape[1]
  sums, cnt = structure.host_sums(ens, truth.size, n_member, None, truth, None,
                                  1, *grid, col_class, n_class, order, lags)
  assert sums.dtype == np.float64 and cnt.dtype == np.int32
  assert sums.shape == (1, grid[0], n_class, n_lag, 3)
  assert cnt.shape == (1, grid[0], n_class, n_lag, 2)
  # the counts: equal; all three terms non-negative; no -0.0 anywhere
  np.testing.assert_array_equal(
      cnt, vnp.dense_counts(ens, truth, col_class, n_class, lags))
  assert (sums >= 0).all() and not np.signbit(sums).any()
  # valid + invalid = the columns of the class where the lag exists
  cols = np.bincount(col_class, minlength=n_class)
  for l, (a, _) in enumerate(lags):
    there = np.arange(grid[0]) + a < grid[0]
    np.testing.assert_array_equal(
        cnt[0, :, :, l].sum(axis=-1), there[:, None] * cols[None, :])
  rtol = vnp.table_rtol(*grid, n_class)
  assert rtol <= vnp.worst_case_rtol(*grid, n_class)
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'time', cases.TERM, cases.LAG)
    assert da.dtype == np.float64 and da.shape[-2:] == (3, n_lag)
    assert got.attrs == {'ensemble_size': n_member, 'lags': tuple(lags),
                         'order': float(order)}
    assert list(got['region'].values) == list(oregions)
    assert list(got[cases.TERM].values) == list(cases.TERMS)
    np.testing.assert_array_equal(got[cases.LAG].values, np.arange(n_lag))
    assert got[cases.LAG].values.dtype == np.int64
    for r, (name, region) in enumerate(oregions.items()):
      w = _oracle_region_weights(region, lat, lon)
      want = vnp.dense_table(ens, truth, w, lags, order, skipna)
      msg = f'{name} skipna={skipna}'
      np.testing.assert_array_equal(np.isnan(da.values[r]), np.isnan(want),
                                    err_msg=msg)
      live = ~np.isnan(want)
      np.testing.assert_array_equal(da.values[r][live] == 0, want[live] == 0,
                                    err_msg=msg)
      pos = live & (want > 0)
      err = np.abs(da.values[r] - want)[pos] / want[pos]
      if err.size:
        WORST['fraction'] = max(WORST['fraction'], err.max() / rtol)
        print(f'{msg}: worst relative error {err.max() / U:.2f} u, '
              f'{err.max() / rtol:.3f} of the bound')
        assert err.max() <= rtol, msg
    # a lag that no row reaches is NaN throughout
    for l, (a, _) in enumerate(lags):
      if a >= grid[0]:
        assert np.isnan(da.values[..., l]).all()
    if not nan:
      reach = [l for l, (a, _) in enumerate(lags) if a < grid[0]]
      assert np.isfinite(da.values[0][..., reach]).all()
    elif not skipna:
      assert np.isnan(da.values[0][:, 0, 0]).any()
  # one region alone is that slice of the fused pass within twice the bound
  # (other column classes, the same pairs)
  metric = structure.VariogramTable(lags, order=order)
  for name in ('global', 'europe'):
    one = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               region=helpers.to_gpu_region(oregions[name]))
    assert one[NAME].dims == tables[True][NAME].dims[1:]
    fused = tables[True][NAME].values[list(oregions).index(name)]
    np.testing.assert_allclose(one[NAME].values, fused, rtol=2 * rtol, atol=0,
                               equal_nan=True)


def test_the_worst_fraction_of_the_bound_is_reported():
  # (after the cases above in file order; a lone run has nothing to report)
  print(f"worst observed fraction of table_rtol: {WORST['fraction']:.3f}")
  assert WORST['fraction'] <= 1.0


# ---------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('order', cases.ORDERS)
def test_a_forecast_that_is_the_truth_scores_zero(order):
  _, truth = cases.planted(1, 2, 5, 30, np.float32, seed=1)
  forecast, tru = cases.datasets(truth[None].copy(), truth)
  lags = cases.LAGS + ((5, 1),)
  for skipna in (False, True):
    got = structure.VariogramTable(lags, order=order).compute_chunk(
        g(forecast), g(tru), skipna=skipna,
        regions=cases.product_regions(cases.oracle_regions()))[NAME].values
    live = ~np.isnan(got[..., 0, :])
    assert live.any()
    score = got[..., 2, :][live]
    assert (score == 0).all() and not np.signbit(score).any()
    np.testing.assert_array_equal(got[..., 1, :].view(np.uint64),
                                  got[..., 0, :].view(np.uint64))
    # the lag (5, 1) needs a sixth row
    assert np.isnan(got[..., -1]).all()
    assert skipna == bool(np.isfinite(got[0, :, :, 0]).all())


def test_order_one_column_lags_are_the_mae_of_the_rolled_truth():
  n_row, n_col = 19, 72
  _, truth = cases.arrays(1, 3, n_row, n_col, np.float64, seed=2)
  forecast, tru = cases.datasets(truth[None].copy(), truth)
  lags = ((0, 1), (0, -1), (0, 5), (0, 32), (0, -32))
  got = structure.VariogramTable(lags, order=1).compute_chunk(
      g(forecast), g(tru))[NAME].values
  assert got.shape == (3, 3, len(lags))
  for l, (_, b) in enumerate(lags):
    rolled, _ = cases.datasets(np.roll(truth, -b, axis=-1)[None], truth)
    mae = np.asarray(om.MAE().compute_chunk(
        rolled.isel(realization=0), tru)[NAME].data)
    np.testing.assert_allclose(got[:, 0, l], mae, rtol=n_col * U, atol=0)
    assert (mae > 0).all()


@pytest.mark.parametrize('order', cases.ORDERS)
def test_a_column_lag_and_its_wrap_give_the_same_bits(order):
  n_col = 30
  ens, truth = cases.planted(7, 2, 5, n_col, np.float32, seed=3)
  cls = cases.rotated(n_col, 3)
  for b in (1, 3, 29, -4):
    other = b - n_col if b > 0 else b + n_col
    args = (ens, truth.size, 7, None, truth, None, 2, 5, n_col, cls, 3, order)
    one = structure.host_sums(*args, ((0, b), (2, b)))
    two = structure.host_sums(*args, ((0, other), (2, other)))
    np.testing.assert_array_equal(one[0].view(np.uint64),
                                  two[0].view(np.uint64))
    np.testing.assert_array_equal(one[1], two[1])
    assert one[1][..., 0].any() and one[1][..., 1].any()


def test_pairs_by_hand():
  """One row of four columns, two members: every number written out."""
  truth = np.array([[[1.0, 3.0, 0.0, np.nan]]], np.float32)
  ens = np.array([[[[0.0, 4.0, 1.0, 2.0]]], [[[2.0, 3.0, 1.0, 0.0]]]],
                 np.float32)
  cls = np.zeros(4, np.int32)
  for order, gfun in ((1, abs), (2, lambda d: d * d),
                      (0.5, lambda d: np.sqrt(abs(d)))):
    sums, cnt = structure.host_sums(ens, 4, 2, None, truth, None, 1, 1, 4, cls,
                                    1, order, ((0, 1), (1, 0)))
    # lag (0, 1): anchors 0, 1 are valid, 2 (partner NaN) and 3 are not
    gy = [gfun(1.0 - 3.0), gfun(3.0 - 0.0)]
    gf = [(gfun(0.0 - 4.0) + gfun(2.0 - 3.0)) / 2,
          (gfun(4.0 - 1.0) + gfun(3.0 - 1.0)) / 2]
    want = [gy[0] + gy[1], gf[0] + gf[1],
            (gy[0] - gf[0]) ** 2 + (gy[1] - gf[1]) ** 2]
    np.testing.assert_array_equal(sums[0, 0, 0, 0], want)
    np.testing.assert_array_equal(cnt[0, 0, 0, 0], [2, 2])
    # lag (1, 0): the only row has no row below it
    assert not sums[0, 0, 0, 1].any() and not cnt[0, 0, 0, 1].any()


def test_a_deterministic_forecast_is_one_member():
  ens, truth = cases.planted(1, 2, 5, 30, np.float64, seed=4)
  forecast, tru = cases.datasets(ens, truth)
  plain = g(forecast).isel(realization=0)
  for metric in (structure.VariogramTable(cases.LAGS),
                 structure.VariogramTable(cases.LAGS, ensemble_dim=None)):
    got = metric.compute_chunk(plain, g(tru), skipna=True)
    assert got.attrs['ensemble_size'] == 1
    want = structure.VariogramTable(cases.LAGS).compute_chunk(
        g(forecast), g(tru), skipna=True)
    np.testing.assert_array_equal(got[NAME].values, want[NAME].values)


# ---------------------------------------------------------------------------
# 3. the scores
# ---------------------------------------------------------------------------
def test_scores_on_a_hand_written_table():
  p = np.array([[[2.0, 4.0, 0.0, np.nan], [1.0, 4.0, 0.0, 1.0],
                 [0.5, 0.0, 0.0, 3.0]],
                [[1.0, 1.0, 1.0, 1.0], [2.0, 3.0, 4.0, 5.0],
                 [1.0, 2.0, 0.0, 4.0]]])
  table = _table(p)
  ratio = structure.variogram_ratio(table)
  assert ratio.dims == ('d0', cases.LAG)
  np.testing.assert_array_equal(
      ratio.values, [[0.5, 1.0, np.nan, np.nan], [2.0, 3.0, 4.0, 5.0]])
  score = structure.variogram_score(table)
  assert score.dims == ('d0',)
  np.testing.assert_array_equal(score.values, [3.5, 7.0])
  weighted = structure.variogram_score(table, lag_weights=(1, 0.5, 0, 0.25))
  np.testing.assert_array_equal(weighted.values, [1.25, 3.0])
  ref = _table(p[::-1].copy())
  skill = structure.variogram_skill(table, ref)
  assert skill.dims == ('d0', cases.LAG)
  np.testing.assert_array_equal(
      skill.values, [[0.5, 1.0, np.nan, 0.25], [-1.0, -np.inf, np.nan,
                                               1.0 - 4.0 / 3.0]])
  with pytest.raises(ValueError, match='4 weights'):
    structure.variogram_score(table, lag_weights=(1, 2))
  with pytest.raises(ValueError, match='not a variogram table'):
    structure.variogram_ratio(xl.DataArray(p, ('d0', cases.LAG, cases.TERM)))
  with pytest.raises(ValueError, match='differ in shape'):
    structure.variogram_skill(table, _table(p[:, :, :3]))


def test_a_smoothed_forecast_has_a_ratio_below_one():
  rs = np.random.RandomState(0)
  truth = rs.normal(size=(1, 9, 68)).astype(np.float32)
  smooth = (truth + np.roll(truth, 1, -1) + np.roll(truth, -1, -1)) / 3
  forecast, tru = cases.datasets(smooth[None].astype(np.float32), truth)
  table = structure.VariogramTable(((0, 1), (0, 2), (0, 8)), order=2
                                   ).compute_chunk(g(forecast), g(tru))
  ratio = structure.variogram_ratio(table)[NAME].values
  assert (ratio < 0.6).all()
  score = structure.variogram_score(table)
  assert score[NAME].dims == ('time',) and (score[NAME].values > 0).all()
  skill = structure.variogram_skill(table, table)[NAME].values
  np.testing.assert_array_equal(skill, 0.0)


# ---------------------------------------------------------------------------
# 4. the metric protocol: time mean, bootstrap, Eval, Pooled
# ---------------------------------------------------------------------------
def test_compute_is_the_time_mean_of_the_tables():
  n_time = 3
  ens, truth = cases.arrays(7, n_time, 5, 30, np.float32, seed=3)
  forecast, tru = cases.datasets(ens, truth)
  metric = structure.VariogramTable(cases.LAGS, order=1)
  whole = metric.compute(g(forecast), g(tru))
  assert whole[NAME].dims == (cases.TERM, cases.LAG)
  assert whole.attrs == {'ensemble_size': 7, 'lags': cases.LAGS, 'order': 1.0}
  chunks = [metric.compute_chunk(g(forecast.isel(time=slice(k, k + 1))),
                                 g(tru.isel(time=slice(k, k + 1)))
                                 )[NAME].values[0] for k in range(n_time)]
  np.testing.assert_allclose(whole[NAME].values, np.mean(chunks, axis=0),
                             rtol=4 * U, atol=0)
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               regions=regions)
  fan = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  cases.assert_same_dataset(fan, every)
  mean = metric.compute_regions(g(forecast), g(tru), regions, True)
  assert mean[NAME].dims == ('region', cases.TERM, cases.LAG)
  assert mean.attrs['order'] == 1.0 and mean.attrs['ensemble_size'] == 7


def test_bootstrap_and_every_score_carry_the_replicate_dim():
  ens, truth = cases.arrays(7, 6, 5, 30, np.float64, seed=4)
  forecast, tru = cases.datasets(ens, truth)
  tables = structure.VariogramTable(cases.LAGS).compute_chunk(g(forecast),
                                                              g(tru))
  assert tables[NAME].dims == ('time', cases.TERM, cases.LAG)
  kwargs = dict(n_replicate=25, block_length=2, seed=2)
  out = bs.bootstrap(tables, structure.variogram_score, **kwargs)
  counts = bs.block_plan(6, 25, 2, seed=2)
  rep = bs.resample_means(tables, counts)
  reps = structure.variogram_score(rep)[NAME]
  assert reps.dims == (bs.REPLICATE,) and reps.shape == (25,)
  assert np.isfinite(reps.values).all()
  np.testing.assert_array_equal(out[NAME + '_standard_error'].values,
                                np.asarray(reps.values).std(axis=0, ddof=1))
  loop = bs.bootstrap(tables, structure.variogram_score, vectorized=False,
                      **kwargs)
  cases.assert_same_dataset(out, loop)
  # every function keeps the leading dim; a DataArray gives the result itself
  lead = (bs.REPLICATE,)
  assert structure.variogram_ratio(rep)[NAME].dims == lead + (cases.LAG,)
  assert structure.variogram_ratio(rep[NAME]).dims == lead + (cases.LAG,)
  assert structure.variogram_skill(rep, rep)[NAME].dims == lead + (cases.LAG,)
  assert structure.variogram_score(rep[NAME]).dims == lead


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 30, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = structure.VariogramTable(cases.LAGS)
  assert metric._fused_regions and not metric._reads_slabs_in_place
  cfg = config.Eval(metrics={'variogram': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims
  assert da.dims[-2:] == (cases.TERM, cases.LAG)
  assert [d for d in da.dims if d != 'metric'][0] == 'region'
  want = metric.compute_chunk(g(forecast), g(tru), regions=regions)[NAME]
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(want.shape), want.values)
  assert list(loop['region'].values) == list(regions)


def test_pooled_at_window_one_is_the_plain_table():
  from weatherbench2_amd import pooling
  ens, truth = cases.arrays(7, 2, 5, 30, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = structure.VariogramTable(cases.LAGS, order=2)
  plain = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  pooled = pooling.Pooled(metric, neighborhoods=(1,)).compute_chunk_regions(
      g(forecast), g(tru), regions, True)
  assert pooled[NAME].dims == ('neighborhood',) + plain[NAME].dims
  np.testing.assert_array_equal(
      np.asarray(pooled[NAME].values)[0].view(np.uint64),
      np.asarray(plain[NAME].values).view(np.uint64))


# ---------------------------------------------------------------------------
# 5. the refusals
# ---------------------------------------------------------------------------
def _refuses(call, match):
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    with pytest.raises(ValueError, match=match):
      call()
  finally:
    engine.set_launch_hook(old)
  assert not calls


def test_refusals_come_before_any_launch():
  ens, truth = cases.arrays(3, 1, 19, 72, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  run = lambda *args, **kwargs: structure.VariogramTable(
      *args, **kwargs).compute_chunk(g(forecast), g(tru))
  for order in (0, 1.5, 3, 'one', None, -1):
    _refuses(lambda: run(order=order), 'order=')
  _refuses(lambda: run(()), 'non-empty sequence')
  _refuses(lambda: run((1, 2)), 'non-empty sequence')
  _refuses(lambda: run(((0, 1, 2),)), 'non-empty sequence')
  _refuses(lambda: run(((0, 0.5),)), 'whole numbers')
  _refuses(lambda: run((('a', 1),)), 'whole numbers')
  _refuses(lambda: run(((0, 0),)), r'\(0, 0\)')
  _refuses(lambda: run(((-1, 0),)), 'row offset must be >= 0')
  _refuses(lambda: run(((0, 1), (1, 0), (0, 1))), 'given twice')
  _refuses(lambda: run(tuple((1, b) for b in range(17))), '17 lags.*1 to 16')
  _refuses(lambda: run(((17, 0),)), 'row offset 17.*0 to 16')
  _refuses(lambda: run(((0, 33),)), 'column offset of size 33.*up to 32')
  _refuses(lambda: run(((0, -33),)), 'column offset of size 33.*up to 32')
  # |b| must be below the number of longitudes
  small = cases.datasets(*cases.arrays(3, 1, 5, 8, np.float32))
  _refuses(lambda: structure.VariogramTable(((0, 8),)).compute_chunk(
      g(small[0]), g(small[1])), 'column offset of size 8.*8 longitudes')
  # a regional longitude axis is not cyclic
  part = g(forecast).isel(longitude=slice(0, 40))
  _refuses(lambda: structure.VariogramTable().compute_chunk(
      part, g(tru).isel(longitude=slice(0, 40))), 'not cyclic')
  metric = structure.VariogramTable()
  lsm = xl.DataArray(np.ones((19, 72)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  _refuses(lambda: metric.compute_chunk(
      g(forecast), g(tru), regions={'global': None,
                                    'the-land': greg.LandRegion(lsm)}),
           'the-land.*LandRegion.*2-D')
  many = {f'r{k}': greg.SliceRegion(lon_slice=slice(0, float(lon[k])))
          for k in range(70)}
  _refuses(lambda: metric.compute_chunk(g(forecast), g(tru), regions=many),
           'classes')
  big = cases.datasets(*cases.arrays(structure.MAX_MEMBERS + 1, 1, 5, 30,
                                     np.float32))
  _refuses(lambda: metric.compute_chunk(g(big[0]), g(big[1])),
           f'{structure.MAX_MEMBERS + 1} members.*1 to 128')
  for dtype in (np.float16, np.int32):
    odd = cases.datasets(ens.astype(dtype), truth)
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
    odd = cases.datasets(ens, truth.astype(dtype))
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
  # variables that differ in ensemble size
  two = xl.Dataset({NAME: g(forecast)[NAME],
                    'other': g(forecast).isel(realization=slice(0, 2))[NAME]},
                   {k: v for k, v in g(forecast).coords.items()
                    if k != 'realization'})
  tru2 = xl.Dataset({NAME: g(tru)[NAME], 'other': g(tru)[NAME]},
                    g(tru).coords)
  _refuses(lambda: metric.compute_chunk(two, tru2), 'differ in ensemble size')
  # 16 lags at the limits and 128 members are taken
  wide = tuple((a, 32 if a % 2 else -32) for a in range(16))[1:] + ((16, 0),)
  assert run(wide)[NAME].shape[-2:] == (3, 16)
  full = cases.datasets(*cases.arrays(128, 1, 5, 30, np.float32))
  assert metric.compute_chunk(g(full[0]), g(full[1])).attrs[
      'ensemble_size'] == 128
  assert run().attrs['lags'] == structure.DEFAULT_LAGS


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_both_symbols_are_exported_and_declared(lib):
  import os
  h = lib.load()
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  header = open(os.path.join(root, 'include', 'wb2hip.h')).read()
  for name in ('wb2_variogram_sums', 'wb2_variogram_geometry'):
    assert getattr(h, name) is not None
    assert re.search(r'^int %s\(' % name, header, re.M), name
  assert 'K27' in header and 'n_slot = 3 n_lag' in header
  from weatherbench2_amd import build
  assert 'variogram.hip' in build.SOURCES


def test_engine_refuses_bad_tables_sizes_and_lags_on_the_host(lib):
  """Host tensors stand in for the operands: every refusal below comes from
  the host checks, before anything is uploaded or launched."""
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32)
  e, y = torch.from_numpy(ens), torch.from_numpy(truth)
  cls = cases.rotated(n_col, 2)
  slab = n_row * n_col
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def sums(ens=e, stride=n_outer * slab, n_member=n_member, ens_slab=None,
           truth=y, truth_slab=None, n_outer=n_outer, cls=cls, n_class=2,
           order=0.5, lags=((0, 1), (1, 0))):
    return engine.variogram_sums(ens, stride, n_member, ens_slab, truth,
                                 truth_slab, n_outer, n_row, n_col, cls,
                                 n_class, order, lags)
  try:
    for kwargs, error, match in (
        (dict(ens_slab=np.arange(n_outer) + 1), IndexError, 'member slabs'),
        (dict(ens_slab=np.arange(n_outer - 1)), ValueError, 'member slab'),
        (dict(stride=n_outer * slab + 1), IndexError, 'member slabs'),
        (dict(truth=y[:2].clone()), IndexError, 'truth slabs'),
        (dict(truth_slab=np.array([0, 1, 2, -1])), IndexError, 'truth slabs'),
        (dict(cls=cls + 1), IndexError, 'col_class'),
        (dict(cls=cls[:-1]), IndexError, 'col_class'),
        (dict(n_member=0), ValueError, '0 members'),
        (dict(n_member=129, stride=0), ValueError, '129 members'),
        (dict(stride=-1), ValueError, 'bad sizes'),
        (dict(n_outer=-1), ValueError, 'bad sizes'),
        (dict(order=3), ValueError, 'order='),
        (dict(order='x'), ValueError, 'order='),
        (dict(lags=()), ValueError, 'non-empty'),
        (dict(lags=((0, 0),)), ValueError, r'\(0, 0\)'),
        (dict(lags=((-1, 1),)), ValueError, '>= 0'),
        (dict(lags=((0, 1), (0, 1))), ValueError, 'twice'),
        (dict(lags=((0, 8),)), ValueError, 'below n_col=8'),
        (dict(lags=((0, -8),)), ValueError, 'below n_col=8'),
        (dict(lags=((17, 0),)), ValueError, 'row offset 17'),
        (dict(lags=tuple((a, 1) for a in range(17))), ValueError, '17 lags'),
        (dict(truth=y.double()), TypeError, 'dtype'),
        (dict(ens=e.half(), truth=y.half()), TypeError, 'dtype'),
        (dict(truth=y.transpose(-1, -2)), ValueError, 'contiguous'),
        (dict(n_class=65), lib.Wb2HipError, 'n_class='),
        # float64 strips of 17 row offsets: over the LDS budget
        (dict(ens=e.double(), truth=y.double(),
              lags=tuple((a, 0) for a in range(1, 17))), lib.Wb2HipError,
         'LDS budget')):
      with pytest.raises(error, match=match):
        sums(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
  good = torch.zeros(1, 2, 3, 4, 3, dtype=torch.float64)
  with pytest.raises(ValueError, match='sums must be'):
    engine.variogram_fold(good, torch.zeros(1, 2, 3, 4, 3, dtype=torch.int32),
                          None, np.ones((1, 2)), np.ones((1, 3), np.int32))
  with pytest.raises(ValueError, match='wrow'):
    engine.variogram_fold(good, torch.zeros(1, 2, 3, 4, 2, dtype=torch.int32),
                          None, np.ones((1, 4)), np.ones((1, 3), np.int32))


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data
  lag = lambda *pairs: np.array(pairs, np.int32).reshape(-1, 2)
  deep = lag(*[(a, 0) for a in range(1, 17)])

  def sums(dtype=lib.WB2_F32, ens=b, n_member=5, stride=8, n_outer=2, n_row=2,
           n_col=4, n_class=2, order=0, lags=lag((0, 1), (1, -2)), n_lag=2,
           out=b, cnt=b):
    return h.wb2_variogram_sums(
        dtype, ens, None, b, None, n_member, stride, n_outer, n_row, n_col, b,
        n_class, order, None if lags is None else lags.ctypes.data, n_lag,
        out, cnt, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=129), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(n_lag=0), b'n_lag='),
      (dict(lags=deep, n_lag=17), b'n_lag='), (dict(order=3), b'order_code='),
      (dict(order=-1), b'order_code='), (dict(lags=None), b'null pointer'),
      (dict(lags=lag((17, 0)), n_lag=1), b'row offset'),
      (dict(lags=lag((-1, 1)), n_lag=1), b'row offset'),
      (dict(lags=lag((0, 33)), n_lag=1), b'column offset'),
      (dict(lags=lag((0, -33)), n_lag=1), b'column offset'),
      (dict(lags=lag((0, 4)), n_lag=1), b'below n_col'),
      (dict(lags=lag((1, -4)), n_lag=1), b'below n_col'),
      (dict(lags=lag((0, 1), (0, 0))), b'(0, 0)'),
      (dict(dtype=lib.WB2_F64, lags=deep, n_lag=16), b'LDS budget'),
      (dict(stride=-1), b'member_stride='), (dict(n_row=-1), b'negative'),
      (dict(ens=None), b'null pointer'), (dict(out=None), b'null pointer'),
      (dict(cnt=None), b'null pointer'),
      (dict(n_col=1 << 28, lags=lag((0, 1)), n_lag=1), b'too long')):
    assert sums(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert sums(ens=None, **empty) == 0


def test_geometry_values_and_the_lds_refusal(lib):
  h = lib.load()
  for dtype, size in ((torch.float32, 4), (torch.float64, 8)):
    for n_member in (1, 50, 128):
      for lags, n_off in ((((0, 1),), 1), (structure.DEFAULT_LAGS, 5),
                          (cases.LAGS, 3),
                          (tuple((a, 32) for a in range(1, 9)), 9)):
        geo = engine.variogram_geometry(dtype, n_member, 13, 2, lags)
        # the formula of include/wb2hip.h
        strips = 4 * n_off * 128 * size
        tile = 64 * ((3 * len(lags)) | 1) * 8
        assert geo['lds_bytes'] == max(strips, tile) + 256 <= 65536
        assert (geo['min_member'], geo['max_member']) == (
            structure.MIN_MEMBERS, structure.MAX_MEMBERS) == (1, 128)
        assert geo['max_lags'] == structure.MAX_LAGS == 16
        assert geo['max_row_offset'] == structure.MAX_ROW_OFFSET >= 8
        assert geo['max_col_offset'] == structure.MAX_COL_OFFSET >= 32
        assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
        assert geo['max_grid_outer'] == engine.conditional_geometry(
            dtype)['max_grid_outer']
  deep = tuple((a, 0) for a in range(1, 17))
  assert engine.variogram_geometry(torch.float32, 1, 1, 0.5, deep)[
      'lds_bytes'] == 4 * 17 * 128 * 4 + 256
  with pytest.raises(lib.Wb2HipError, match='LDS budget') as ei:
    engine.variogram_geometry(torch.float64, 1, 1, 0.5, deep)
  lg = np.array(deep, np.int32)
  b = np.zeros(8, np.int64).ctypes.data
  assert h.wb2_variogram_sums(lib.WB2_F64, b, None, b, None, 1, 8, 1, 1, 4, b,
                              1, 0, lg.ctypes.data, 16, b, b, None) < 0
  assert h.wb2_last_error().decode() in str(ei.value)
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.variogram_geometry(torch.float32, 129)
  with pytest.raises(lib.Wb2HipError, match='n_class='):
    engine.variogram_geometry(torch.float32, 1, 65)
  with pytest.raises(lib.Wb2HipError, match='row offset'):
    engine.variogram_geometry(torch.float32, 1, 1, 1, ((17, 0),))
  with pytest.raises(ValueError, match='order='):
    engine.variogram_geometry(torch.float32, 1, 1, 4)
  with pytest.raises(TypeError):
    engine.variogram_geometry(torch.float16)
  one = np.array([[0, 1]], np.int32)
  null = h.wb2_variogram_geometry(lib.WB2_F32, 1, 1, 0, one.ctypes.data, 1,
                                  None, None, None, None, None, None, None,
                                  None, None)
  assert null < 0 and b'null pointer' in h.wb2_last_error()
