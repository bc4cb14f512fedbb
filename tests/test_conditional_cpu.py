"""Conditional verification on the host path (no GPU): the dense restatement,
the marginal against the oracle's region means, exact cases planted by hand,
validity and emptiness, the metric protocol, the scores and the refusals."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import metrics_np as om
from tests import conditional_cases as cases
from tests import conditional_np as cnp
from tests import helpers
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import conditional as cond
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import pooling
from weatherbench2_amd import regions as greg
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = cnp.U

# every member count, dtype and grid; the NaN patterns, what is binned and the
# bin counts cycle so that each meets both dtypes and both grids
CASES = [(grid, m, dtype, cases.NANS[(a + b + c) % 4],
          cases.BYS[(a + b + 2 * c) % 3], cases.BINS[(2 * a + b + c) % 5])
         for a, grid in enumerate(cases.GRIDS)
         for b, m in enumerate(cases.MEMBERS)
         for c, dtype in enumerate(cases.DTYPES)]
# one member has no spread to bin by
CASES = [(grid, m, dtype, nan, 'forecast' if m == 1 and by == 'spread' else by,
          n_bin) for grid, m, dtype, nan, by, n_bin in CASES]
_ID = lambda v: getattr(v, '__name__', None) or (
    'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


def _metric(by, n_bin, **kwargs):
  return cond.ConditionalTable(cases.edges(by, n_bin), by=by, **kwargs)


@functools.lru_cache(maxsize=None)
def _case(grid, n_member, dtype, nan, by, n_bin):
  """The arrays, the oracle datasets and the product's tables (every region,
  both skipna) of one case: computed once, shared and left unchanged."""
  n_time = 2 if grid == cases.GRIDS[0] else 1
  ens, truth = cases.arrays(n_member, n_time, *grid, dtype, nan)
  forecast, tru = cases.datasets(ens, truth)
  oregions = cases.oracle_regions()
  metric = _metric(by, n_bin)
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, oregions, tables


# ---------------------------------------------------------------------------
# 1. the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('grid,n_member,dtype,nan,by,n_bin', CASES, ids=_ID)
def test_table_equals_the_dense_restatement(grid, n_member, dtype, nan, by,
                                            n_bin):
  ens, truth, forecast, tru, oregions, tables = _case(
      grid, n_member, dtype, nan, by, n_bin)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  given = cases.edges(by, n_bin)
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'time', 'term', 'bin')
    assert da.dtype == np.float64
    assert got.attrs == {'ensemble_size': n_member, 'by': by,
                         'bin_edges': given}
    assert list(got['region'].values) == list(oregions)
    assert list(got['term'].values) == list(cond.TERMS)
    np.testing.assert_array_equal(got['bin'].values, np.arange(n_bin))
    for r, (name, region) in enumerate(oregions.items()):
      w = _oracle_region_weights(region, lat, lon)
      want, scale = cnp.dense_table(ens, truth, w, given, by, skipna)
      atol = cnp.table_atol(len(lat), len(lon), n_bin, scale)
      msg = f'{name} skipna={skipna}'
      np.testing.assert_array_equal(np.isnan(da.values[r]), np.isnan(want),
                                    err_msg=msg)
      live = ~np.isnan(want)
      assert (np.abs(da.values[r] - want)[live] <= atol[live]).all(), msg
      # an empty bin of a live cell is 0 in every term
      empty = live & (want[:, :1, :] == 0)
      assert (da.values[r][empty] == 0).all(), msg
    if nan == 'none':
      assert np.isfinite(da.values[0]).all()
    elif not skipna:
      assert np.isnan(da.values[0]).any()
  # the bin of every point is the restatement's: the counts of the host sums
  # per (outer index, row, bin) are its histogram
  n_time, n_row, n_col = truth.shape
  sums, cnt = cond.host_sums(
      ens, truth.size, n_member, None, truth, None, n_time, n_row, n_col,
      np.zeros(n_col, np.int32), 1, by, cases.kernel_edges(by, n_bin))
  which = cnp.point_bins(ens, truth, given, by)
  valid = cnp.point_fields(ens, truth)[3]
  for o in range(n_time):
    for i in range(n_row):
      np.testing.assert_array_equal(
          cnt[o, i, 0], np.bincount(which[o, i][valid[o, i]],
                                    minlength=n_bin))
  # one region alone (None, and one that wraps) is that slice of the fused
  # pass: the same bins, and sums over other column classes (each side within
  # the bound of the exact value)
  metric = _metric(by, n_bin)
  for name in ('global', 'europe'):
    one = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               region=helpers.to_gpu_region(oregions[name]))
    assert one[NAME].dims == tables[True][NAME].dims[1:]
    fused = tables[True][NAME].values[list(oregions).index(name)]
    _, scale = cnp.dense_table(
        ens, truth, _oracle_region_weights(oregions[name], lat, lon), given,
        by, True)
    atol = 2 * cnp.table_atol(len(lat), len(lon), n_bin, scale)
    live = ~np.isnan(fused)
    np.testing.assert_array_equal(np.isnan(one[NAME].values), ~live)
    assert (np.abs(one[NAME].values - fused)[live] <= atol[live]).all(), name
    np.testing.assert_array_equal(one[NAME].values[:, 0], fused[:, 0])


# ---------------------------------------------------------------------------
# 2. the marginal against the oracle's region means
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_bin', [1, 5])
@pytest.mark.parametrize('n_member', [2, 7, 33])
def test_marginal_equals_the_oracles_region_means(n_member, n_bin):
  grid = cases.GRIDS[1]
  by = cases.BYS[(n_member + n_bin) % 3]
  ens, truth, forecast, tru, oregions, tables = _case(
      grid, n_member, np.float64, 'none', by, n_bin)
  table = tables[False]
  m = cond.marginal(table)[NAME]
  assert m['variance'].dims == ('region', 'time')
  atol = cnp.marginal_atol(ens, truth, grid[0] * grid[1], n_bin)
  mean = forecast.mean('realization', skipna=False)
  for r, (name, region) in enumerate(oregions.items()):
    want = {
        'variance': om.EnsembleVariance().compute_chunk(
            forecast, tru, region=region)[NAME].data,
        'squared_error': om.EnsembleMeanMSE().compute_chunk(
            forecast, tru, region=region)[NAME].data,
        'bias': om.Bias().compute_chunk(mean, tru, region=region)[NAME].data}
    for key, value in want.items():
      np.testing.assert_allclose(m[key].values[r], value, rtol=0,
                                 atol=atol[key], err_msg=f'{name} {key}')
    np.testing.assert_allclose(m['weight'].values[r], 1.0, rtol=0,
                               atol=(n_bin + 2 * grid[0] + 4) * U)
    if n_bin == 1:  # no edges: the table IS those metrics
      for k, key in ((3, 'variance'), (4, 'squared_error')):
        np.testing.assert_allclose(table[NAME].values[r, :, k, 0], want[key],
                                   rtol=0, atol=atol[key])
      np.testing.assert_array_equal(table[NAME].values[r, :, 0, 0], 1.0)
  assert np.abs(m['variance'].values).min() > 0.1


# ---------------------------------------------------------------------------
# 3. exact cases planted by hand
# ---------------------------------------------------------------------------
def _columns(cols, dtype, n_row=2):
  """(forecast, truth) Datasets of [(members, truth)] per column, the same in
  every row."""
  n_member = len(cols[0][0])
  ens = np.empty((n_member, 1, n_row, len(cols)), dtype=dtype)
  truth = np.empty((1, n_row, len(cols)), dtype=dtype)
  for j, (members, y) in enumerate(cols):
    ens[:, 0, :, j] = np.array(members, dtype=dtype)[:, None]
    truth[0, :, j] = y
  forecast, tru = cases.datasets(ens, truth)
  return g(forecast), g(tru)


def _close(got, want):
  """Within a few roundings: the weights of the rows are no powers of two, so
  wrow * s is rounded (the bin of every point, and with it every `weight` made
  of equal counts, is exact)."""
  np.testing.assert_allclose(got, want, rtol=8 * U, atol=0)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_values_on_an_edge_belong_to_the_upper_bin(dtype):
  # members (-2, 0, 2): mu = 0, s2 = (4 + 0 + 4) / 2 = 4 exactly, spread 2.0
  cols = [((-2.0, 0.0, 2.0), 1.0), ((-1.0, 0.0, 1.0), 0.5),
          ((0.0, 4.0, 8.0), 4.0), ((2.0, 2.0, 2.0), 2.0)]
  forecast, tru = _columns(cols, dtype)
  p = cond.ConditionalTable((2.0,), by='spread').compute_chunk(
      forecast, tru)[NAME].values[0]
  # columns 0 (s = 2, ON the edge) and 2 (s = 4) are the upper bin
  np.testing.assert_array_equal(p[0], [0.5, 0.5])
  _close(p[3], [(1.0 + 0.0) / 4, (4.0 + 16.0) / 4])
  _close(p[1], [(0.0 + 2.0) / 4, (0.0 + 4.0) / 4])
  _close(p[2], [(0.5 + 2.0) / 4, (1.0 + 4.0) / 4])
  _close(p[4], [(0.25 + 0.0) / 4, (1.0 + 0.0) / 4])
  # mu on an edge (0.0 and 4.0), y on an edge (0.5, 1.0 and 2.0)
  p = cond.ConditionalTable((0.0, 4.0), by='forecast').compute_chunk(
      forecast, tru)[NAME].values[0]
  _close(p[0], [0.0, 0.75, 0.25])
  p = cond.ConditionalTable((0.5, 1.0, 2.0, 4.5), by='truth').compute_chunk(
      forecast, tru)[NAME].values[0]
  np.testing.assert_array_equal(p[0], [0.0, 0.25, 0.25, 0.5, 0.0])
  # the scores of that table: an empty bin is 0 with NaN conditional means
  table = cond.ConditionalTable((0.5, 1.0, 2.0, 4.5), by='truth'
                                ).compute_chunk(forecast, tru)
  np.testing.assert_array_equal(table[NAME].values[0][:, 0], 0.0)
  means = cond.conditional_means(table)[NAME]
  assert means['truth'].dims == ('time', 'bin')
  _close(means['truth'].values[0][1:4], [0.5, 1.0, 3.0])
  assert np.isnan(means['truth'].values[0][[0, 4]]).all()
  assert np.isnan(means['mse'].values[0][[0, 4]]).all()
  np.testing.assert_array_equal(means['weight'].values[0],
                                [0.0, 0.25, 0.25, 0.5, 0.0])
  bias = cond.conditional_bias(table)[NAME].values[0]
  _close(bias[1:3], [-0.5, -1.0])
  assert abs(bias[3]) <= 8 * U * 3.0
  assert np.isnan(bias[[0, 4]]).all()
  se = cond.spread_error(table)[NAME]
  _close(se['spread'].values[0][1:3], [1.0, 2.0])
  _close(se['error'].values[0][1:3], [0.5, 1.0])
  _close(se['ratio'].values[0][1:3], [2.0, 2.0])
  # debiased, M = 3: bin 1 has mse 0.25 - 1 / 3 < 0 (NaN), bin 2 1 - 4 / 3
  deb = cond.spread_error(table, debiased=True)[NAME]
  assert np.isnan(deb['error'].values[0]).all()
  deb = cond.spread_error(table, debiased=True, ensemble_size=8)[NAME]
  _close(deb['error'].values[0][1:3],
                                np.sqrt([0.25 - 1.0 / 8, 1.0 - 4.0 / 8]))
  with pytest.raises(ValueError, match='ensemble size'):
    cond.spread_error(table[NAME], debiased=True)
  with pytest.raises(ValueError, match='not a conditional table'):
    cond.marginal(xl.DataArray(np.zeros((2, 3)), ('a', 'b')))


# ---------------------------------------------------------------------------
# 4. validity and emptiness
# ---------------------------------------------------------------------------
def test_nan_points_are_invalid_and_dead_cells_are_nan():
  cols = [((0.0, 2.0), 1.0), ((0.0, 2.0), np.nan), ((np.nan, 2.0), 1.0),
          ((4.0, 6.0), 5.0)]
  forecast, tru = _columns(cols, np.float32)
  metric = cond.ConditionalTable((3.0,), by='forecast')
  off = metric.compute_chunk(forecast, tru, skipna=False)[NAME].values
  assert off.shape == (1, 5, 2) and np.isnan(off).all()
  on = metric.compute_chunk(forecast, tru, skipna=True)[NAME].values[0]
  np.testing.assert_array_equal(on[0], [0.5, 0.5])   # columns 0 and 3
  _close(on[1], [0.5, 2.5])
  _close(on[3], [1.0, 1.0])   # s2 = 2 in both
  # all points in one bin: the other is 0, not NaN
  one = cond.ConditionalTable((30.0,), by='forecast').compute_chunk(
      forecast, tru, skipna=True)[NAME].values[0]
  np.testing.assert_array_equal(one[:, 1], 0.0)
  np.testing.assert_array_equal(one[0], [1.0, 0.0])
  # a cell without valid mass is NaN with skipna on too
  dead = _columns([((0.0, np.nan), 1.0), ((0.0, 1.0), np.nan)], np.float64)
  for skipna in (False, True):
    assert np.isnan(metric.compute_chunk(*dead, skipna=skipna)[NAME].values
                    ).all()


def test_a_deterministic_forecast_is_one_member():
  ens, truth = cases.arrays(1, 2, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  edges = cases.edges('forecast', 5)
  want = cond.ConditionalTable(edges, by='forecast').compute_chunk(
      g(forecast), g(tru), skipna=True)
  flat = g(forecast).isel(realization=0)
  assert 'realization' not in flat[NAME].dims
  for metric in (cond.ConditionalTable(edges, by='forecast'),
                 cond.ConditionalTable(edges, by='truth', ensemble_dim=None)):
    got = metric.compute_chunk(flat, g(tru), skipna=True)
    assert got.attrs['ensemble_size'] == 1
    assert got[NAME].dims == ('time', 'term', 'bin')
    if metric.by == 'forecast':
      np.testing.assert_array_equal(got[NAME].values, want[NAME].values)
    # the variance is +0.0, not NaN and not -0.0
    v = got[NAME].values[:, 3]
    assert (v == 0).all() and not np.signbit(v).any()
  with pytest.raises(ValueError, match="one member.*by='spread'"):
    cond.ConditionalTable((1.0,), by='spread').compute_chunk(flat, g(tru))
  with pytest.raises(ValueError, match="one member.*by='spread'"):
    cond.ConditionalTable((1.0,), by='spread').compute_chunk(g(forecast),
                                                             g(tru))
  deb = cond.spread_error(want, debiased=True)[NAME]
  assert np.isnan(deb['error'].values).all()
  assert np.isnan(deb['ratio'].values).all()
  assert np.isfinite(cond.spread_error(want)[NAME]['error'].values).any()


# ---------------------------------------------------------------------------
# 5. the metric protocol
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
  run = lambda *args, **kwargs: cond.ConditionalTable(
      *args, **kwargs).compute_chunk(g(forecast), g(tru))
  _refuses(lambda: run((1.0,), by='error'), "by='error'")
  _refuses(lambda: run((1.0, 1.0)), 'strictly increasing')
  _refuses(lambda: run((2.0, 1.0), by='truth'), 'strictly increasing')
  _refuses(lambda: run((1.0, np.inf), by='truth'), 'finite')
  _refuses(lambda: run((np.nan,), by='forecast'), 'finite')
  _refuses(lambda: run(((1.0, 2.0),), by='truth'), '1-D')
  _refuses(lambda: run(tuple(range(64)), by='truth'), '64 bin edges.*0 to 63')
  _refuses(lambda: run((-1.0, 1.0), by='spread'), '>= 0')
  # distinct standard deviations whose squares are not: 1e-200^2 = 0 = 0^2,
  # and 1 + 2^-52 squares to the neighbour of 1 only after rounding
  _refuses(lambda: run((0.0, 1e-200), by='spread'), 'squared')
  _refuses(lambda: run((1e200, 2e200), by='spread'), 'squared')
  _refuses(lambda: run({'other': (1.0,)}, by='truth'),
           f'no entry for variable {NAME!r}')
  metric = cond.ConditionalTable((1.0,), by='truth')
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
  for n_member in (cond.MAX_MEMBERS + 1, 128):
    big = cases.datasets(*cases.arrays(n_member, 1, 5, 8, np.float32))
    _refuses(lambda: metric.compute_chunk(g(big[0]), g(big[1])),
             f'{n_member} members.*1 to 64')
  for dtype in (np.float16, np.int32):
    odd = cases.datasets(ens.astype(dtype), truth)
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
    odd = cases.datasets(ens, truth.astype(dtype))
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
  # 63 edges are taken
  assert run(tuple(range(63)), by='truth')[NAME].shape[-1] == 64
  assert run((), by='truth')[NAME].shape[-1] == 1


def test_edges_per_variable():
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32, 'member')
  forecast, tru = cases.datasets(ens, truth)
  f, t_ = g(forecast), g(tru)
  two = lambda ds: xl.Dataset({NAME: ds[NAME], 'other': ds[NAME]}, ds.coords)
  a, b = (0.5, 1.0, 1.5), (0.25, 0.75, 2.0)
  got = cond.ConditionalTable({NAME: a, 'other': b, 'unused': (1.0,)}
                              ).compute_chunk(two(f), two(t_), skipna=True)
  assert got.attrs['bin_edges'] == {NAME: a, 'other': b, 'unused': (1.0,)}
  for name, e in ((NAME, a), ('other', b)):
    want = cond.ConditionalTable(e).compute_chunk(f, t_, skipna=True)
    np.testing.assert_array_equal(got[name].values, want[NAME].values)
  assert (got[NAME].values != got['other'].values).any()
  with pytest.raises(ValueError, match='number of bins'):
    cond.ConditionalTable({NAME: a, 'other': (1.0,)}).compute_chunk(
        two(f), two(t_))


def test_compute_is_the_time_mean_of_the_chunk_tables():
  ens, truth = cases.arrays(7, 3, 5, 8, np.float32, 'truth', seed=3)
  forecast, tru = cases.datasets(ens, truth)
  metric = _metric('spread', 5)
  for skipna in (False, True):
    whole = metric.compute(g(forecast), g(tru), skipna=skipna)
    assert whole[NAME].dims == ('term', 'bin')
    assert whole.attrs == {'ensemble_size': 7, 'by': 'spread',
                           'bin_edges': cases.edges('spread', 5)}
    chunks = [metric.compute_chunk(g(forecast.isel(time=slice(k, k + 1))),
                                   g(tru.isel(time=slice(k, k + 1))),
                                   skipna=skipna)[NAME].values[0]
              for k in range(3)]
    mean = np.nanmean(chunks, axis=0) if skipna else np.mean(chunks, axis=0)
    np.testing.assert_allclose(whole[NAME].values, mean, rtol=4 * U,
                               equal_nan=True)
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               regions=regions)
  fan = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  cases.assert_same_dataset(fan, every)
  mean = metric.compute_regions(g(forecast), g(tru), regions, True)
  assert mean[NAME].dims == ('region', 'term', 'bin')
  assert mean.attrs['ensemble_size'] == 7 and mean.attrs['by'] == 'spread'


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = _metric('truth', 5)
  assert metric._fused_regions and not metric._reads_slabs_in_place
  cfg = config.Eval(metrics={'conditional': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims and da.dims[-2:] == ('term', 'bin')
  assert [d for d in da.dims if d != 'metric'][0] == 'region'
  want = metric.compute_chunk(g(forecast), g(tru), regions=regions)[NAME]
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(want.shape), want.values)
  assert list(loop['region'].values) == list(regions)


def test_bootstrap_carries_the_replicate_dim():
  ens, truth = cases.arrays(7, 6, 5, 8, np.float64, seed=4)
  forecast, tru = cases.datasets(ens, truth)
  tables = cond.ConditionalTable((1.0,), by='spread').compute_chunk(
      g(forecast), g(tru))
  assert tables[NAME].dims == ('time', 'term', 'bin')
  score = lambda t: cond.spread_error(t)['ratio']
  out = bs.bootstrap(tables, score, n_replicate=25, block_length=2, seed=2)
  counts = bs.block_plan(6, 25, 2, seed=2)
  reps = score(bs.resample_means(tables, counts))[NAME]
  assert reps.dims == (bs.REPLICATE, 'bin') and reps.shape == (25, 2)
  assert np.isfinite(reps.values).all()
  np.testing.assert_array_equal(out[NAME + '_standard_error'].values,
                                np.asarray(reps.values).std(axis=0, ddof=1))
  assert out[NAME + '_standard_error'].dims == ('bin',)
  np.testing.assert_array_equal(
      out[NAME].values,
      score(bs.resample_means(tables, np.ones((1, 6), np.int32))
            )[NAME].values[0])
  loop = bs.bootstrap(tables, score, n_replicate=25, block_length=2, seed=2,
                      vectorized=False)
  cases.assert_same_dataset(out, loop)
  # the debiased score reads the ensemble size from the resampled table
  deb = bs.bootstrap(tables, lambda t: cond.spread_error(
      t, debiased=True)['ratio'], n_replicate=5, seed=1)
  assert (deb[NAME].values > out[NAME].values).all()
  # every score keeps the leading dim; a DataArray gives the result itself
  rep = bs.resample_means(tables, counts)
  assert cond.marginal(rep)[NAME]['bias'].dims == (bs.REPLICATE,)
  assert cond.marginal(rep)['bias'][NAME].dims == (bs.REPLICATE,)
  assert cond.conditional_bias(rep)[NAME].dims == (bs.REPLICATE, 'bin')
  assert cond.conditional_means(rep[NAME])['mse'].dims == (bs.REPLICATE, 'bin')
  with pytest.raises(KeyError):
    cond.spread_error(rep)['no-such-field']


def test_pooled_at_window_one_is_the_plain_table():
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = _metric('forecast', 5)
  plain = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  pooled = pooling.Pooled(metric, neighborhoods=(1,)).compute_chunk_regions(
      g(forecast), g(tru), regions, True)
  assert pooled[NAME].dims == ('neighborhood',) + plain[NAME].dims
  np.testing.assert_array_equal(
      np.asarray(pooled[NAME].values)[0].view(np.uint64),
      np.asarray(plain[NAME].values).view(np.uint64))


# ---------------------------------------------------------------------------
# 6. the spread-error diagnostic on a reliable ensemble
# ---------------------------------------------------------------------------
def test_a_reliable_ensemble_has_a_debiased_ratio_of_one_in_every_bin():
  """20 000 points, 10 members, the truth drawn like a member, the per-point
  spread spanning a decade (tests/conditional_cases.py: `reliable`).  The
  standard error of the ratio sqrt(a / c), a = mean s2, c = mean (se - s2 / M)
  over the points of a bin, is the delta method's from the sample:
  ratio / 2 * sqrt(var(s2_i / a - c_i / c) / n)."""
  n_member = 10
  ens, truth = cases.reliable(20000, n_member, seed=3)
  n = truth.size
  edges = np.array(cases.RELIABLE_EDGES) ** 2
  sums, cnt = cond.host_sums(ens, n, n_member, None, truth, None, 1, 1, n,
                             np.zeros(n, np.int32), 1, 'spread', edges)
  table, counts = cond.host_fold(sums, cnt, [n], np.ones((1, 1)),
                                 np.ones((1, 1), np.int32))
  p = cond.normalize(table, counts, False)[0, 0]
  da = xl.DataArray(p, ('term', 'bin'))
  ratio = cond.spread_error(da, debiased=True, ensemble_size=n_member
                            )['ratio'].values
  plain = cond.spread_error(da)['ratio'].values
  mu, s2, se, valid = cnp.point_fields(ens, truth)
  which = cnp.point_bins(ens, truth, cases.RELIABLE_EDGES, 'spread')
  assert valid.all()
  held = np.bincount(which.reshape(-1), minlength=4)
  np.testing.assert_array_equal(held, cnt[0, 0, 0])
  checked = 0
  for b in range(4):
    if held[b] <= 1000:
      continue
    sel = which.reshape(-1) == b
    a_i = s2.reshape(-1)[sel]
    c_i = se.reshape(-1)[sel] - a_i / n_member
    z = a_i / a_i.mean() - c_i / c_i.mean()
    stderr = ratio[b] / 2 * np.sqrt(z.var(ddof=1) / held[b])
    assert abs(ratio[b] - 1.0) <= 4 * stderr, (b, ratio[b], stderr)
    # the plain ratio is low by sqrt(1 + 1 / M): the debiasing matters
    assert abs(plain[b] / ratio[b] - 1 / np.sqrt(1 + 1 / n_member)) < 0.01
    checked += 1
  assert checked == 2 and held[[0, 3]].sum() == 0
  assert np.isnan(ratio[[0, 3]]).all()


# ---------------------------------------------------------------------------
# 7. the engine and the C ABI refuse on the host
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_both_symbols_are_exported_and_declared(lib):
  import os
  h = lib.load()
  header = open(os.path.join(os.path.dirname(os.path.dirname(
      os.path.abspath(__file__))), 'include', 'wb2hip.h')).read()
  for name in ('wb2_conditional_sums', 'wb2_conditional_geometry'):
    assert getattr(h, name) is not None
    assert re.search(r'^int %s\(' % name, header, re.M), name
  assert 'K24' in header and 'THE ORDER OF THE SUM' in header


def test_engine_refuses_bad_tables_sizes_and_edges_on_the_host(lib):
  """Host tensors stand in for the operands: every refusal below comes from
  the host checks, before anything is uploaded or launched."""
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32)
  e, y = torch.from_numpy(ens), torch.from_numpy(truth)
  cls = cases.classes(n_col, 2)
  slab = n_row * n_col
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def sums(ens=e, stride=n_outer * slab, n_member=n_member, ens_slab=None,
           truth=y, truth_slab=None, n_outer=n_outer, cls=cls, n_class=2,
           mode='truth', edges=(0.0, 1.0)):
    return engine.conditional_sums(ens, stride, n_member, ens_slab, truth,
                                   truth_slab, n_outer, n_row, n_col, cls,
                                   n_class, mode, edges)
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
        (dict(n_member=65, stride=0), ValueError, '65 members'),
        (dict(stride=-1), ValueError, 'bad sizes'),
        (dict(n_outer=-1), ValueError, 'bad sizes'),
        (dict(mode='error'), ValueError, 'mode='),
        (dict(mode=3), ValueError, 'mode='),
        (dict(edges=(1.0, 1.0)), ValueError, 'strictly increasing'),
        (dict(edges=(1.0, 0.0)), ValueError, 'strictly increasing'),
        (dict(edges=(np.nan,)), ValueError, 'finite'),
        (dict(edges=(0.0, np.inf)), ValueError, 'finite'),
        (dict(edges=np.arange(64.0)), ValueError, '64 bin edges'),
        (dict(edges=np.zeros((2, 2))), ValueError, '1-D'),
        (dict(truth=y.double()), TypeError, 'dtype'),
        (dict(ens=e.half(), truth=y.half()), TypeError, 'dtype'),
        (dict(truth=y.transpose(-1, -2)), ValueError, 'contiguous')):
      with pytest.raises(error, match=match):
        sums(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
  with pytest.raises(ValueError, match='sums must be'):
    engine.conditional_fold(torch.zeros(1, 2, 3, 2, 3, dtype=torch.float64),
                            torch.zeros(1, 2, 3, 2, dtype=torch.int32), [4] * 3,
                            np.ones((1, 2)), np.ones((1, 3), np.int32))
  good = (torch.zeros(1, 2, 3, 2, 4, dtype=torch.float64),
          torch.zeros(1, 2, 3, 2, dtype=torch.int32))
  with pytest.raises(ValueError, match='wrow'):
    engine.conditional_fold(*good, [4] * 3, np.ones((1, 4)),
                            np.ones((1, 3), np.int32))
  with pytest.raises(ValueError, match='class_cols'):
    engine.conditional_fold(*good, [4], np.ones((1, 2)),
                            np.ones((1, 3), np.int32))


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data

  def sums(dtype=lib.WB2_F32, ens=b, n_member=5, stride=8, n_outer=2, n_row=2,
           n_col=4, n_class=2, mode=0, edges=b, n_edge=3, out=b):
    return h.wb2_conditional_sums(dtype, ens, None, b, None, n_member, stride,
                                  n_outer, n_row, n_col, b, n_class, mode,
                                  edges, n_edge, out, b, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=65), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(n_edge=-1), b'n_edge='),
      (dict(n_edge=64), b'n_edge='), (dict(mode=3), b'mode='),
      (dict(mode=-1), b'mode='), (dict(stride=-1), b'member_stride='),
      (dict(n_row=-1), b'negative'), (dict(ens=None), b'null pointer'),
      (dict(edges=None), b'null pointer'), (dict(out=None), b'null pointer')):
    assert sums(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert sums(ens=None, **empty) == 0


def test_geometry_agrees_with_the_limits_of_the_python_layer(lib):
  for dtype in (torch.float32, torch.float64):
    for m in cases.MEMBERS:
      for n_bin in cases.BINS:
        geo = engine.conditional_geometry(dtype, m, 3, n_bin - 1)
        assert (geo['min_member'], geo['max_member']) == (cond.MIN_MEMBERS,
                                                          cond.MAX_MEMBERS)
        assert geo['max_edges'] == cond.MAX_EDGES == 63
        assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
        # the formula of include/wb2hip.h
        assert geo['lds_bytes'] == 4 * 64 * 8 + 64 * 4
        assert geo['max_grid_outer'] == engine.twcrps_geometry(
            dtype)['max_grid_outer']
  assert engine.conditional_geometry(torch.float32, 1, events.MAX_CLASSES, 0)
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.conditional_geometry(torch.float32, cond.MAX_MEMBERS + 1, 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.conditional_geometry(torch.float32, 0, 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_class='):
    engine.conditional_geometry(torch.float32, 1, events.MAX_CLASSES + 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_edge='):
    engine.conditional_geometry(torch.float32, 1, 1, cond.MAX_EDGES + 1)
  with pytest.raises(TypeError):
    engine.conditional_geometry(torch.float16, 1, 1, 0)
