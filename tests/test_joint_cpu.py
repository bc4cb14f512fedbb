"""Distributions-oriented verification on the host: `distribution.JointTable`
against the dense restatement of tests/joint_np.py, its ties to the event and
the conditional tables, the scores, the metric protocol and the refusals of the
engine and the C ABI (no device needed: nothing is launched)."""
import functools
import re

import numpy as np
import pytest
import torch

from tests import helpers
from tests import joint_cases as cases
from tests import joint_np as jnp_
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import conditional as cond
from weatherbench2_amd import distribution as dist
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import neighborhood
from weatherbench2_amd import regions as greg
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = jnp_.U
GRID = (19, 72)   # every predefined region holds points
MEMBERS = (1, 2, 7)
# every member count, side and edge count; dtype and NaN pattern cycle
CASES = [(m, side, n_edge, cases.DTYPES[(a + b + c) % 2],
          cases.NANS[(a + 2 * b + c) % 4])
         for a, m in enumerate(MEMBERS)
         for b, side in enumerate(cases.SIDES)
         for c, n_edge in enumerate(cases.EDGES)]
_ID = lambda v: getattr(v, '__name__', None) or str(v)
WORST = {'fraction': 0.0}


def _table(values):
  """A joint table DataArray of a [.., B, B] array (leading dims d0, d1 ..)."""
  values = np.asarray(values, dtype=np.float64)
  lead = tuple(f'd{k}' for k in range(values.ndim - 2))
  return xl.DataArray(values, lead + (cases.TRUTH_BIN, cases.FORECAST_BIN))


@functools.lru_cache(maxsize=None)
def _case(n_member, side, n_edge, dtype, nan):
  """The arrays (values planted on the edges, +-inf), the oracle datasets and
  the product's tables (every region, both skipna) of one case: computed once,
  shared and left unchanged."""
  given = cases.edges(n_edge)
  ens, truth = cases.planted(n_member, 1, *GRID, dtype, given, nan=False,
                             seed=n_edge)
  extra = cases.arrays(n_member, 1, *GRID, dtype, nan, seed=n_edge)
  ens[np.isnan(extra[0])] = np.nan
  truth[np.isnan(extra[1])] = np.nan
  forecast, tru = cases.datasets(ens, truth)
  oregions = cases.oracle_regions()
  metric = dist.JointTable(given, side=side)
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, oregions, tables


# ---------------------------------------------------------------------------
# 1. the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_member,side,n_edge,dtype,nan', CASES, ids=_ID)
def test_host_path_equals_the_dense_restatement(n_member, side, n_edge, dtype,
                                                nan):
  ens, truth, forecast, tru, oregions, tables = _case(n_member, side, n_edge,
                                                      dtype, nan)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  given = cases.edges(n_edge)
  n_bin = n_edge + 1
  # the counts: equal
  col_class, mult, wrow = events.column_classes(
      cases.product_regions(oregions), lat, lon)
  n_class = mult.shape[1]
  cnt = dist.host_counts(ens, truth.size, n_member, None, truth, None, 1,
                         *GRID, col_class, n_class, given, side)
  assert cnt.dtype == np.int32
  assert cnt.shape == (1,) + (GRID[0], n_class, n_bin * n_bin + 1)
  want = jnp_.dense_counts(ens, truth, col_class, n_class, given, side)
  np.testing.assert_array_equal(cnt, want)
  # the valid codes of a (row, class) sum to M x its valid points
  ok = jnp_.valid_points(ens, truth)[0]
  for c in range(n_class):
    np.testing.assert_array_equal(cnt[0, :, c, :-1].sum(axis=-1),
                                  n_member * ok[:, col_class == c].sum(axis=1))
  # planted values: some truth and some member lie exactly on an edge
  if n_edge:
    assert np.isin(truth[ok[None]], given).any()
    assert np.isinf(truth).any() and np.isinf(ens).any()
  rtol = jnp_.table_rtol(GRID[0], n_class)
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'time', cases.TRUTH_BIN, cases.FORECAST_BIN)
    assert da.dtype == np.float64 and da.shape[-2:] == (n_bin, n_bin)
    assert got.attrs == {'ensemble_size': n_member, 'bin_edges': given,
                         'side': side}
    assert list(got['region'].values) == list(oregions)
    for dim in (cases.TRUTH_BIN, cases.FORECAST_BIN):
      np.testing.assert_array_equal(got[dim].values, np.arange(n_bin))
      assert got[dim].values.dtype == np.int64
    for r, (name, region) in enumerate(oregions.items()):
      w = _oracle_region_weights(region, lat, lon)
      want = jnp_.dense_table(ens, truth, w, given, side, skipna)
      msg = f'{name} skipna={skipna}'
      np.testing.assert_array_equal(np.isnan(da.values[r]), np.isnan(want),
                                    err_msg=msg)
      live = ~np.isnan(want)
      # a category pair without a point is exactly 0
      np.testing.assert_array_equal(da.values[r][live] == 0, want[live] == 0,
                                    err_msg=msg)
      err = np.abs(da.values[r] - want)[live & (want > 0)] / want[
          live & (want > 0)]
      if err.size:
        WORST['fraction'] = max(WORST['fraction'], err.max() / rtol)
        print(f'{msg}: worst relative error {err.max() / U:.2f} u, '
              f'{err.max() / rtol:.3f} of the bound')
        assert err.max() <= rtol, msg
      # a live cell sums to 1
      if live.any():
        total = da.values[r].reshape(1, -1).sum(axis=-1)
        np.testing.assert_allclose(total, 1.0, rtol=0,
                                   atol=(n_bin * n_bin + rtol / U) * U)
    if nan == 'none':
      assert np.isfinite(da.values[0]).all()
    elif not skipna:
      assert np.isnan(da.values[0]).any()
  # one region alone is that slice of the fused pass within twice the bound
  # (other column classes, the same integers)
  metric = dist.JointTable(given, side=side)
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


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_values_on_an_edge_and_infinities(dtype):
  """One row by hand: edges (0, 1); truth and the single member step through
  below, on and above them and +-inf."""
  vals = np.array([-np.inf, -0.5, 0.0, 0.5, 1.0, 1.5, np.inf], dtype)
  n = vals.size
  ens = np.tile(vals, n).reshape(1, 1, 1, n * n)       # member: fast index
  truth = np.repeat(vals, n).reshape(1, 1, n * n)      # truth: slow index
  want_bin = {'right': [0, 0, 1, 1, 2, 2, 2], 'left': [0, 0, 0, 1, 1, 2, 2]}
  for side in cases.SIDES:
    cnt = dist.host_counts(ens, n * n, 1, None, truth, None, 1, 1, n * n,
                           np.zeros(n * n, np.int32), 1, (0.0, 1.0), side)
    want = np.zeros((3, 3), np.int64)
    for a in want_bin[side]:
      for b in want_bin[side]:
        want[a, b] += 1
    np.testing.assert_array_equal(cnt[0, 0, 0, :9].reshape(3, 3), want)
    assert cnt[0, 0, 0, 9] == 0
    np.testing.assert_array_equal(
        dist.host_bins(vals.astype(np.float64), (0.0, 1.0), side),
        want_bin[side])
    np.testing.assert_array_equal(
        jnp_.point_bins(vals, (0.0, 1.0), side), want_bin[side])


def test_nan_points_are_invalid_and_dead_cells_are_nan():
  ens, truth = cases.arrays(3, 2, 5, 8, np.float32)
  truth[0, 2, 3] = np.nan      # time 0: one invalid point
  ens[1, 1] = np.nan           # time 1: no valid point at all
  forecast, tru = cases.datasets(ens, truth)
  metric = dist.JointTable((0.0,))
  strict = metric.compute_chunk(g(forecast), g(tru))[NAME].values
  lax = metric.compute_chunk(g(forecast), g(tru), skipna=True)[NAME].values
  assert np.isnan(strict).all()
  assert np.isfinite(lax[0]).all() and np.isnan(lax[1]).all()
  np.testing.assert_allclose(lax[0].sum(), 1.0, rtol=8 * U)


def test_a_deterministic_forecast_is_one_member():
  ens, truth = cases.arrays(1, 2, 5, 8, np.float64, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  plain = g(forecast).isel(realization=0)
  for metric in (dist.JointTable((-0.5, 0.5)),
                 dist.JointTable((-0.5, 0.5), ensemble_dim=None)):
    got = metric.compute_chunk(plain, g(tru), skipna=True)
    assert got.attrs['ensemble_size'] == 1
    want = dist.JointTable((-0.5, 0.5)).compute_chunk(g(forecast), g(tru),
                                                      skipna=True)
    np.testing.assert_array_equal(got[NAME].values, want[NAME].values)


# ---------------------------------------------------------------------------
# 2. the ties to the event table (K18) and the conditional table (K24)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_member', (1, 7))
def test_left_sided_counts_collapse_to_the_event_counts(n_member):
  n_outer, n_row, n_col = 2, 5, 8
  given = cases.edges(8)
  n_bin = len(given) + 1
  ens, truth = cases.planted(n_member, n_outer, n_row, n_col, np.float32,
                             given, seed=n_member)
  cls = cases.rotated(n_col, 3)
  front = (ens, truth.size, n_member, None, truth, None)
  cnt = dist.host_counts(*front, n_outer, n_row, n_col, cls, 3, given, 'left')
  joint = cnt[..., :-1].reshape(cnt.shape[:-1] + (n_bin, n_bin)).astype(
      np.int64)
  for k, edge in enumerate(given):
    thr = np.full(truth.shape, edge, np.float32)
    ev = events.host_counts(*front, [thr], None, n_outer, n_row, n_col, cls, 3
                            )[0].astype(np.int64)
    np.testing.assert_array_equal(ev[..., -1], cnt[..., -1])  # invalid
    ev = ev[..., :-1].reshape(ev.shape[:-1] + (2, n_member + 1))
    lo, hi = slice(0, k + 1), slice(k + 1, n_bin)
    two = np.stack([
        np.stack([joint[..., lo, lo].sum((-1, -2)),
                  joint[..., lo, hi].sum((-1, -2))], -1),
        np.stack([joint[..., hi, lo].sum((-1, -2)),
                  joint[..., hi, hi].sum((-1, -2))], -1)], -2)
    members = np.arange(n_member + 1)
    if n_member == 1:
      np.testing.assert_array_equal(two, ev)       # the 2 x 2 table itself
    # the forecast-above column: sum_k k cnt[obs][k]; the other M - k
    np.testing.assert_array_equal(two[..., 1], (ev * members).sum(-1))
    np.testing.assert_array_equal(two[..., 0],
                                  (ev * (n_member - members)).sum(-1))
  assert joint.sum() > 0


def test_collapse_equals_the_contingency_table_of_the_event():
  """A deterministic forecast, side='left': `collapse(table, k)` against
  `events.contingency` of `EventTable(ConstantThreshold(edge_k))`.  Either side
  is within (2 n_row + 2) u of the exact frequency (tests/joint_np.py; the
  event table divides by a sequential sum of 4 codes: 2 more) and a quadrant
  sums at most B * B terms."""
  n_row, n_col = 5, 8
  given = cases.edges(8)
  ens, truth = cases.planted(1, 2, n_row, n_col, np.float64, given, seed=5)
  forecast, tru = cases.datasets(ens, truth)
  f = g(forecast).isel(realization=0)
  table = dist.JointTable(given, side='left').compute_chunk(f, g(tru),
                                                            skipna=True)
  rtol = (2 * (2 * n_row + 2) + 2 + (len(given) + 1) ** 2) * U
  for k, edge in enumerate(given):
    ev = events.EventTable(thresholds=[neighborhood.ConstantThreshold(edge)]
                           ).compute_chunk(f, g(tru), skipna=True)
    want = events.contingency(ev)[NAME]
    two = dist.collapse(table, k)
    assert two[NAME].dims == ('time', events.OBSERVED, events.EXCEEDING)
    got = events.contingency(two)[NAME]
    for field in ('hits', 'false_alarms', 'misses', 'correct_negatives'):
      np.testing.assert_allclose(got[field].values, want[field].values[0],
                                 rtol=rtol, atol=0)
  with pytest.raises(ValueError, match='edge_index'):
    dist.collapse(table, len(given))


def test_truth_marginal_is_the_conditional_tables_weight():
  """side='right' is `ConditionalTable`'s binning: the truth histogram against
  the `weight` of `ConditionalTable(by='truth')`.  The joint side: every p
  within (2 n_row + 2) u, B of them added (B - 1); the conditional side
  (tests/conditional_np.py): a bin's mass n_row u, the valid mass (n_row + B -
  1) u, the division u."""
  n_row, n_col = 5, 8
  given = cases.edges(8)
  n_bin = len(given) + 1
  # (values on the 0.25 grid of the edges; the conditional table does not pin
  # +-inf, so none is planted)
  ens, truth = cases.arrays(7, 2, n_row, n_col, np.float32, 'both', seed=2)
  assert np.isin(truth, given).any()
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  table = dist.JointTable(given).compute_chunk(g(forecast), g(tru),
                                               skipna=True, regions=regions)
  weight = cond.ConditionalTable(given, by='truth').compute_chunk(
      g(forecast), g(tru), skipna=True, regions=regions)[NAME].values[..., 0, :]
  got = dist.marginals(table)[NAME]['truth']
  assert got.dims == ('region', 'time', 'bin')
  rtol = ((2 * n_row + 2 + n_bin - 1) + (2 * n_row + n_bin)) * U
  np.testing.assert_allclose(got.values, weight, rtol=rtol, atol=0,
                             equal_nan=True)
  assert np.isfinite(weight).any()


# ---------------------------------------------------------------------------
# 3. the scores
# ---------------------------------------------------------------------------
def _all_scores(table):
  return {'pc': dist.proportion_correct(table), 'heidke': dist.heidke(table),
          'peirce': dist.peirce(table), 'gerrity': dist.gerrity(table),
          'overlap': dist.histogram_overlap(table),
          'mi': dist.mutual_information(table)}


def test_a_perfect_forecast_scores_one():
  p = np.diag([0.2, 0.5, 0.25, 0.05])
  s = _all_scores(_table(p))
  for name in ('pc', 'heidke', 'peirce', 'gerrity', 'overlap'):
    np.testing.assert_allclose(s[name].values, 1.0, rtol=8 * U, err_msg=name)
  # the mutual information of a perfect forecast is the entropy of the truth
  h = -(np.diag(p) * np.log(np.diag(p))).sum()
  np.testing.assert_allclose(s['mi'].values, h, rtol=8 * U)
  np.testing.assert_array_equal(dist.frequency_bias(_table(p)).values, 1.0)


def test_independent_marginals_score_zero():
  pt = np.array([0.1, 0.4, 0.3, 0.2])
  pf = np.array([0.25, 0.25, 0.4, 0.1])
  p = pt[:, None] * pf[None, :]
  s = _all_scores(_table(p))
  for name in ('heidke', 'peirce', 'gerrity', 'mi'):
    assert abs(s[name].values) <= 16 * U, name
  m = dist.marginals(_table(p))
  np.testing.assert_allclose(m['forecast'].values, pf, rtol=4 * U)
  np.testing.assert_allclose(m['truth'].values, pt, rtol=4 * U)
  np.testing.assert_allclose(dist.frequency_bias(_table(p)).values, pf / pt,
                             rtol=8 * U)
  np.testing.assert_allclose(s['overlap'].values,
                             np.minimum(pf, pt).sum(), rtol=8 * U)


def test_gerrity_is_peirce_for_two_categories():
  rs = np.random.RandomState(0)
  p = rs.rand(6, 2, 2)
  p /= p.sum(axis=(1, 2), keepdims=True)
  # (both are differences of terms of order 1: an absolute tolerance)
  np.testing.assert_allclose(dist.gerrity(_table(p)).values,
                             dist.peirce(_table(p)).values, rtol=0,
                             atol=64 * U)


def test_gerrity_on_a_hand_computed_table():
  """p = [[.30 .10 .00] [.10 .20 .10] [.00 .05 .15]], truth marginal (.4, .4,
  .2): P_1 = .4, P_2 = .8, a_1 = .6 / .4 = 3/2, a_2 = .2 / .8 = 1/4, b = 1/2.
    s_11 = (a_1 + a_2) / 2             = (3/2 + 1/4) / 2         = 7/8
    s_22 = (1/a_1 + a_2) / 2           = (2/3 + 1/4) / 2         = 11/24
    s_33 = (1/a_1 + 1/a_2) / 2         = (2/3 + 4) / 2           = 7/3
    s_12 = (a_2 - 1) / 2               = -3/8
    s_13 = (-2) / 2                    = -1
    s_23 = (1/a_1 - 1) / 2             = -1/6
  score = .30 * 7/8 + .20 * 11/24 + .15 * 7/3 + (.10 + .10) * (-3/8)
          + 0 * (-1) + (.10 + .05) * (-1/6)
        = .2625 + .091666.. + .35 - .075 - .025 = .604166.. = 29/48."""
  p = np.array([[0.30, 0.10, 0.00], [0.10, 0.20, 0.10], [0.00, 0.05, 0.15]])
  s = dist.gerrity_matrix(p.sum(axis=1))
  want = np.array([[7 / 8, -3 / 8, -1.0], [-3 / 8, 11 / 24, -1 / 6],
                   [-1.0, -1 / 6, 7 / 3]])
  np.testing.assert_allclose(s, want, rtol=16 * U)
  np.testing.assert_allclose(dist.gerrity(_table(p)).values, 29 / 48,
                             rtol=16 * U)
  # one category: no score; a truth category that never occurs: a_r = inf or 0
  assert np.isnan(dist.gerrity(_table([[1.0]])).values)
  empty = np.array([[0.0, 0.0, 0.0], [0.2, 0.3, 0.1], [0.1, 0.1, 0.2]])
  assert np.isnan(dist.gerrity(_table(empty)).values)
  last = np.array([[0.2, 0.3, 0.1], [0.1, 0.1, 0.2], [0.0, 0.0, 0.0]])
  assert np.isnan(dist.gerrity(_table(last)).values)


def test_conditional_distributions_sum_to_one_and_zero_over_zero_is_nan():
  rs = np.random.RandomState(1)
  p = rs.rand(4, 5, 5)
  p /= p.sum(axis=(1, 2), keepdims=True)
  like = dist.conditional_distribution(_table(p), 'truth')
  cal = dist.conditional_distribution(_table(p), given='forecast')
  assert like.dims == cal.dims == ('d0', cases.TRUTH_BIN, cases.FORECAST_BIN)
  np.testing.assert_allclose(like.values.sum(axis=-1), 1.0, rtol=8 * U)
  np.testing.assert_allclose(cal.values.sum(axis=-2), 1.0, rtol=8 * U)
  np.testing.assert_allclose(like.values * p.sum(axis=-1)[..., None], p,
                             rtol=4 * U)
  with pytest.raises(ValueError, match='given='):
    dist.conditional_distribution(_table(p), 'neither')
  # equal marginals overlap fully
  sym = p + np.swapaxes(p, -1, -2)
  np.testing.assert_allclose(
      dist.histogram_overlap(_table(sym / 2)).values, 1.0, rtol=8 * U)
  # every 0/0 is NaN: an empty truth category and an empty forecast category
  q = np.array([[0.5, 0.0, 0.1], [0.0, 0.0, 0.0], [0.2, 0.0, 0.2]])
  assert np.isnan(dist.conditional_distribution(_table(q), 'truth'
                                                ).values[1]).all()
  assert np.isnan(dist.conditional_distribution(_table(q), 'forecast'
                                                ).values[:, 1]).all()
  assert np.isnan(dist.frequency_bias(_table(q)).values[1])
  one = _table([[1.0, 0.0], [0.0, 0.0]])   # a constant field, always right
  assert np.isnan(dist.heidke(one).values)
  assert np.isnan(dist.peirce(one).values)
  assert dist.mutual_information(one).values == 0.0   # 0 log 0 = 0
  dead = _table(np.full((3, 3), np.nan))
  for name, v in _all_scores(dead).items():
    assert np.isnan(v.values), name
  with pytest.raises(ValueError, match='not a joint table'):
    dist.heidke(xl.DataArray(p, ('a', 'b', 'c')))
  with pytest.raises(ValueError, match='not a joint table'):
    dist.heidke(_table(p[:, :3]))


# ---------------------------------------------------------------------------
# 4. the metric protocol: time mean, bootstrap, Eval, Pooled
# ---------------------------------------------------------------------------
def test_compute_is_the_table_of_the_pooled_points():
  """No NaN, so every time holds the same valid mass and the time mean of the
  tables is the table of all points.  Every chunk table is within (2 n_row +
  2) u of its exact value, the mean of T of them adds T u, the restatement 3 u
  (tests/joint_np.py)."""
  n_time, n_row, n_col = 3, 5, 8
  given = cases.edges(8)
  ens, truth = cases.arrays(7, n_time, n_row, n_col, np.float32, seed=3)
  forecast, tru = cases.datasets(ens, truth)
  metric = dist.JointTable(given, side='left')
  whole = metric.compute(g(forecast), g(tru))
  assert whole[NAME].dims == (cases.TRUTH_BIN, cases.FORECAST_BIN)
  assert whole.attrs == {'ensemble_size': 7, 'bin_edges': given,
                         'side': 'left'}
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  w = np.tile(_oracle_region_weights(None, lat, lon), (n_time, 1))
  want = jnp_.dense_table(ens.reshape(7, 1, n_time * n_row, n_col),
                          truth.reshape(1, n_time * n_row, n_col), w, given,
                          'left', False)[0]
  np.testing.assert_allclose(whole[NAME].values, want,
                             rtol=(2 * n_row + n_time + 5) * U, atol=0)
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
  assert mean[NAME].dims == ('region', cases.TRUTH_BIN, cases.FORECAST_BIN)
  assert mean.attrs['side'] == 'left' and mean.attrs['ensemble_size'] == 7


def test_bootstrap_and_every_score_carry_the_replicate_dim():
  ens, truth = cases.arrays(7, 6, 5, 8, np.float64, seed=4)
  forecast, tru = cases.datasets(ens, truth)
  tables = dist.JointTable((-0.5, 0.5)).compute_chunk(g(forecast), g(tru))
  assert tables[NAME].dims == ('time', cases.TRUTH_BIN, cases.FORECAST_BIN)
  out = bs.bootstrap(tables, dist.heidke, n_replicate=25, block_length=2,
                     seed=2)
  counts = bs.block_plan(6, 25, 2, seed=2)
  rep = bs.resample_means(tables, counts)
  reps = dist.heidke(rep)[NAME]
  assert reps.dims == (bs.REPLICATE,) and reps.shape == (25,)
  assert np.isfinite(reps.values).all()
  np.testing.assert_array_equal(out[NAME + '_standard_error'].values,
                                np.asarray(reps.values).std(axis=0, ddof=1))
  loop = bs.bootstrap(tables, dist.heidke, n_replicate=25, block_length=2,
                      seed=2, vectorized=False)
  cases.assert_same_dataset(out, loop)
  # every function keeps the leading dim; a DataArray gives the result itself
  lead = (bs.REPLICATE,)
  assert dist.marginals(rep)[NAME]['truth'].dims == lead + ('bin',)
  assert dist.marginals(rep)['forecast'][NAME].dims == lead + ('bin',)
  assert dist.frequency_bias(rep)[NAME].dims == lead + ('bin',)
  for fn in (dist.histogram_overlap, dist.proportion_correct, dist.peirce,
             dist.gerrity, dist.mutual_information):
    assert fn(rep)[NAME].dims == lead, fn.__name__
    assert fn(rep[NAME]).dims == lead, fn.__name__
  both = (cases.TRUTH_BIN, cases.FORECAST_BIN)
  assert dist.conditional_distribution(rep, 'forecast')[NAME].dims == (
      lead + both)
  assert dist.collapse(rep, 1)[NAME].dims == lead + (events.OBSERVED,
                                                     events.EXCEEDING)


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = dist.JointTable(cases.edges(8))
  assert metric._fused_regions and not metric._reads_slabs_in_place
  cfg = config.Eval(metrics={'joint': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims
  assert da.dims[-2:] == (cases.TRUTH_BIN, cases.FORECAST_BIN)
  assert [d for d in da.dims if d != 'metric'][0] == 'region'
  want = metric.compute_chunk(g(forecast), g(tru), regions=regions)[NAME]
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(want.shape), want.values)
  assert list(loop['region'].values) == list(regions)


def test_pooled_at_window_one_is_the_plain_table():
  from weatherbench2_amd import pooling
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = dist.JointTable(cases.edges(8))
  plain = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  pooled = pooling.Pooled(metric, neighborhoods=(1,)).compute_chunk_regions(
      g(forecast), g(tru), regions, True)
  assert pooled[NAME].dims == ('neighborhood',) + plain[NAME].dims
  np.testing.assert_array_equal(
      np.asarray(pooled[NAME].values)[0].view(np.uint64),
      np.asarray(plain[NAME].values).view(np.uint64))


def test_edges_per_variable():
  ens, truth = cases.arrays(7, 2, 5, 8, np.float32, 'member')
  forecast, tru = cases.datasets(ens, truth)
  f, t_ = g(forecast), g(tru)
  two = lambda ds: xl.Dataset({NAME: ds[NAME], 'other': ds[NAME]}, ds.coords)
  a, b = (-0.5, 0.0, 0.5), (-0.25, 0.75, 2.0)
  got = dist.JointTable({NAME: a, 'other': b, 'unused': (1.0,)}
                        ).compute_chunk(two(f), two(t_), skipna=True)
  assert got.attrs['bin_edges'] == {NAME: a, 'other': b, 'unused': (1.0,)}
  for name, e in ((NAME, a), ('other', b)):
    want = dist.JointTable(e).compute_chunk(f, t_, skipna=True)
    np.testing.assert_array_equal(got[name].values, want[NAME].values)
  assert (got[NAME].values != got['other'].values).any()
  with pytest.raises(ValueError, match='number of categories'):
    dist.JointTable({NAME: a, 'other': (1.0,)}).compute_chunk(two(f), two(t_))


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
  run = lambda *args, **kwargs: dist.JointTable(
      *args, **kwargs).compute_chunk(g(forecast), g(tru))
  _refuses(lambda: run((1.0,), side='middle'), "side='middle'")
  _refuses(lambda: run((1.0, 1.0)), 'strictly increasing')
  _refuses(lambda: run((2.0, 1.0)), 'strictly increasing')
  _refuses(lambda: run((1.0, np.inf)), 'finite')
  _refuses(lambda: run((np.nan,)), 'finite')
  _refuses(lambda: run(((1.0, 2.0),)), '1-D')
  _refuses(lambda: run(('a',)), 'numbers')
  _refuses(lambda: run(tuple(range(32))), '32 bin edges.*0 to 31')
  _refuses(lambda: run({'other': (1.0,)}),
           f'no entry for variable {NAME!r}')
  metric = dist.JointTable((1.0,))
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
  big = cases.datasets(*cases.arrays(dist.MAX_MEMBERS + 1, 1, 5, 8,
                                     np.float32))
  _refuses(lambda: metric.compute_chunk(g(big[0]), g(big[1])),
           f'{dist.MAX_MEMBERS + 1} members.*1 to 128')
  for dtype in (np.float16, np.int32):
    odd = cases.datasets(ens.astype(dtype), truth)
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
    odd = cases.datasets(ens, truth.astype(dtype))
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
  # 31 edges, 128 members and no edge at all are taken
  assert run(tuple(range(31)))[NAME].shape[-2:] == (32, 32)
  assert run(())[NAME].shape[-2:] == (1, 1)
  full = cases.datasets(*cases.arrays(128, 1, 5, 8, np.float32))
  assert metric.compute_chunk(g(full[0]), g(full[1])).attrs[
      'ensemble_size'] == 128


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
  for name in ('wb2_joint_counts', 'wb2_joint_counts_geometry'):
    assert getattr(h, name) is not None
    assert re.search(r'^int %s\(' % name, header, re.M), name
  assert 'K26' in header and 'The fold: wb2_event_fold with n_code' in header


def test_engine_refuses_bad_tables_sizes_and_edges_on_the_host(lib):
  """Host tensors stand in for the operands: every refusal below comes from
  the host checks, before anything is uploaded or launched."""
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32)
  e, y = torch.from_numpy(ens), torch.from_numpy(truth)
  cls = cases.rotated(n_col, 2)
  slab = n_row * n_col
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def counts(ens=e, stride=n_outer * slab, n_member=n_member, ens_slab=None,
             truth=y, truth_slab=None, n_outer=n_outer, cls=cls, n_class=2,
             edges=(0.0, 1.0), side='right'):
    return engine.joint_counts(ens, stride, n_member, ens_slab, truth,
                               truth_slab, n_outer, n_row, n_col, cls, n_class,
                               edges, side)
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
        (dict(side='middle'), ValueError, 'side='),
        (dict(side=2), ValueError, 'side='),
        (dict(edges=(1.0, 1.0)), ValueError, 'strictly increasing'),
        (dict(edges=(1.0, 0.0)), ValueError, 'strictly increasing'),
        (dict(edges=(np.nan,)), ValueError, 'finite'),
        (dict(edges=(0.0, np.inf)), ValueError, 'finite'),
        (dict(edges=np.arange(32.0)), ValueError, '32 bin edges'),
        (dict(edges=np.zeros((2, 2))), ValueError, '1-D'),
        (dict(truth=y.double()), TypeError, 'dtype'),
        (dict(ens=e.half(), truth=y.half()), TypeError, 'dtype'),
        (dict(truth=y.transpose(-1, -2)), ValueError, 'contiguous'),
        # 64 classes x 32 categories: not even one row fits the LDS budget
        (dict(n_class=64, edges=np.arange(31.0)), lib.Wb2HipError,
         'LDS budget')):
      with pytest.raises(error, match=match):
        counts(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
  with pytest.raises(ValueError, match='cnt must be'):
    engine.joint_fold(torch.zeros(1, 2, 3, 5, dtype=torch.float64),
                      np.ones((1, 2)), np.ones((1, 3), np.int32))
  with pytest.raises(ValueError, match='wrow'):
    engine.joint_fold(torch.zeros(1, 2, 3, 5, dtype=torch.int32),
                      np.ones((1, 4)), np.ones((1, 3), np.int32))


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data

  def counts(dtype=lib.WB2_F32, ens=b, n_member=5, stride=8, n_outer=2,
             n_row=2, n_col=4, n_class=2, edges=b, n_edge=3, side=0, out=b):
    return h.wb2_joint_counts(dtype, ens, None, b, None, n_member, stride,
                              n_outer, n_row, n_col, b, n_class, edges, n_edge,
                              side, out, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=129), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(n_edge=-1), b'n_edge='),
      (dict(n_edge=32), b'n_edge='), (dict(side=2), b'side='),
      (dict(side=-1), b'side='), (dict(stride=-1), b'member_stride='),
      (dict(n_row=-1), b'negative'), (dict(ens=None), b'null pointer'),
      (dict(edges=None), b'null pointer'), (dict(out=None), b'null pointer'),
      (dict(n_class=64, n_edge=31), b'LDS budget'),
      (dict(n_col=1 << 28), b'too long')):
    assert counts(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert counts(ens=None, **empty) == 0
  # no edge needs no edge array
  assert counts(edges=None, n_edge=0, n_outer=0) == 0


def test_geometry_values_and_the_lds_refusal(lib):
  h = lib.load()
  for dtype in (torch.float32, torch.float64):
    for n_member in (1, 50, 128):
      for n_class, n_edge, rows in ((1, 0, 4), (13, 9, 4), (3, 31, 4),
                                    (8, 31, 1), (15, 31, 1), (64, 1, 4),
                                    (64, 10, 2), (64, 14, 1), (16, 31, None),
                                    (64, 31, None)):
        n_code = (n_edge + 1) ** 2 + 1
        if rows is None:
          with pytest.raises(lib.Wb2HipError, match='LDS budget') as ei:
            engine.joint_geometry(dtype, n_member, n_class, n_edge)
          # the counting call says the same
          b = np.zeros(8, np.int64).ctypes.data
          assert h.wb2_joint_counts(
              engine.dtype_code(dtype), b, None, b, None, n_member, 8, 1, 1, 4,
              b, n_class, b, n_edge, 0, b, None) < 0
          assert h.wb2_last_error().decode() in str(ei.value)
          continue
        for wide in (False, True):
          geo = engine.joint_geometry(dtype, n_member, n_class, n_edge, wide)
          assert geo['rows_per_group'] == rows, (n_class, n_edge)
          # the formula of include/wb2hip.h, within K18's budget
          assert geo['lds_bytes'] == rows * n_class * n_code * 4 <= 65536
          assert rows == 4 or 2 * rows * n_class * n_code * 4 > 65536
          assert geo['max_edges'] == dist.MAX_EDGES == 31
          assert geo['max_grid_outer'] == engine.event_counts_geometry(
              dtype, 1, 1, 1)['max_grid_outer']
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.joint_geometry(torch.float32, dist.MAX_MEMBERS + 1, 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.joint_geometry(torch.float32, 0, 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_class='):
    engine.joint_geometry(torch.float32, 1, events.MAX_CLASSES + 1, 0)
  with pytest.raises(lib.Wb2HipError, match='n_edge='):
    engine.joint_geometry(torch.float32, 1, 1, dist.MAX_EDGES + 1)
  with pytest.raises(TypeError):
    engine.joint_geometry(torch.float16)
  null = h.wb2_joint_counts_geometry(lib.WB2_F32, 1, 1, 0, 0, None, None,
                                     None, None)
  assert null < 0 and b'null pointer' in h.wb2_last_error()
