"""Quantile and interval verification on the host:
`quantile_scores.QuantileScoreTable` against the dense restatement of
tests/quantile_score_np.py, its identities, the scores, the metric protocol
and the refusals of the engine and the C ABI (no device needed: nothing is
launched)."""
import functools
import math
import re

import numpy as np
import pytest
import torch

from tests import helpers
from tests import quantile_np
from tests import quantile_score_cases as cases
from tests import quantile_score_np as qnp
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import quantile_scores as qs
from weatherbench2_amd import regions as greg
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = qnp.U
MEMBERS = (1, 2, 7, 33)
# every grid, member count and method; dtype, NaNs and the field cycle
CASES = [(grid, m, method, cases.DTYPES[(a + b + c) % 2],
          ('none', 'truth', 'member', 'both')[(a + 2 * b + c) % 4],
          'precip' if (a + b) % 2 else 'normal')
         for a, grid in enumerate(cases.GRIDS)
         for b, m in enumerate(MEMBERS)
         for c, method in enumerate(cases.METHODS)]
_ID = lambda v: ('x'.join(map(str, v)) if isinstance(v, tuple) else
                 getattr(v, '__name__', None) or str(v))
LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
WORST = {'fraction': 0.0}


@pytest.fixture(scope='module', autouse=True)
def lib():
  """The built library, before any test of this module: the engine's
  geometry calls need it, whichever test runs first."""
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


@functools.lru_cache(maxsize=None)
def _case(grid, n_member, method, dtype, nan, kind):
  """The arrays, the oracle datasets and the product's tables (every region,
  both skipna) of one case: computed once, shared and left unchanged."""
  ens, truth = cases.arrays(n_member, 1, *grid, dtype, nan=nan,
                            seed=grid[1] + n_member, kind=kind)
  forecast, tru = cases.datasets(ens, truth)
  oregions = cases.oracle_regions()
  metric = qs.QuantileScoreTable(LEVELS, method=method)
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, oregions, tables


# ---------------------------------------------------------------------------
# 1. the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('grid,n_member,method,dtype,nan,kind', CASES, ids=_ID)
def test_host_path_equals_the_dense_restatement(grid, n_member, method, dtype,
                                                nan, kind):
  ens, truth, forecast, tru, oregions, tables = _case(grid, n_member, method,
                                                      dtype, nan, kind)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  n_level = len(LEVELS)
  col_class, mult, wrow = events.column_classes(
      cases.product_regions(oregions), lat, lon)
  n_class = mult.shape[1]
  level_tables = engine.quantile_score_levels(LEVELS, n_member, method)
  sums, cnt, valid = qs.host_sums(ens, truth.size, n_member, None, truth, None,
                                  1, *grid, col_class, n_class, level_tables)
  assert sums.dtype == np.float64
  assert cnt.dtype == np.int32 and valid.dtype == np.int32
  assert sums.shape == cnt.shape == (1, grid[0], n_class, n_level, 2)
  assert valid.shape == (1, grid[0], n_class, 2)
  # the counts: equal
  want_cnt, want_valid = qnp.dense_counts(ens, truth, col_class, n_class,
                                          LEVELS, method)
  np.testing.assert_array_equal(cnt, want_cnt)
  np.testing.assert_array_equal(valid, want_valid)
  np.testing.assert_array_equal(
      valid.sum(axis=-1)[0], np.broadcast_to(
          np.bincount(col_class, minlength=n_class), (grid[0], n_class)))
  # the pinball sums are non-negative; no -0.0 anywhere
  assert (sums[..., 0] >= 0).all() and not np.signbit(sums[sums == 0]).any()
  if kind == 'precip' and n_member > 1:
    assert cnt[..., 1].sum() > 0   # ties at zero
  rtol = qnp.table_rtol(*grid, n_class)
  assert rtol <= qnp.worst_case_rtol(*grid, n_class) or grid[0] <= 2
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'time', cases.TERM, cases.LEVEL)
    assert da.dtype == np.float64 and da.shape[-2:] == (4, n_level)
    assert got.attrs == {'ensemble_size': n_member, 'method': method,
                         'levels': LEVELS}
    assert list(got['region'].values) == list(oregions)
    assert list(got[cases.TERM].values) == list(cases.TERMS)
    np.testing.assert_array_equal(got[cases.LEVEL].values, np.array(LEVELS))
    assert got[cases.LEVEL].values.dtype == np.float64
    for r, (name, region) in enumerate(oregions.items()):
      w = _oracle_region_weights(region, lat, lon)
      want, scale = qnp.dense_table(ens, truth, w, LEVELS, method, skipna)
      msg = f'{name} skipna={skipna}'
      np.testing.assert_array_equal(np.isnan(da.values[r]), np.isnan(want),
                                    err_msg=msg)
      live = ~np.isnan(want)
      # what is exactly zero on one side is so on the other
      np.testing.assert_array_equal((da.values[r] == 0)[live & (scale == 0)],
                                    True, err_msg=msg)
      pos = live & (scale > 0)
      err = np.abs(da.values[r] - want)[pos] / scale[pos]
      if err.size:
        WORST['fraction'] = max(WORST['fraction'], err.max() / rtol)
        assert err.max() <= rtol, (msg, err.max() / U)
    whole = list(oregions).index('global')
    if nan == 'none':
      assert np.isfinite(da.values[whole]).all()
    elif not skipna and np.isnan(truth).any() | np.isnan(ens).any():
      assert np.isnan(da.values[whole]).all()


def test_the_worst_fraction_of_the_bound_is_reported():
  # (after the cases above in file order; a lone run has nothing to report)
  print(f"worst observed fraction of table_rtol: {WORST['fraction']:.3f}")
  assert WORST['fraction'] <= 1.0


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', (1, 2, 7, 33))
def test_linear_quantile_is_bit_equal_to_the_quantile_kernels_restatement(
    dtype, n_member):
  ens, truth = cases.arrays(n_member, 2, 5, 30, dtype, seed=5)
  levels = np.array(LEVELS + (0.3, 0.62))
  levels.sort()
  tables = engine.quantile_score_levels(levels, n_member, 'linear')
  _, q, _, _, ok = qs.host_terms(ens, truth, tables)
  assert ok.all()
  want = quantile_np.quantile(ens, levels, axis=0, skipna=False)
  quantile_np.assert_bit_equal(np.moveaxis(q, -1, 0), want)
  # and through the table: one point per cell
  one = cases.datasets(ens[:, :, 2:3, 4:5], truth[:, 2:3, 4:5])
  one[0].coords['latitude'] = one[1].coords['latitude'] = np.array([10.0])
  one[0].coords['longitude'] = one[1].coords['longitude'] = np.array([0.0])
  table = qs.QuantileScoreTable(tuple(levels)).compute_chunk(g(one[0]),
                                                             g(one[1]))
  quantile_np.assert_bit_equal(
      np.ascontiguousarray(table[NAME].values[:, 1, :].T),
      np.ascontiguousarray(want[:, :, 2, 4]))


# ---------------------------------------------------------------------------
# 2. the identities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', (1, 2, 7, 33))
def test_hazen_levels_give_the_crps_of_the_crps_table(dtype, n_member):
  grid = (9, 68)
  ens, truth = cases.arrays(n_member, 2, *grid, dtype, nan='both', seed=6)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  levels = (np.arange(1, n_member + 1) - 0.5) / n_member
  table = qs.QuantileScoreTable(tuple(levels), method='hazen').compute_chunk(
      g(forecast), g(tru), skipna=True, regions=regions)
  got = qs.crps_from_quantiles(table)[NAME]
  want = cd.crps(cd.CRPSTable().compute_chunk(
      g(forecast), g(tru), skipna=True, regions=regions))[NAME]
  assert got.dims == want.dims == ('region', 'time')
  n_class = events.column_classes(regions, *cases.grid(*grid))[1].shape[1]
  spread = float(np.nanmax(ens) - np.nanmin(ens)) if n_member > 1 else 0.0
  rtol, atol = qnp.crps_identity_tol(*grid, n_class, n_member, spread)
  live = ~np.isnan(want.values)
  np.testing.assert_array_equal(np.isnan(got.values), ~live)
  err = np.abs(got.values - want.values)[live]
  bound = rtol * np.abs(want.values)[live] + atol
  print(f'worst: {(err / bound).max():.3f} of the bound')
  assert live.any() and (err <= bound).all()


@pytest.mark.parametrize('method', cases.METHODS)
def test_interval_scores_equal_the_per_point_winkler_score_and_coverage(
    method):
  grid, n_member = (9, 68), 7
  ens, truth = cases.arrays(n_member, 2, *grid, np.float32, nan='truth',
                            seed=7, kind='precip')
  forecast, tru = cases.datasets(ens, truth)
  oregions = cases.oracle_regions()
  regions = cases.product_regions(oregions)
  lat, lon = cases.grid(*grid)
  levels = (0.05, 0.25, 0.4, 0.5, 0.75, 0.95)   # 0.4 has no partner
  table = qs.QuantileScoreTable(levels, method=method).compute_chunk(
      g(forecast), g(tru), skipna=True, regions=regions)
  score = qs.interval_score(table)[NAME]
  cover = qs.interval_coverage(table)[NAME]
  width = qs.interval_width(table)[NAME]
  assert score.dims == cover.dims == width.dims == (
      'region', 'time', cases.INTERVAL)
  np.testing.assert_array_equal(score.coords[cases.INTERVAL],
                                [1 - 2 * 0.25, 1 - 2 * 0.05])
  n_class = events.column_classes(regions, lat, lon)[1].shape[1]
  # each side: two table terms against their exact means, a few roundings
  rtol = 2 * qnp.table_rtol(*grid, n_class) + 8 * U
  for k, tau in enumerate((0.25, 0.05)):
    point, covered, ok = qnp.winkler(ens, truth, tau, method)
    _, q, _, _, _ = qnp.point_terms(ens, truth, (tau, 1 - tau), method)
    for r, region in enumerate(oregions.values()):
      w = _oracle_region_weights(region, lat, lon)
      for o in range(2):
        mass = math.fsum(w[ok[o]])
        if mass == 0:
          assert np.isnan(score.values[r, o, k])
          continue
        want = math.fsum(w[ok[o]] * point[o][ok[o]]) / mass
        assert abs(score.values[r, o, k] - want) <= rtol * want
        want = math.fsum(w[ok[o]] * covered[o][ok[o]]) / mass
        # (three frequencies within [0, 1] are combined)
        assert abs(cover.values[r, o, k] - want) <= 3 * rtol
        gap = (q[o][..., 1] - q[o][..., 0])[ok[o]]
        want = math.fsum(w[ok[o]] * gap) / mass
        scale = math.fsum(w[ok[o]] * np.abs(q[o][ok[o]]).sum(-1)) / mass
        assert abs(width.values[r, o, k] - want) <= rtol * scale
  with pytest.raises(ValueError, match='no pair'):
    qs.interval_score(qs.QuantileScoreTable((0.1, 0.5, 0.8)).compute_chunk(
        g(forecast), g(tru)))


def test_direct_mode_on_the_ensembles_quantiles_equals_ensemble_mode():
  for dtype in cases.DTYPES:
    ens, truth = cases.arrays(7, 2, 5, 30, dtype, nan='truth', seed=8,
                              kind='precip')
    forecast, tru = cases.datasets(ens, truth)
    regions = cases.product_regions(cases.oracle_regions())
    # levels whose 'linear' quantiles fall on members: exact in the dtype
    levels = (0.0, 0.5, 1.0)
    q = quantile_np.quantile(ens, levels, axis=0, skipna=False).astype(dtype)
    assert not np.isnan(q).any()
    qf, qt = cases.quantile_datasets(q, truth, levels)
    for kwargs in (dict(levels=None), dict(levels=levels)):
      direct = qs.QuantileScoreTable(quantile_dim=cases.QDIM, **kwargs)
      got = direct.compute_chunk(g(qf), g(qt), skipna=True, regions=regions)
      want = qs.QuantileScoreTable(levels).compute_chunk(
          g(forecast), g(tru), skipna=True, regions=regions)
      assert got.attrs == {'ensemble_size': 1, 'method': 'linear',
                           'levels': levels}
      want = want.assign_attrs(ensemble_size=1)
      cases.assert_same_dataset(got, want)
  with pytest.raises(ValueError, match='differ from the coordinate'):
    qs.QuantileScoreTable((0.0, 0.5, 0.9), quantile_dim=cases.QDIM
                          ).compute_chunk(g(qf), g(qt))
  # a NaN in any quantile value makes the point invalid
  q[1, 0, 2, 3] = np.nan
  qf, qt = cases.quantile_datasets(q, truth, levels)
  table = qs.QuantileScoreTable(None, quantile_dim=cases.QDIM).compute_chunk(
      g(qf), g(qt))
  assert np.isnan(table[NAME].values[0]).all()


def test_a_direct_and_an_ensemble_variable_in_one_dataset():
  """Each variable of a mixed Dataset gets the table it gets alone; the
  levels are the quantile coordinate for both."""
  levels = (0.1, 0.5, 0.9)
  ens, truth = cases.arrays(7, 2, 5, 30, np.float32, nan='truth', seed=11)
  q, _ = cases.arrays(3, 2, 5, 30, np.float32, nan='member', seed=12)
  q = np.sort(q, axis=0)
  forecast, tru = cases.datasets(ens, truth)
  qf, qt = cases.quantile_datasets(q, truth, levels)
  regions = cases.product_regions(cases.oracle_regions())
  gf, gq, gt = g(forecast), g(qf), g(tru)
  coords = dict(gf.coords)
  coords.update(gq.coords)
  for first, second in (('members', 'quantiles'), ('quantiles', 'members')):
    pick = {'members': gf[NAME], 'quantiles': gq[NAME]}
    mixed = xl.Dataset({first: pick[first], second: pick[second]}, coords)
    both = xl.Dataset({first: gt[NAME], second: gt[NAME]}, gt.coords)
    for kwargs in (dict(levels=None), dict(levels=levels, method='hazen')):
      metric = qs.QuantileScoreTable(quantile_dim=cases.QDIM, **kwargs)
      for extra in (dict(regions=regions), dict()):
        got = metric.compute_chunk(mixed, both, skipna=True, **extra)
        assert list(got.data_vars) == [first, second]
        assert got.attrs == {'ensemble_size': 7, 'method': metric.method,
                             'levels': levels}
        np.testing.assert_array_equal(got[cases.LEVEL].values, levels)
        alone = qs.QuantileScoreTable(levels, metric.method).compute_chunk(
            gf, gt, skipna=True, **extra)[NAME]
        direct = metric.compute_chunk(gq, g(qt), skipna=True, **extra)[NAME]
        for name, want in (('members', alone), ('quantiles', direct)):
          assert got[name].dims == want.dims
          np.testing.assert_array_equal(
              np.asarray(got[name].values).view(np.uint64),
              np.asarray(want.values).view(np.uint64))
        assert np.isfinite(got['members'].values).any()
        assert np.isfinite(got['quantiles'].values).any()
  # levels that differ from the coordinate are refused for the whole Dataset
  with pytest.raises(ValueError, match='differ from the coordinate'):
    qs.QuantileScoreTable((0.1, 0.5, 0.8), quantile_dim=cases.QDIM
                          ).compute_chunk(mixed, both)


def test_the_end_levels_and_a_single_member():
  ens, truth = cases.arrays(5, 1, 5, 30, np.float64, seed=9)
  forecast, tru = cases.datasets(ens, truth)
  table = qs.QuantileScoreTable((0.0, 1.0)).compute_chunk(g(forecast), g(tru))
  p = table[NAME].values[0]
  lo, hi = ens.min(axis=0)[0], ens.max(axis=0)[0]
  # tau = 0: only a truth below the minimum costs; tau = 1: above the maximum
  tables = engine.quantile_score_levels((0.0, 1.0), 5)
  pin, q, below, tie, ok = qs.host_terms(ens[:, 0], truth[0], tables)
  np.testing.assert_array_equal(q[..., 0], lo)
  np.testing.assert_array_equal(q[..., 1], hi)
  np.testing.assert_array_equal(pin[..., 0], np.maximum(lo - truth[0], 0))
  np.testing.assert_array_equal(pin[..., 1], np.maximum(truth[0] - hi, 0))
  assert np.isfinite(p).all() and (p[0] >= 0).all()
  assert np.array_equal(tables[0], [0, 4]) and np.array_equal(tables[1], [1, 4])
  assert np.array_equal(tables[2], [0.0, 0.0])
  # M = 1: every level is the forecast itself, whatever the method; the
  # pinball loss at 1/2 is half the absolute error
  det = cases.datasets(ens[:1], truth)
  det_f = xl.Dataset({NAME: g(det[0])[NAME].isel(realization=0)},
                     {k: v for k, v in g(det[0]).coords.items()
                      if k != 'realization'})
  first = None
  for method in cases.METHODS:
    for fc in (g(det[0]), det_f):
      got = qs.QuantileScoreTable((0.1, 0.5), method=method).compute_chunk(
          fc, g(det[1]))
      assert got.attrs['ensemble_size'] == 1
      v = got[NAME].values
      first = v if first is None else first
      np.testing.assert_array_equal(v.view(np.uint64), first.view(np.uint64))
  np.testing.assert_array_equal(first[0, 1, 0], first[0, 1, 1])
  mae = np.abs(ens[0, 0].astype(np.float64) - truth[0])
  sums, _, _ = qs.host_sums(ens[:1], 0, 1, None, truth, None, 1, 5, 30,
                            np.zeros(30, np.int32), 1,
                            engine.quantile_score_levels((0.5,), 1))
  np.testing.assert_allclose(sums[0, :, 0, 0, 0], 0.5 * mae.sum(axis=1),
                             rtol=40 * U)


def test_seventeen_levels_are_the_two_launches_halves():
  ens, truth = cases.arrays(7, 2, 5, 30, np.float32, nan='both', seed=10)
  cls = cases.runs(30, 3)
  levels = np.linspace(0.02, 0.98, 17)
  tables = engine.quantile_score_levels(levels, 7, 'weibull')
  args = (ens, truth.size, 7, None, truth, None, 2, 5, 30, cls, 3)
  whole = qs.host_sums(*args, tables)
  first = qs.host_sums(*args, tuple(a[:16] for a in tables))
  last = qs.host_sums(*args, tuple(a[16:] for a in tables))
  for k in range(2):
    np.testing.assert_array_equal(
        whole[k].view(np.uint64 if k == 0 else np.int32),
        np.concatenate([first[k], last[k]], axis=3).view(
            np.uint64 if k == 0 else np.int32))
  np.testing.assert_array_equal(whole[2], first[2])
  np.testing.assert_array_equal(whole[2], last[2])
  forecast, tru = cases.datasets(ens, truth)
  t17 = qs.QuantileScoreTable(tuple(levels), 'weibull').compute_chunk(
      g(forecast), g(tru), skipna=True)[NAME].values
  t16 = qs.QuantileScoreTable(tuple(levels[:16]), 'weibull').compute_chunk(
      g(forecast), g(tru), skipna=True)[NAME].values
  np.testing.assert_array_equal(t17[..., :16].view(np.uint64),
                                np.ascontiguousarray(t16).view(np.uint64))


# ---------------------------------------------------------------------------
# 3. the scores: host arithmetic on any table
# ---------------------------------------------------------------------------
def _table(values, levels):
  """A quantile score table DataArray of a [.., 4, L] array."""
  values = np.asarray(values, dtype=np.float64)
  lead = tuple(f'd{k}' for k in range(values.ndim - 2))
  return xl.DataArray(values, lead + (cases.TERM, cases.LEVEL),
                      {cases.LEVEL: np.asarray(levels, dtype=np.float64)})


def test_scores_on_a_hand_made_table():
  levels = (0.1, 0.5, 0.9)
  p = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 4.0], [0.125, 0.25, 0.75],
                [0.0, 0.5, 0.125]])
  table = _table(np.stack([p, 2 * p]), levels)
  np.testing.assert_array_equal(qs.quantile_score(table).values,
                                np.stack([p[0], 2 * p[0]]))
  assert qs.quantile_score(table).dims == ('d0', cases.LEVEL)
  for ties, c in (('below', 0.0), ('half', 0.5), ('above', 1.0)):
    np.testing.assert_array_equal(
        qs.observed_frequency(table, ties=ties).values[0], p[2] + c * p[3])
  with pytest.raises(ValueError, match='ties='):
    qs.observed_frequency(table, ties='none')
  assert qs.interval_width(table).dims == ('d0', cases.INTERVAL)
  np.testing.assert_array_equal(qs.interval_width(table).values[0], [5.0])
  np.testing.assert_array_equal(qs.interval_coverage(table).values[0],
                                [0.75 + 0.125 - 0.125])
  np.testing.assert_array_equal(qs.interval_score(table).values[0],
                                [(1.0 + 3.0) / 0.1])
  np.testing.assert_array_equal(qs.interval_score(table).coords[
      cases.INTERVAL], [1 - 2 * 0.1])
  np.testing.assert_array_equal(qs.quantile_skill(table, table).values, 0.0)
  ref = _table(np.stack([2 * p, 2 * p]), levels)
  np.testing.assert_array_equal(qs.quantile_skill(table, ref).values[0], 0.5)
  with pytest.raises(ValueError, match='differ in levels'):
    qs.quantile_skill(table, _table(np.stack([p, p]), (0.1, 0.5, 0.8)))
  # w = (0.3, 0.4, 0.3): midpoints 0.3 and 0.7
  np.testing.assert_allclose(qs.crps_weights(levels), [0.3, 0.4, 0.3],
                             rtol=4 * U)
  np.testing.assert_allclose(
      qs.crps_from_quantiles(table).values,
      [2 * (0.3 * 1 + 0.4 * 2 + 0.3 * 3), 4 * (0.3 * 1 + 0.4 * 2 + 0.3 * 3)],
      rtol=8 * U)
  assert qs.crps_from_quantiles(table).dims == ('d0',)
  # every 0/0 is NaN
  zero = _table(np.zeros((4, 3)), levels)
  assert np.isnan(qs.quantile_skill(zero, zero).values).all()
  with pytest.raises(ValueError, match='not a quantile score table'):
    qs.quantile_score(xl.DataArray(np.zeros((3, 3)), ('term', 'level'),
                                   {'level': np.arange(3.0)}))
  # a Dataset gives {variable: result}
  ds = xl.Dataset({'a': table, 'b': ref}, {cases.LEVEL: np.array(levels)})
  out = qs.interval_score(ds)
  assert set(out.data_vars) == {'a', 'b'}
  np.testing.assert_array_equal(out['b'].values[0], [2 * (1.0 + 3.0) / 0.1])


# ---------------------------------------------------------------------------
# 4. the metric protocol: time mean, bootstrap, Eval, Pooled
# ---------------------------------------------------------------------------
def test_compute_is_the_time_mean_of_the_tables():
  n_time = 3
  ens, truth = cases.arrays(7, n_time, 5, 30, np.float32, seed=3)
  forecast, tru = cases.datasets(ens, truth)
  metric = qs.QuantileScoreTable(cases.LEVELS, method='hazen')
  whole = metric.compute(g(forecast), g(tru))
  assert whole[NAME].dims == (cases.TERM, cases.LEVEL)
  assert whole.attrs == {'ensemble_size': 7, 'method': 'hazen',
                         'levels': cases.LEVELS}
  chunks = [metric.compute_chunk(g(forecast.isel(time=slice(k, k + 1))),
                                 g(tru.isel(time=slice(k, k + 1)))
                                 )[NAME].values[0] for k in range(n_time)]
  np.testing.assert_allclose(whole[NAME].values, np.mean(chunks, axis=0),
                             rtol=4 * U, atol=4 * U)
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               regions=regions)
  fan = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  cases.assert_same_dataset(fan, every)
  mean = metric.compute_regions(g(forecast), g(tru), regions, True)
  assert mean[NAME].dims == ('region', cases.TERM, cases.LEVEL)
  assert mean.attrs['method'] == 'hazen' and mean.attrs['ensemble_size'] == 7


def test_bootstrap_and_every_score_carry_the_replicate_dim():
  ens, truth = cases.arrays(7, 6, 5, 30, np.float64, seed=4)
  forecast, tru = cases.datasets(ens, truth)
  tables = qs.QuantileScoreTable(cases.LEVELS).compute_chunk(g(forecast),
                                                             g(tru))
  assert tables[NAME].dims == ('time', cases.TERM, cases.LEVEL)
  kwargs = dict(n_replicate=25, block_length=2, seed=2)
  out = bs.bootstrap(tables, qs.crps_from_quantiles, **kwargs)
  counts = bs.block_plan(6, 25, 2, seed=2)
  rep = bs.resample_means(tables, counts)
  reps = qs.crps_from_quantiles(rep)[NAME]
  assert reps.dims == (bs.REPLICATE,) and reps.shape == (25,)
  assert np.isfinite(reps.values).all()
  np.testing.assert_array_equal(out[NAME + '_standard_error'].values,
                                np.asarray(reps.values).std(axis=0, ddof=1))
  loop = bs.bootstrap(tables, qs.crps_from_quantiles, vectorized=False,
                      **kwargs)
  cases.assert_same_dataset(out, loop)
  # every function keeps the leading dim; a DataArray gives the result itself
  lead = (bs.REPLICATE,)
  for fn in (qs.quantile_score, qs.observed_frequency):
    assert fn(rep)[NAME].dims == lead + (cases.LEVEL,)
    assert fn(rep[NAME]).dims == lead + (cases.LEVEL,)
  for fn in (qs.interval_width, qs.interval_coverage, qs.interval_score):
    assert fn(rep)[NAME].dims == lead + (cases.INTERVAL,)
    assert fn(rep)[NAME].shape == (25, 2)
  assert qs.quantile_skill(rep, rep)[NAME].dims == lead + (cases.LEVEL,)


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 30, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = qs.QuantileScoreTable(cases.LEVELS)
  assert metric._fused_regions and not metric._reads_slabs_in_place
  cfg = config.Eval(metrics={'quantile_score': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims
  assert da.dims[-2:] == (cases.TERM, cases.LEVEL)
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
  metric = qs.QuantileScoreTable(cases.LEVELS, method='weibull')
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
  run = lambda *args, **kwargs: qs.QuantileScoreTable(
      *args, **kwargs).compute_chunk(g(forecast), g(tru))
  for method in ('nearest', 'median_unbiased', None, 7):
    _refuses(lambda: run(method=method), 'method=')
  _refuses(lambda: run(()), 'non-empty')
  _refuses(lambda: run(((0.1, 0.2),)), 'non-empty 1-D')
  _refuses(lambda: run(('a',)), 'numbers')
  _refuses(lambda: run((-0.1, 0.5)), r'within \[0, 1\]')
  _refuses(lambda: run((0.5, 1.5)), r'within \[0, 1\]')
  _refuses(lambda: run((0.5, np.nan)), 'finite')
  _refuses(lambda: run((0.5, np.inf)), 'finite')
  _refuses(lambda: run((0.5, 0.5)), 'strictly increasing')
  _refuses(lambda: run((0.5, 0.25)), 'strictly increasing')
  _refuses(lambda: run(tuple(np.linspace(0, 1, 65))), '65 levels.*1 to 64')
  _refuses(lambda: run(None), 'levels=None')
  # direct mode: at most 16 quantile forecasts, levels from the coordinate
  q17 = np.sort(cases.arrays(17, 1, 5, 30, np.float32)[0], axis=0)
  qf, qt = cases.quantile_datasets(q17, truth[:, :5, :30],
                                   np.linspace(0.1, 0.9, 17))
  direct = qs.QuantileScoreTable(None, quantile_dim=cases.QDIM)
  _refuses(lambda: direct.compute_chunk(g(qf), g(qt)),
           '17 levels.*1 to 16 quantile forecasts')
  qf, qt = cases.quantile_datasets(q17[:3], truth[:, :5, :30], (0.1, 0.9, 0.5))
  _refuses(lambda: direct.compute_chunk(g(qf), g(qt)), 'strictly increasing')
  qf, qt = cases.quantile_datasets(q17[:3], truth[:, :5, :30], (0.1, 0.5, 1.5))
  _refuses(lambda: direct.compute_chunk(g(qf), g(qt)), r'within \[0, 1\]')
  metric = qs.QuantileScoreTable()
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
  big = cases.datasets(*cases.arrays(qs.MAX_MEMBERS + 1, 1, 5, 30, np.float32))
  _refuses(lambda: metric.compute_chunk(g(big[0]), g(big[1])),
           f'{qs.MAX_MEMBERS + 1} members.*1 to 64')
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
  # 64 levels and 64 members are taken
  full = cases.datasets(*cases.arrays(64, 1, 5, 30, np.float32))
  table = qs.QuantileScoreTable(tuple(np.linspace(0, 1, 64))).compute_chunk(
      g(full[0]), g(full[1]))
  assert table.attrs['ensemble_size'] == 64
  assert table[NAME].shape[-2:] == (4, 64)
  assert run().attrs['levels'] == qs.DEFAULT_LEVELS == cases.LEVELS


def test_level_tables_of_the_three_methods():
  lo, hi, t, tau, omt = engine.quantile_score_levels((0.0, 0.3, 0.5, 1.0), 5)
  np.testing.assert_array_equal(lo, [0, 1, 2, 4])
  np.testing.assert_array_equal(hi, [1, 2, 3, 4])
  np.testing.assert_array_equal(t, [0.0, 0.3 * 4 - 1, 0.0, 0.0])
  np.testing.assert_array_equal(omt, 1.0 - np.array([0.0, 0.3, 0.5, 1.0]))
  assert lo.dtype == hi.dtype == np.int32 and t.dtype == tau.dtype == float
  for method in cases.METHODS:
    for m in (1, 2, 7, 33, 64):
      levels = np.linspace(0, 1, 23)
      lo, hi, t, _, _ = engine.quantile_score_levels(levels, m, method)
      wlo, whi, wt = qnp.positions(levels, m, method)
      np.testing.assert_array_equal(lo, wlo)
      np.testing.assert_array_equal(hi, whi)
      np.testing.assert_array_equal(t, wt)
      assert (0 <= lo).all() and (lo <= hi).all() and (hi < m).all()
      assert (0 <= t).all() and (t < 1).all()
  # hazen below 1 / (2 M) and weibull below 1 / (M + 1) clamp to the minimum
  assert engine.quantile_score_levels((0.01,), 7, 'hazen')[0][0] == 0
  assert engine.quantile_score_levels((0.01,), 7, 'hazen')[2][0] == 0.0
  assert engine.quantile_score_levels((0.99,), 7, 'weibull')[0][0] == 6
  lo, hi, t, _, _ = engine.quantile_score_levels((0.2, 0.7), 2, direct=True)
  assert lo.tolist() == hi.tolist() == [0, 1] and t.tolist() == [0.0, 0.0]
  with pytest.raises(ValueError, match='2 levels for 3 quantile forecasts'):
    engine.quantile_score_levels((0.2, 0.7), 3, direct=True)
  with pytest.raises(ValueError, match='0 members'):
    engine.quantile_score_levels((0.2, 0.7), 0)


def test_both_symbols_are_exported_and_declared(lib):
  import os
  h = lib.load()
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  header = open(os.path.join(root, 'include', 'wb2hip.h')).read()
  for name in ('wb2_quantile_score_sums', 'wb2_quantile_score_geometry'):
    assert getattr(h, name) is not None
    assert re.search(r'^int %s\(' % name, header, re.M), name
  assert 'K28' in header and 'n_slot = 2 n_level' in header
  from weatherbench2_amd import build
  assert 'quantile_score.hip' in build.SOURCES


def test_engine_refuses_bad_tables_and_sizes_on_the_host(lib):
  """Host tensors stand in for the operands: every refusal below comes from
  the host checks, before anything is uploaded or launched."""
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32)
  e, y = torch.from_numpy(ens), torch.from_numpy(truth)
  cls = cases.rotated(n_col, 2)
  slab = n_row * n_col
  good = engine.quantile_score_levels((0.1, 0.5), n_member)
  swap = lambda k, v: tuple(v if i == k else a for i, a in enumerate(good))
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def sums(ens=e, stride=n_outer * slab, n_member=n_member, ens_slab=None,
           truth=y, truth_slab=None, n_outer=n_outer, cls=cls, n_class=2,
           tables=good, direct=False):
    return engine.quantile_score_sums(ens, stride, n_member, ens_slab, truth,
                                      truth_slab, n_outer, n_row, n_col, cls,
                                      n_class, tables, direct)
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
        (dict(tables=good[:4]), ValueError, 'level tables must be'),
        (dict(tables=swap(0, np.array([0, 3]))), ValueError, 'lo <= hi'),
        (dict(tables=swap(1, np.array([1, 3]))), ValueError, 'hi < n_member'),
        (dict(tables=swap(0, np.array([-1, 1]))), ValueError, '0 <= lo'),
        (dict(tables=swap(2, np.array([0.2, 1.0]))), ValueError, 't < 1'),
        (dict(tables=swap(2, np.array([0.2]))), ValueError, 'one length'),
        (dict(tables=tuple(a[:0] for a in good)), ValueError, 'non-empty'),
        (dict(direct=True), ValueError, 'lo == hi'),
        (dict(tables=engine.quantile_score_levels(
            np.linspace(0, 1, 17), n_member),
              n_member=17, stride=0, direct=True), ValueError, 'lo == hi'),
        (dict(truth=y.double()), TypeError, 'dtype'),
        (dict(ens=e.half(), truth=y.half()), TypeError, 'dtype'),
        (dict(truth=y.transpose(-1, -2)), ValueError, 'contiguous'),
        (dict(n_class=65), lib.Wb2HipError, 'n_class=')):
      with pytest.raises(error, match=match):
        sums(**kwargs)
      assert not calls, kwargs
    lo17 = np.arange(17, dtype=np.int32)
    with pytest.raises(ValueError, match='17 levels.*1 to 16'):
      sums(n_member=17, stride=0, direct=True,
           tables=(lo17, lo17, np.zeros(17), np.linspace(0, 1, 17),
                   1 - np.linspace(0, 1, 17)))
    assert not calls
  finally:
    engine.set_launch_hook(old)
  ok = torch.zeros(1, 2, 3, 4, 2, dtype=torch.float64)
  cnt = torch.zeros(1, 2, 3, 4, 2, dtype=torch.int32)
  with pytest.raises(ValueError, match='sums must be'):
    engine.quantile_score_fold(ok, cnt, torch.zeros(1, 2, 3, 3,
                                                    dtype=torch.int32),
                               None, np.ones((1, 2)), np.ones((1, 3), np.int32))
  with pytest.raises(ValueError, match='wrow'):
    engine.quantile_score_fold(ok, cnt, torch.zeros(1, 2, 3, 2,
                                                    dtype=torch.int32),
                               None, np.ones((1, 4)), np.ones((1, 3), np.int32))


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data
  i32 = lambda *v: np.array(v, np.int32)
  f64 = np.zeros(17)

  def sums(dtype=lib.WB2_F32, ens=b, n_member=5, stride=8, n_outer=2, n_row=2,
           n_col=4, n_class=2, mode=0, n_level=2, lo=i32(0, 3), hi=i32(1, 4),
           t=f64, out=b, cnt=b, valid=b):
    return h.wb2_quantile_score_sums(
        dtype, ens, None, b, None, n_member, stride, n_outer, n_row, n_col, b,
        n_class, mode, n_level, None if lo is None else lo.ctypes.data,
        hi.ctypes.data, None if t is None else t.ctypes.data, f64.ctypes.data,
        f64.ctypes.data, out, cnt, valid, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=65), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(mode=2), b'mode='),
      (dict(mode=-1), b'mode='), (dict(n_level=0), b'n_level='),
      (dict(n_level=17), b'n_level='), (dict(lo=None), b'null pointer'),
      (dict(t=None), b'null pointer'),
      (dict(lo=i32(0, 5), hi=i32(1, 5)), b'positions'),
      (dict(lo=i32(2, 3), hi=i32(1, 4)), b'positions'),
      (dict(lo=i32(-1, 3)), b'positions'),
      (dict(mode=1), b'lo == hi'),
      (dict(stride=-1), b'member_stride='), (dict(n_row=-1), b'negative'),
      (dict(ens=None), b'null pointer'), (dict(out=None), b'null pointer'),
      (dict(cnt=None), b'null pointer'), (dict(valid=None), b'null pointer'),
      (dict(n_col=1 << 28), b'too long')):
    assert sums(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert sums(ens=None, **empty) == 0


def test_geometry_values(lib):
  h = lib.load()
  for dtype, size in ((torch.float32, 4), (torch.float64, 8)):
    for n_member in (1, 16, 50, 64):
      for n_level in (1, 5, 16):
        geo = engine.quantile_score_geometry(dtype, n_member, 13, n_level)
        # the formula of include/wb2hip.h
        members = n_member * 64 * size
        tile = 64 * ((2 * n_level) | 1) * 8
        assert geo['lds_bytes'] == max(members, tile) + 256 <= 65536
        assert (geo['min_member'], geo['max_member']) == (
            qs.MIN_MEMBERS, qs.MAX_MEMBERS) == (1, 64)
        assert geo['max_levels'] == qs.MAX_DIRECT_LEVELS == 16
        assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
        assert geo['max_grid_outer'] == engine.conditional_geometry(
            dtype)['max_grid_outer']
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.quantile_score_geometry(torch.float32, 65)
  with pytest.raises(lib.Wb2HipError, match='n_class='):
    engine.quantile_score_geometry(torch.float32, 1, 65)
  with pytest.raises(lib.Wb2HipError, match='n_level='):
    engine.quantile_score_geometry(torch.float32, 1, 1, 17)
  with pytest.raises(TypeError):
    engine.quantile_score_geometry(torch.float16)
  null = h.wb2_quantile_score_geometry(lib.WB2_F32, 1, 1, 0, 1, None, None,
                                       None, None, None, None, None)
  assert null < 0 and b'null pointer' in h.wb2_last_error()
