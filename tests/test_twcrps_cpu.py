"""Threshold-weighted CRPS on the host path (no GPU): the dense restatement,
the plain-CRPS limit against the oracle and against the CRPS decomposition,
the two tails adding up, exact cases planted by hand, the metric protocol and
the refusals."""
import functools

import numpy as np
import pytest
import torch

from oracle import metrics_np as om
from tests import helpers
from tests import twcrps_cases as cases
from tests import twcrps_np as tnp
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import regions as greg
from weatherbench2_amd import threshold_weighted as tw
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.neighborhood import ConstantThreshold

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = tnp.U
INF = float('inf')

# every member count, dtype and grid; the NaN patterns, the tails and the
# threshold counts cycle so that each meets both dtypes and both grids
CASES = [(grid, m, dtype, cases.NANS[(a + b + c) % 5],
          cases.TAILS[(a + b) % 2], cases.N_THRESHOLDS[(b + 2 * c) % 3])
         for a, grid in enumerate(cases.GRIDS)
         for b, m in enumerate(cases.MEMBERS)
         for c, dtype in enumerate(cases.DTYPES)]
# ... and the other tail of a few of them
CASES += [(grid, m, dtype, nan, cases.TAILS[1 - cases.TAILS.index(tail)], n)
          for grid, m, dtype, nan, tail, n in CASES[::5]]
_ID = lambda v: getattr(v, '__name__', None) or (
    'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


def _metric(ths, tail='upper', **kwargs):
  return tw.ThresholdWeightedCRPS(thresholds=ths, tail=tail, **kwargs)


@functools.lru_cache(maxsize=None)
def _case(grid, n_member, dtype, nan, tail, n_thr):
  """The arrays, the oracle datasets, the threshold fields and the product's
  tables (every region, both skipna) of one case: computed once, shared and
  left unchanged."""
  n_time = 2 if grid == cases.GRIDS[0] else 1
  ens, truth = cases.arrays(n_member, n_time, *grid, dtype, nan)
  forecast, tru = cases.datasets(ens, truth)
  fields = cases.threshold_fields(n_thr, n_time, *grid, dtype, nan)
  oregions = cases.oracle_regions()
  metric = _metric(cases.thresholds(fields, tru, g), tail)
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, fields, oregions, tables


@functools.lru_cache(maxsize=None)
def _plain_case(grid, n_member, dtype, nan):
  """The plain limit: tail 'upper' under the constant threshold -inf, every
  region, both skipna."""
  n_time = 2 if grid == cases.GRIDS[0] else 1
  ens, truth = cases.arrays(n_member, n_time, *grid, dtype, nan)
  forecast, tru = cases.datasets(ens, truth)
  oregions = cases.oracle_regions()
  regions = cases.product_regions(oregions)
  metric = _metric([ConstantThreshold(-INF)])
  tables = {skipna: metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                         regions=regions)
            for skipna in (False, True)}
  return ens, truth, forecast, tru, oregions, regions, tables


# ---------------------------------------------------------------------------
# 1. the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('grid,n_member,dtype,nan,tail,n_thr', CASES, ids=_ID)
def test_table_equals_the_dense_restatement(grid, n_member, dtype, nan, tail,
                                            n_thr):
  ens, truth, forecast, tru, fields, oregions, tables = _case(
      grid, n_member, dtype, nan, tail, n_thr)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  rtol = tnp.table_rtol(len(lat), len(lon), n_member)
  weights = {name: _oracle_region_weights(region, lat, lon)
             for name, region in oregions.items()}
  points = [tnp.point_fields(ens, truth, f, tail) for f in fields]
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'quantile', 'time', 'term')
    assert da.dtype == np.float64
    assert got.attrs == {'threshold_method': 'FieldThreshold',
                         'ensemble_size': n_member, 'tail': tail}
    assert list(got['region'].values) == list(oregions)
    assert list(got['term'].values) == list(tw.TERMS)
    np.testing.assert_array_equal(got['quantile'].values,
                                  0.1 * (np.arange(n_thr) + 1))
    for r, name in enumerate(oregions):
      for q, (terms, valid) in enumerate(points):
        want = tnp.dense_table(terms, valid, weights[name], n_member, skipna)
        np.testing.assert_allclose(da.values[r, q], want, rtol=rtol, atol=0,
                                   equal_nan=True,
                                   err_msg=f'{name} q={q} skipna={skipna}')
    if nan == 'none':
      assert np.isfinite(da.values[0]).all()
    elif nan == 'threshold':
      # validity is per threshold: threshold 0 (and 4) has NaNs of its own
      assert np.isnan(fields[0]).any()
      if skipna and n_thr > 1:
        valid = [v for _, v in points]
        assert (valid[0] != valid[1]).any()
    elif not skipna:
      assert np.isnan(da.values[0]).any()
    if n_member == 1:
      np.testing.assert_array_equal(
          da.values[..., 1][~np.isnan(da.values[..., 1])], 0.0)
  # one region alone (None, and one that wraps) is that slice of the fused
  # pass
  metric = _metric(cases.thresholds(fields, tru, g), tail)
  for name in ('global', 'europe'):
    one = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               region=helpers.to_gpu_region(oregions[name]))
    assert one[NAME].dims == tables[True][NAME].dims[1:]
    np.testing.assert_array_equal(
        one[NAME].values,
        tables[True][NAME].values[list(oregions).index(name)])


def test_the_gap_form_is_the_pair_sum_on_the_quarter_grid():
  """On values that are multiples of 0.25 every operation of both forms is
  exact, so B equals the written-out pair sum bit for bit."""
  ens, truth = cases.arrays(7, 1, 5, 8, np.float64)
  fields = cases.threshold_fields(1, 1, 5, 8, np.float64)
  for tail in cases.TAILS:
    for idx in np.ndindex(*truth.shape):
      members = [ens[(m,) + idx] for m in range(7)]
      a, b = tnp.point_terms(members, truth[idx], fields[0][idx], tail)
      assert b == tnp.pair_sum(members, fields[0][idx], tail)
      got = tw.host_point_terms(np.array(members)[:, None],
                                truth[idx][None], fields[0][idx][None],
                                tail == 'lower')
      assert (got[0][0], got[1][0]) == (a, b) and not got[2][0]


# ---------------------------------------------------------------------------
# 2. the plain CRPS in the limit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', [1, 7, 50])
def test_minus_infinity_above_is_plus_infinity_below(n_member, dtype):
  *_, forecast, tru, _, regions, tables = _plain_case(
      cases.GRIDS[1], n_member, dtype, 'both')
  lower = _metric([ConstantThreshold(INF)], 'lower')
  for skipna in (False, True):
    other = lower.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                regions=regions)
    a, b = tables[skipna][NAME], other[NAME]
    assert a.dims == b.dims
    np.testing.assert_array_equal(a.values.view(np.uint64),
                                  b.values.view(np.uint64))
    assert other.attrs == dict(tables[skipna].attrs, tail='lower')
  assert np.isfinite(tables[True][NAME].values).any()


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('n_member', [2, 7, 33])
@pytest.mark.parametrize('grid', cases.GRIDS, ids=_ID)
def test_fair_twcrps_of_the_plain_limit_equals_the_oracles_crps(
    grid, n_member, skipna):
  """skipna=False: the oracle's `CRPS`.  skipna=True: NaNs in the truth only,
  and the oracle's POINTWISE CRPS (`SpatialCRPS`) averaged by its own
  `spatial_average`, as tests/test_crps_decomposition_cpu.py does and for its
  reason: the oracle's `CRPS` averages the spread over the points whose truth
  is NaN too, the table leaves such a point out of both terms."""
  ens, truth, forecast, tru, oregions, _, tables = _plain_case(
      grid, n_member, np.float64, 'truth' if skipna else 'none')
  got = tw.twcrps(tables[skipna], fair=True)[NAME]
  assert got.dims == ('region', 'quantile', 'time')
  atol = tnp.fair_atol(ens, truth, grid[0] * grid[1])
  if skipna:
    assert np.isnan(truth).any()
    field = om.SpatialCRPS().compute_chunk(forecast, tru, skipna=True)
    chunk = lambda region: om.spatial_average(field, region, True)
  else:
    chunk = lambda region: om.CRPS().compute_chunk(forecast, tru,
                                                   region=region)
  for r, (name, region) in enumerate(oregions.items()):
    want = chunk(region)[NAME]
    assert got.dims[2:] == want.dims, name
    np.testing.assert_allclose(got.values[r, 0], want.data, rtol=0, atol=atol,
                               equal_nan=True, err_msg=name)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', [1, 3, 50, 64])
def test_plain_twcrps_equals_the_crps_of_the_decomposition_table(n_member,
                                                                 dtype):
  grid = cases.GRIDS[1]
  ens, truth, forecast, tru, _, regions, tables = _plain_case(
      grid, n_member, dtype, 'both')
  for skipna in (False, True):
    want = cd.crps(cd.CRPSTable().compute_chunk(
        g(forecast), g(tru), skipna=skipna, regions=regions))[NAME]
    got = tw.twcrps(tables[skipna])[NAME]
    assert got.dims == ('region', 'quantile', 'time')
    a, b = got.values[:, 0], want.values
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    atol = tnp.plain_atol(ens, truth, *grid, tables[skipna][NAME].values[:, 0])
    ok = ~np.isnan(a)
    assert ok.any() or not skipna
    assert (np.abs(a - b)[ok] <= atol[ok]).all()


# ---------------------------------------------------------------------------
# 3. the tails add up
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('nan', ['none', 'both'])
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', [1, 2, 7, 50])
def test_upper_plus_lower_is_the_plain_table(n_member, dtype, nan):
  grid = cases.GRIDS[1]
  *_, forecast, tru, _, regions, plain = _plain_case(grid, n_member, dtype,
                                                     nan)
  fields = cases.threshold_fields(4, 1, *grid, dtype)
  ths = cases.thresholds(fields, tru, g)
  for skipna in (False, True):
    up, low = (_metric(ths, tail).compute_chunk(
        g(forecast), g(tru), skipna=skipna, regions=regions)[NAME].values
               for tail in cases.TAILS)
    whole = np.broadcast_to(plain[skipna][NAME].values, up.shape)
    np.testing.assert_array_equal(np.isnan(up), np.isnan(whole))
    np.testing.assert_array_equal(np.isnan(low), np.isnan(whole))
    ok = ~np.isnan(whole)
    atol = tnp.tails_atol(*grid, n_member, up, low, whole)
    assert (np.abs(up + low - whole)[ok] <= atol[ok]).all()
    if skipna or nan == 'none':
      # (a finite threshold inside the data really splits the score)
      assert (up[ok] < whole[ok]).any() and (low[ok] < whole[ok]).any()


# ---------------------------------------------------------------------------
# 4. exact cases planted by hand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_planted_points_give_their_hand_computed_sums(dtype):
  ens, truth, t, a, b = cases.planted(dtype)
  n_col = truth.shape[-1]
  thr = np.full(truth.shape, t, dtype=dtype)
  # every column a class of its own: the sums of a class are one point's terms
  sums, cnt = tw.host_sums(ens, truth.size, 3, None, truth, None, [thr], None,
                           1, 2, n_col, np.arange(n_col), n_col)
  for row in range(2):
    np.testing.assert_array_equal(sums[0, 0, row, :, 0], a)
    np.testing.assert_array_equal(sums[0, 0, row, :, 1], b)
  assert (cnt == 1).all()
  # the other tail of the same points, from max(z, t) + min(z, t) = z + t
  plain = tw.host_sums(ens, truth.size, 3, None, truth, None,
                       [np.full(truth.shape, -INF, dtype=dtype)], None, 1, 2,
                       n_col, np.arange(n_col), n_col)[0]
  low = tw.host_sums(ens, truth.size, 3, None, truth, None, [thr], None, 1, 2,
                     n_col, np.arange(n_col), n_col, True)[0]
  np.testing.assert_array_equal(low + sums, plain)


def _one_column(members, truth, dtype):
  """(forecast, truth) of the same point at latitudes -45 and 45."""
  ens = np.broadcast_to(np.array(members, dtype=dtype).reshape(-1, 1, 1, 1),
                        (len(members), 1, 2, 1)).copy()
  forecast, tru = cases.datasets(ens, np.full((1, 2, 1), truth, dtype=dtype))
  for ds in (forecast, tru):
    ds.coords['latitude'] = np.array([-45.0, 45.0])
  return g(forecast), g(tru)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_exact_answers_of_the_metric(dtype):
  def table(members, truth, t, tail='upper'):
    forecast, tru = _one_column(members, truth, dtype)
    da = _metric([ConstantThreshold(t)], tail).compute_chunk(forecast,
                                                             tru)[NAME]
    assert da.dims == ('quantile', 'time', 'term') and da.shape == (1, 1, 2)
    return da.values[0, 0]

  # the threshold above every member and the truth: nothing in the tail
  np.testing.assert_array_equal(table([0.0, -1.0, 0.5], 0.25, 1.0), [0, 0])
  # all members below, the truth above: abs_error is y - t, in float64
  y, t = dtype(2.5), dtype(1.0)
  got = table([0.0, -2.0, 0.75], y, t)
  assert got[0] == np.float64(y) - np.float64(t) and got[1] == 0.0
  # the truth exactly on the threshold: it is clamped to itself
  got = table([3.0, 0.0, 1.0], 1.0, 1.0)
  np.testing.assert_allclose(got, [2.0 / 3, 4.0 / 9], rtol=4 * U)
  # a member exactly on the threshold
  got = table([4.0, 1.0, 2.0], 0.5, 1.0)
  np.testing.assert_allclose(got, [4.0 / 3, 6.0 / 9], rtol=4 * U)
  # all members equal: no pair distance, in either tail
  for tail in cases.TAILS:
    got = table([2.0, 2.0, 2.0], 3.0, 2.5, tail)
    assert got[1] == 0.0
    assert got[0] == 0.5  # (|2.5 - 3| above, |2 - 2.5| below)
  # the lower tail of the second case: members keep their distances
  got = table([0.0, -2.0, 0.75], 2.5, 1.0, 'lower')
  np.testing.assert_allclose(
      got, [(1.0 + 3.0 + 0.25) / 3, (2 * 2.0 + 2 * 0.75) / 9], rtol=4 * U)
  # M = 1: no pair distance, and the fair form has no spread to take
  forecast, tru = _one_column([0.5], 2.0, dtype)
  one = _metric([ConstantThreshold(1.0)]).compute_chunk(forecast, tru)
  np.testing.assert_array_equal(one[NAME].values[0, 0], [1.0, 0.0])
  assert one.attrs['ensemble_size'] == 1
  np.testing.assert_array_equal(tw.twcrps(one)[NAME].values, [[1.0]])
  assert np.isnan(tw.twcrps(one, fair=True)[NAME].values).all()


# ---------------------------------------------------------------------------
# 5. structure
# ---------------------------------------------------------------------------
def _lead_case(dtype=np.float32):
  """A forecast with a lead dim, a truth without it and thresholds without
  the time and lead dims."""
  rs = np.random.RandomState(0)
  lat, lon = cases.grid(5, 8)
  coords = {'realization': np.arange(3),
            'time': np.array(['2020-01-01', '2020-01-02'], 'datetime64[ns]'),
            'prediction_timedelta': np.arange(4) * np.timedelta64(1, 'D'),
            'latitude': lat, 'longitude': lon}
  dims = ('realization', 'time', 'prediction_timedelta', 'latitude',
          'longitude')
  full = (np.round(rs.normal(size=(3, 2, 4, 5, 8)) * 4) / 4).astype(dtype)
  tru = (np.round(rs.normal(size=(2, 5, 8)) * 4) / 4).astype(dtype)
  full[1, 0, 2, 3, 4] = tru[1, 4, 7] = np.nan
  forecast = xl.Dataset({'x': xl.DataArray(full, dims)}, coords)
  truth = xl.Dataset({'x': xl.DataArray(tru, dims[1:2] + dims[3:])}, coords)
  fields = [(np.round(rs.normal(size=(5, 8)) * 2) / 4 + c).astype(dtype)
            for c in (-0.5, 0.5)]
  ths = [cases.FieldThreshold(xl.Dataset(
      {'x': xl.DataArray(f, dims[3:])},
      {'latitude': lat, 'longitude': lon}), q)
         for f, q in zip(fields, (0.5, 0.9))]
  return forecast, truth, ths, full, tru, fields


def test_dims_coords_attrs_and_the_outer_dim_order():
  forecast, truth, ths, full, tru, fields = _lead_case()
  regions = {'global': None, 'north': helpers.to_gpu_region(
      helpers.predefined_regions()['northern-hemisphere'])}
  out = _metric(ths).compute_chunk(forecast, truth, skipna=True,
                                   regions=regions)
  da = out['x']
  assert da.dims == ('region', 'quantile', 'time', 'prediction_timedelta',
                     'term')
  assert da.shape == (2, 2, 2, 4, 2) and da.dtype == np.float64
  event = events.EventTable(thresholds=ths).compute_chunk(
      forecast, truth, skipna=True, regions=regions)['x']
  assert da.dims[:-1] == event.dims[:-2]  # as EventTable orders them
  np.testing.assert_array_equal(out['quantile'].values, [0.5, 0.9])
  assert list(out['region'].values) == ['global', 'north']
  assert list(out['term'].values) == ['abs_error', 'pair_distance']
  np.testing.assert_array_equal(out['prediction_timedelta'].values,
                                forecast.coords['prediction_timedelta'])
  assert out.attrs == {'threshold_method': 'FieldThreshold',
                       'ensemble_size': 3, 'tail': 'upper'}
  # the values: the restatement with the truth and thresholds broadcast
  lat, lon = cases.grid(5, 8)
  w = _oracle_region_weights(None, lat, lon)
  for q, f in enumerate(fields):
    for lead in range(4):
      terms, valid = tnp.point_fields(full[:, :, lead], tru, f)
      want = tnp.dense_table(terms, valid, w, 3, True)
      np.testing.assert_allclose(da.values[0, q, :, lead], want,
                                 rtol=tnp.table_rtol(5, 8, 3), atol=0)
  # `regions=` is one region at a time
  for r, region in enumerate(regions.values()):
    one = _metric(ths).compute_chunk(forecast, truth, region=region,
                                     skipna=True)['x']
    assert one.dims == da.dims[1:]
    np.testing.assert_array_equal(one.values, da.values[r])


def test_a_deterministic_forecast_is_one_member():
  ens, truth = cases.arrays(1, 2, 5, 8, np.float32, 'truth')
  forecast, tru = cases.datasets(ens, truth)
  fields = cases.threshold_fields(2, 2, 5, 8, np.float32)
  ths = cases.thresholds(fields, tru, g)
  want = _metric(ths).compute_chunk(g(forecast), g(tru), skipna=True)
  flat = g(forecast).isel(realization=0)
  assert 'realization' not in flat[NAME].dims
  for metric in (_metric(ths), _metric(ths, ensemble_dim=None)):
    got = metric.compute_chunk(flat, g(tru), skipna=True)
    assert got.attrs['ensemble_size'] == 1
    assert got[NAME].dims == ('quantile', 'time', 'term')
    np.testing.assert_array_equal(got[NAME].values, want[NAME].values)
  np.testing.assert_array_equal(want[NAME].values[..., 1], 0.0)
  # a threshold-weighted absolute error
  lat, lon = cases.grid(5, 8)
  w = _oracle_region_weights(None, lat, lon)
  for q, f in enumerate(fields):
    err = np.abs(np.maximum(ens[0].astype(np.float64), f) -
                 np.maximum(truth.astype(np.float64), f))
    ok = ~np.isnan(err)
    mean = [(w * np.where(ok[k], err[k], 0)).sum() / (w * ok[k]).sum()
            for k in range(2)]
    np.testing.assert_allclose(want[NAME].values[q, :, 0], mean,
                               rtol=4 * 40 * U)
  assert np.isnan(tw.twcrps(want, fair=True)[NAME].values).all()


def test_compute_is_the_time_mean_of_the_chunk_tables():
  ens, truth = cases.arrays(7, 3, 5, 8, np.float32, 'truth', seed=3)
  forecast, tru = cases.datasets(ens, truth)
  # (thresholds without the time dim: they serve every slice of the times)
  ths = cases.thresholds(cases.threshold_fields(2, 3, 5, 8, np.float32,
                                                lead=False), tru, g, lead=False)
  metric = _metric(ths, 'lower')
  for skipna in (False, True):
    whole = metric.compute(g(forecast), g(tru), skipna=skipna)
    assert whole[NAME].dims == ('quantile', 'term')
    assert whole.attrs['ensemble_size'] == 7 and whole.attrs['tail'] == 'lower'
    chunks = [metric.compute_chunk(g(forecast.isel(time=slice(k, k + 1))),
                                   g(tru.isel(time=slice(k, k + 1))),
                                   skipna=skipna)[NAME].values[:, 0]
              for k in range(3)]
    mean = np.nanmean(chunks, axis=0) if skipna else np.mean(chunks, axis=0)
    np.testing.assert_allclose(whole[NAME].values, mean, rtol=4 * U,
                               equal_nan=True)
    # the scores are taken from the mean table
    score = tw.twcrps(whole, fair=True)[NAME]
    assert score.dims == ('quantile',)
    np.testing.assert_allclose(
        score.values, whole[NAME].values[:, 0] - whole[NAME].values[:, 1] *
        (7.0 / 6.0), rtol=2 * U, equal_nan=True)
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(tru), skipna=True,
                               regions=regions)
  fan = metric.compute_chunk_regions(g(forecast), g(tru), regions, True)
  cases.assert_same_dataset(fan, every)
  mean = metric.compute_regions(g(forecast), g(tru), regions, True)
  assert mean[NAME].dims == ('region', 'quantile', 'term')
  assert mean.attrs['ensemble_size'] == 7


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  ths = cases.thresholds(cases.threshold_fields(2, 2, 5, 8, np.float32), tru,
                         g)
  regions = cases.product_regions(cases.oracle_regions())
  metric = _metric(ths)
  assert metric._fused_regions
  cfg = config.Eval(metrics={'twcrps': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims and da.dims[-1] == 'term'
  assert [d for d in da.dims if d != 'metric'][0] == 'region'
  want = metric.compute_chunk(g(forecast), g(tru), regions=regions)[NAME]
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(want.shape), want.values)
  assert list(loop['region'].values) == list(regions)


def test_scores_are_host_arithmetic_on_the_table():
  coords = {'quantile': np.array([0.5, 0.9]),
            'term': np.array(tw.TERMS, dtype=object)}
  p = np.array([[0.75, 0.25], [0.0, 0.0]])
  ref = np.array([[1.0, 0.5], [0.0, 0.0]])
  table = xl.Dataset({'x': xl.DataArray(p, ('quantile', 'term'), coords)},
                     coords, {'ensemble_size': 5})
  other = xl.Dataset({'x': xl.DataArray(ref, ('quantile', 'term'), coords)},
                     coords, {'ensemble_size': 3})
  np.testing.assert_array_equal(tw.twcrps(table)['x'].values, [0.5, 0.0])
  np.testing.assert_array_equal(tw.twcrps(table, fair=True)['x'].values,
                                [0.75 - 0.25 * (5.0 / 4.0), 0.0])
  np.testing.assert_array_equal(
      tw.twcrps(table['x'], fair=True, ensemble_size=2).values, [0.25, 0.0])
  skill = tw.twcrpss(table, other)['x']
  assert skill.dims == ('quantile',)
  assert skill.values[0] == 1.0 - 0.5 / 0.5 and np.isnan(skill.values[1])
  fair = tw.twcrpss(table, other, fair=True)['x'].values
  assert fair[0] == 1.0 - (0.75 - 0.25 * 1.25) / (1.0 - 0.5 * 1.5)
  assert np.isnan(fair[1])
  with pytest.raises(ValueError, match='ensemble size'):
    tw.twcrps(table['x'], fair=True)
  with pytest.raises(ValueError, match='not a twCRPS table'):
    tw.twcrps(xl.DataArray(np.zeros((2, 3)), ('a', 'b')))


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
  ths = [ConstantThreshold(0.5)]
  metric = _metric(ths)
  _refuses(lambda: _metric(ths, 'middle').compute_chunk(g(forecast), g(tru)),
           "tail='middle'")
  _refuses(lambda: _metric([]).compute_chunk(g(forecast), g(tru)),
           'at least one threshold')
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
  for n_member in (tw.MAX_MEMBERS + 1, 128):  # 65-128: EventTable's range
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


# ---------------------------------------------------------------------------
# 6. the engine and the C ABI refuse on the host
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_engine_refuses_bad_tables_and_sizes_on_the_host(lib):
  """Host tensors stand in for the operands: every refusal below comes from
  the host checks, before anything is uploaded or launched."""
  n_member, n_outer, n_row, n_col = 3, 4, 3, 8
  ens, truth = cases.arrays(n_member, n_outer, n_row, n_col, np.float32)
  thr = cases.threshold_fields(1, n_outer, n_row, n_col, np.float32)[0]
  e, y, h = (torch.from_numpy(a) for a in (ens, truth, thr))
  cls = cases.classes(n_col, 2)
  slab = n_row * n_col
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def sums(ens=e, stride=n_outer * slab, n_member=n_member, ens_slab=None,
           truth=y, truth_slab=None, thrs=(h,), thr_slabs=None,
           n_outer=n_outer, cls=cls, n_class=2):
    return engine.twcrps_sums(ens, stride, n_member, ens_slab, truth,
                              truth_slab, list(thrs), thr_slabs, n_outer,
                              n_row, n_col, cls, n_class)
  try:
    for kwargs, error, match in (
        (dict(ens_slab=np.arange(n_outer) + 1), IndexError, 'member slabs'),
        (dict(ens_slab=np.arange(n_outer - 1)), ValueError, 'member slab'),
        (dict(stride=n_outer * slab + 1), IndexError, 'member slabs'),
        (dict(truth=y[:2].clone()), IndexError, 'truth slabs'),
        (dict(truth_slab=np.array([0, 1, 2, -1])), IndexError, 'truth slabs'),
        (dict(thrs=(h[:1].clone(),)), IndexError, 'threshold slabs'),
        (dict(thr_slabs=[np.full(n_outer, 4)]), IndexError,
         'threshold slabs'),
        (dict(thr_slabs=[None, None]), ValueError, 'per threshold'),
        (dict(thrs=()), ValueError, 'no thresholds'),
        (dict(cls=cls + 1), IndexError, 'col_class'),
        (dict(cls=cls[:-1]), IndexError, 'col_class'),
        (dict(n_member=0), ValueError, '0 members'),
        (dict(n_member=65, stride=0), ValueError, '65 members'),
        (dict(stride=-1), ValueError, 'bad sizes'),
        (dict(n_outer=-1), ValueError, 'bad sizes'),
        (dict(truth=y.double()), TypeError, 'dtype'),
        (dict(thrs=(h.double(),)), TypeError, 'dtype'),
        (dict(ens=e.half(), truth=y.half(), thrs=(h.half(),)), TypeError,
         'dtype'),
        (dict(truth=y.transpose(-1, -2)), ValueError, 'contiguous')):
      with pytest.raises(error, match=match):
        sums(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
  # a threshold read through a table that names slab 0 is within one slab
  with pytest.raises(IndexError, match='threshold slabs'):
    sums(thrs=(h[0].clone(),), thr_slabs=[np.arange(n_outer)])
  with pytest.raises(ValueError, match='sums must be'):
    engine.twcrps_fold(torch.zeros(1, 2, 3, 2, 3, dtype=torch.float64),
                       torch.zeros(1, 2, 3, 2, 1, dtype=torch.int32), [4, 4],
                       np.ones((1, 3)), np.ones((1, 2), np.int32))
  good = (torch.zeros(1, 2, 3, 2, 2, dtype=torch.float64),
          torch.zeros(1, 2, 3, 2, 1, dtype=torch.int32))
  with pytest.raises(ValueError, match='wrow'):
    engine.twcrps_fold(*good, [4, 4], np.ones((1, 4)),
                       np.ones((1, 2), np.int32))
  with pytest.raises(ValueError, match='class_cols'):
    engine.twcrps_fold(*good, [4], np.ones((1, 3)), np.ones((1, 2), np.int32))


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data
  import ctypes
  ptrs = (ctypes.c_void_p * 5)(*([b] * 5))
  none = (ctypes.c_void_p * 5)(b, None, b, b, b)

  def sums(dtype=lib.WB2_F32, ens=b, thr=ptrs, n_thr=5, n_member=5, stride=8,
           n_outer=2, n_row=2, n_col=4, n_class=2, out=b):
    return h.wb2_twcrps_sums(dtype, ens, None, b, None, thr, None, n_thr,
                             n_member, stride, n_outer, n_row, n_col, b,
                             n_class, 0, out, b, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=65), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(n_thr=0), b'n_threshold='),
      (dict(stride=-1), b'member_stride='), (dict(n_row=-1), b'negative'),
      (dict(ens=None), b'null pointer'), (dict(thr=None), b'null pointer'),
      (dict(thr=none), b'null pointer'), (dict(out=None), b'null pointer')):
    assert sums(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert sums(ens=None, **empty) == 0


def test_geometry_agrees_with_the_limits_of_the_python_layer(lib):
  for dtype in (torch.float32, torch.float64):
    for m in cases.MEMBERS:
      for n_thr in (1, 2, 4, 5, 9):
        geo = engine.twcrps_geometry(dtype, m, 3, n_thr)
        assert (geo['min_member'], geo['max_member']) == (tw.MIN_MEMBERS,
                                                          tw.MAX_MEMBERS)
        assert geo['thresholds_per_launch'] == min(n_thr, 4)
        assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
        # the formula of include/wb2hip.h
        assert geo['lds_bytes'] == 2 * min(n_thr, 4) * 65 * 8 <= 4160
  assert engine.twcrps_geometry(torch.float32, 1, events.MAX_CLASSES, 1)
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.twcrps_geometry(torch.float32, tw.MAX_MEMBERS + 1, 1, 1)
  with pytest.raises(lib.Wb2HipError, match='n_class='):
    engine.twcrps_geometry(torch.float32, 1, events.MAX_CLASSES + 1, 1)
  with pytest.raises(lib.Wb2HipError, match='n_threshold='):
    engine.twcrps_geometry(torch.float32, 1, 1, 0)
