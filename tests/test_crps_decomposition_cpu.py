"""CRPS decomposition on the host path (no GPU): known answers, the dense
restatement, the identity reliability + potential = CRPS, the oracle's fair
CRPS, ties, refusals and the metric protocol."""
import functools

import numpy as np
import pytest

from oracle import metrics_np as om
from tests import crps_decomposition_cases as cases
from tests import crps_decomposition_np as cnp
from tests import helpers
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import regions as greg
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
U = cnp.U

# every member count, dtype and grid; the NaN patterns cycle so that each one
# meets both dtypes and both grids
CASES = [(grid, m, dtype, cases.NANS[(a + b + c) % 4])
         for a, grid in enumerate(cases.GRIDS)
         for b, m in enumerate(cases.MEMBERS)
         for c, dtype in enumerate(cases.DTYPES)]
_ID = lambda v: getattr(v, '__name__', None) or (
    'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


@functools.lru_cache(maxsize=None)
def _case(grid, n_member, dtype, nan):
  """The arrays, the oracle datasets, the per-point terms of the restatement
  and the product's tables (every region, both skipna) of one case: computed
  once, shared and left unchanged."""
  n_time = 2 if grid == cases.GRIDS[0] else 1
  ens, truth = cases.arrays(n_member, n_time, *grid, dtype, nan)
  forecast, tru = cases.datasets(ens, truth)
  terms, valid = cnp.point_fields(ens, truth)
  oregions = cases.oracle_regions()
  metric = cd.CRPSTable()
  tables = {skipna: metric.compute_chunk(
      g(forecast), g(tru), skipna=skipna,
      regions=cases.product_regions(oregions)) for skipna in (False, True)}
  return ens, truth, forecast, tru, terms, valid, oregions, tables


def _table(alpha, beta, outlier):
  p = np.array([alpha, beta, outlier], dtype=np.float64)
  return xl.DataArray(p, ('term', 'bin'),
                      {'term': np.array(cd.TERMS, dtype=object),
                       'bin': np.arange(p.shape[-1])})


def _one_point(members, truth, dtype=np.float64):
  """The table of the same point at latitudes -45 and 45 (equal weights: the
  mean of two equal values costs two roundings)."""
  ens = np.broadcast_to(np.array(members, dtype=dtype).reshape(-1, 1, 1, 1),
                        (len(members), 1, 2, 1)).copy()
  forecast, tru = cases.datasets(ens, np.full((1, 2, 1), truth, dtype=dtype))
  for ds in (forecast, tru):
    ds.coords['latitude'] = np.array([-45.0, 45.0])
  return cd.CRPSTable().compute_chunk(g(forecast), g(tru))[NAME]


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_known_answers(dtype):
  rtol = 4 * U
  da = _one_point([0.0, 1.0], 0.25, dtype)
  assert da.dims == ('time', 'term', 'bin') and da.dtype == np.float64
  p = da.values[0]
  np.testing.assert_allclose(p[0], [0, 0.25, 0], rtol=rtol)
  np.testing.assert_allclose(p[1], [0, 0.75, 0], rtol=rtol)
  np.testing.assert_array_equal(p[2], [0, 0, 0])
  np.testing.assert_allclose(cd.crps(da).values, [0.25], rtol=rtol)

  da = _one_point([1.0, 0.0], 2.0, dtype)
  p = da.values[0]
  np.testing.assert_allclose(p[0], [0, 1, 1], rtol=rtol)
  np.testing.assert_array_equal(p[1], [0, 0, 0])
  np.testing.assert_array_equal(p[2], [0, 0, 1])
  np.testing.assert_allclose(cd.crps(da).values, [1.25], rtol=rtol)

  da = _one_point([0.0, 1.0], -1.0, dtype)
  p = da.values[0]
  np.testing.assert_array_equal(p[0], [0, 0, 0])
  np.testing.assert_allclose(p[1], [1, 1, 0], rtol=rtol)
  np.testing.assert_array_equal(p[2], [1, 0, 0])
  np.testing.assert_allclose(cd.crps(da).values, [1.25], rtol=rtol)

  # M = 1: crps is the mean |x - y|; the fair form has no spread to take
  for truth, bins in ((2.0, (1, 0)), (-1.0, (0, 1))):
    da = _one_point([0.5], truth, dtype)
    p = da.values[0]
    assert p.shape == (3, 2)
    hit, miss = bins
    np.testing.assert_allclose(p[1 - hit][hit], 1.5, rtol=rtol)
    np.testing.assert_array_equal(p[1 - hit][miss], 0.0)
    np.testing.assert_array_equal(p[hit], [0, 0])
    np.testing.assert_array_equal(p[2][hit], 1.0)
    np.testing.assert_array_equal(p[2][miss], 0.0)
    np.testing.assert_allclose(cd.crps(da).values, [abs(0.5 - truth)],
                               rtol=rtol)
    assert np.isnan(cd.crps(da, fair=True).values).all()


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_one_member_crps_is_the_mean_absolute_error(dtype):
  ens, truth, forecast, tru, *_ = _case(cases.GRIDS[0], 1, dtype, 'none')
  got = cd.crps(cd.CRPSTable().compute_chunk(g(forecast), g(tru)))[NAME]
  lat = forecast.coord('latitude')
  w = om.get_lat_weights(lat).data[None, :, None]
  err = np.abs(ens[0].astype(np.float64) - truth.astype(np.float64))
  want = (err * w).sum((1, 2)) / (w.sum() * ens.shape[-1])
  n = err.shape[1] * err.shape[2]
  # the dense mean, in NumPy's order: the derived bound of two summation orders
  np.testing.assert_allclose(got.values, want, rtol=cnp.table_rtol(n))
  # the same mean summed in the product's order (|x - y| split by its sign,
  # columns in order, then rows with the row weights): the known-answer bound
  diff = truth.astype(np.float64) - ens[0].astype(np.float64)
  wrow = om.get_lat_weights(lat).data
  for t_ in range(diff.shape[0]):
    parts = []
    for part in (np.maximum(diff[t_], 0.0), np.maximum(-diff[t_], 0.0)):
      acc = mass = 0.0
      for i in range(part.shape[0]):
        s = 0.0
        for j in range(part.shape[1]):
          s = s + part[i, j]
        acc = acc + wrow[i] * s
        mass = mass + wrow[i] * float(part.shape[1])
      parts.append(acc / mass)
    np.testing.assert_allclose(got.values[t_], parts[0] + parts[1],
                               rtol=4 * U, atol=0)
  assert np.isnan(cd.crps(cd.CRPSTable().compute_chunk(
      g(forecast), g(tru)), fair=True)[NAME].values).all()


@pytest.mark.parametrize('grid,n_member,dtype,nan', CASES, ids=_ID)
def test_table_equals_the_dense_restatement(grid, n_member, dtype, nan):
  ens, truth, forecast, tru, terms, valid, oregions, tables = _case(
      grid, n_member, dtype, nan)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  n = len(lat) * len(lon)
  for skipna in (False, True):
    got = tables[skipna]
    da = got[NAME]
    assert da.dims == ('region', 'time', 'term', 'bin')
    assert da.dtype == np.float64
    assert got.attrs == {'ensemble_size': n_member}
    assert list(got['region'].values) == list(oregions)
    assert list(got['term'].values) == list(cd.TERMS)
    np.testing.assert_array_equal(got['bin'].values, np.arange(n_member + 1))
    for r, (name, region) in enumerate(oregions.items()):
      weights = _oracle_region_weights(region, lat, lon)
      want = cnp.dense_table(terms, valid, weights, skipna)
      np.testing.assert_allclose(da.values[r], want, rtol=cnp.table_rtol(n),
                                 atol=0, equal_nan=True,
                                 err_msg=f'{name} skipna={skipna}')
    if nan == 'none':
      assert np.isfinite(da.values[0]).all()
    elif not skipna:
      assert np.isnan(da.values[0]).any()
    # one region alone (None, and one that wraps) is that slice of the fused
    # pass
    for name in ('global', 'europe'):
      one = cd.CRPSTable().compute_chunk(
          g(forecast), g(tru), skipna=skipna,
          region=helpers.to_gpu_region(oregions[name]))
      assert one[NAME].dims == da.dims[1:]
      np.testing.assert_array_equal(
          one[NAME].values, da.values[list(oregions).index(name)])


@pytest.mark.parametrize('grid,n_member,dtype,nan', CASES, ids=_ID)
def test_reliability_plus_potential_is_the_crps(grid, n_member, dtype, nan):
  *_, tables = _case(grid, n_member, dtype, nan)
  for skipna in (False, True):
    table = tables[skipna]
    parts = cd.decomposition(table)[NAME]
    whole = cd.crps(table)[NAME].values
    p = table[NAME].values
    total = parts['reliability'].values + parts['potential'].values
    np.testing.assert_array_equal(np.isnan(total), np.isnan(whole))
    ok = ~np.isnan(whole)
    assert (np.abs(total - whole)[ok] <= cnp.identity_atol(p)[ok]).all()
    # the host arithmetic against the restatement's bin-by-bin sum
    np.testing.assert_allclose(whole, cnp.crps_of_table(p),
                               rtol=4 * (n_member + 4) * U, equal_nan=True)
    assert parts['g'].dims == table[NAME].dims[:-2] + ('bin',)
    assert (parts['reliability'].values[ok] >= 0).all()
    assert (parts['potential'].values[ok] >= 0).all()
    o = parts['o'].values
    assert ((o[~np.isnan(o)] >= 0) & (o[~np.isnan(o)] <= 1)).all()


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('n_member', [2, 7, 33])
@pytest.mark.parametrize('grid', cases.GRIDS, ids=_ID)
def test_fair_crps_of_the_table_equals_the_oracles_crps(grid, n_member,
                                                        skipna):
  """skipna=False: the oracle's `CRPS`.  skipna=True: NaNs in the truth only
  (the reference skips NaN members inside its means, the table calls such a
  point invalid), and the oracle's POINTWISE CRPS (`SpatialCRPS`) averaged by
  its own `spatial_average`: its `CRPS` averages skill and spread separately,
  and the spread -- which never looks at the truth -- keeps the points whose
  truth is NaN, so it is the mean of a different set of points than the skill
  beside it; the table leaves such a point out of both."""
  ens, truth, forecast, tru, _, _, oregions, tables = _case(
      grid, n_member, np.float64, 'truth' if skipna else 'none')
  got = cd.crps(tables[skipna], fair=True)[NAME]
  atol = cnp.fair_atol(ens, truth, grid[0] * grid[1])
  if skipna:
    assert np.isnan(truth).any()
    field = om.SpatialCRPS().compute_chunk(forecast, tru, skipna=True)
    chunk = lambda region: om.spatial_average(field, region, True)
  else:
    chunk = lambda region: om.CRPS().compute_chunk(forecast, tru,
                                                   region=region)
  for r, (name, region) in enumerate(oregions.items()):
    want = chunk(region)[NAME]
    assert got.dims[1:] == want.dims, name
    np.testing.assert_allclose(got.values[r], want.data, rtol=0, atol=atol,
                               equal_nan=True, err_msg=name)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_ties_are_not_outliers(dtype):
  ens, truth, below, above = cases.tie_case(dtype)
  forecast, tru = cases.datasets(ens, truth)
  lat, lon = forecast.coord('latitude'), forecast.coord('longitude')
  table = cd.CRPSTable().compute_chunk(g(forecast), g(tru))[NAME].values[0]
  w = _oracle_region_weights(None, lat, lon)
  # the hand-counted frequencies, summed in the product's order (columns,
  # then rows) so that the comparison is exact
  for flags, got in ((below, table[2, 0]), (above, table[2, -1])):
    wrow = om.get_lat_weights(lat).data
    acc = mass = 0.0
    for i in range(len(lat)):
      acc = acc + wrow[i] * float(flags[0, i].sum())
      mass = mass + wrow[i] * float(len(lon))
    assert got == acc / mass
    np.testing.assert_allclose(got, (w * flags[0]).sum() / w.sum(),
                               rtol=8 * U)
  assert below.sum() == 3 and above.sum() == 4  # (what was planted)
  np.testing.assert_array_equal(table[2, 1:-1], 0.0)


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
  metric = cd.CRPSTable()
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
  big = cases.datasets(*cases.arrays(cd.MAX_MEMBERS + 1, 1, 5, 8, np.float32))
  _refuses(lambda: metric.compute_chunk(g(big[0]), g(big[1])),
           f'{cd.MAX_MEMBERS + 1} members')
  for dtype in (np.float16, np.int32):
    odd = cases.datasets(ens.astype(dtype), truth)
    _refuses(lambda: metric.compute_chunk(g(odd[0]), g(odd[1])),
             'float32 and float64')
  flat = cases.datasets(ens, truth)[1]
  with pytest.raises(ValueError, match='realization'):
    metric.compute_chunk(g(flat), g(tru))
  with pytest.raises(ValueError, match='not a CRPS table'):
    cd.crps(xl.DataArray(np.zeros((2, 2, 3)), ('a', 'b', 'c')))


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_entry_points_refuse_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data

  def sums(dtype=lib.WB2_F32, ens=b, n_member=5, stride=8, n_outer=2, n_row=2,
           n_col=4, n_class=2, out=b):
    return h.wb2_crps_bin_sums(dtype, ens, None, b, None, n_member, stride,
                               n_outer, n_row, n_col, b, n_class, out, b, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_member=0), b'n_member='),
      (dict(n_member=65), b'n_member='), (dict(n_class=0), b'n_class='),
      (dict(n_class=65), b'n_class='), (dict(stride=-1), b'member_stride='),
      (dict(n_row=-1), b'negative'), (dict(ens=None), b'null pointer'),
      (dict(out=None), b'null pointer')):
    assert sums(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert sums(ens=None, **empty) == 0
  assert h.wb2_crps_bin_fold(None, 0, 3, 2, 8, None, None, 2, None, None) == 0
  assert h.wb2_crps_bin_fold(None, 2, 3, 2, 8, None, None, 2, None, None) < 0
  assert b'null pointer' in h.wb2_last_error()
  assert h.wb2_crps_bin_fold(b, 2, 3, 0, 8, b, b, 2, b, None) < 0
  assert b'bad sizes' in h.wb2_last_error()


def test_geometry_is_consistent(lib):
  import torch
  for dtype, size in ((torch.float32, 4), (torch.float64, 8)):
    for m in cases.MEMBERS:
      geo = engine.crps_bins_geometry(dtype, m, 3)
      assert (geo['min_member'], geo['max_member']) == (cd.MIN_MEMBERS,
                                                        cd.MAX_MEMBERS)
      assert geo['tile_cols'] == 64 and geo['rows_per_group'] == 1
      # the formula of include/wb2hip.h
      assert geo['lds_bytes'] == (m + 1) * 65 * size <= 65536
  with pytest.raises(lib.Wb2HipError, match='n_member='):
    engine.crps_bins_geometry(torch.float32, cd.MAX_MEMBERS + 1, 1)


def test_compute_is_the_time_mean_of_the_chunk_tables():
  ens, truth = cases.arrays(7, 3, 5, 8, np.float32, 'truth', seed=3)
  forecast, tru = cases.datasets(ens, truth)
  metric = cd.CRPSTable()
  for skipna in (False, True):
    whole = metric.compute(g(forecast), g(tru), skipna=skipna)
    assert whole[NAME].dims == ('term', 'bin')
    assert whole.attrs == {'ensemble_size': 7}
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
  assert mean.attrs['ensemble_size'] == 7


def test_eval_with_regions_gives_the_leading_region_dim():
  from weatherbench2_amd import config, evaluation
  ens, truth = cases.arrays(3, 2, 5, 8, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  regions = cases.product_regions(cases.oracle_regions())
  metric = cd.CRPSTable()
  cfg = config.Eval(metrics={'crps_table': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims and da.dims[-2:] == ('term', 'bin')
  assert [d for d in da.dims if d != 'metric'][0] == 'region'
  want = metric.compute_chunk(g(forecast), g(tru), regions=regions)[NAME]
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(want.shape), want.values)
  assert list(loop['region'].values) == list(regions)
