"""Pooled verification on the host path (no GPU): `host_pool` against the dense
restatement of tests/pooling_np.py, known answers, the composition law of
`Pooled` for the metrics that have a host path, and the refusals.  (The
composition law for `MSE` and `CRPS`, which run on the device only, is in
tests/test_pooling_gpu.py.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import metrics_np as om
from tests import crps_decomposition_cases as base
from tests import helpers
from tests import pooling_cases as cases
from tests import pooling_np as pnp
from tests import twcrps_np as tnp
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import neighborhood as nb
from weatherbench2_amd import pooling
from weatherbench2_amd import threshold_weighted as tw
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.neighborhood import ConstantThreshold

NAME = cases.NAME
NB = pooling.NEIGHBORHOOD
U = pnp.U
_ID = lambda v: getattr(v, '__name__', None) or (
    'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


# ---------------------------------------------------------------------------
# 1. host_pool against the dense restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('special', cases.SPECIALS)
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('slab', cases.SLABS, ids=lambda s: _ID(s[0]))
def test_host_pool_equals_the_dense_restatement(slab, dtype, special):
  shape, windows = slab
  x = cases.field(shape, dtype, special)
  if special == 'planted':
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(
        x[x == 0]).any()
  mean = pooling.host_pool(x, windows, 'mean')
  top = pooling.host_pool(x, windows, 'max')
  assert mean.shape == top.shape == (len(windows),) + shape
  for w, n in enumerate(windows):
    pnp.assert_mean_close(mean[w], x, n, f'mean, window {n}')
    pnp.assert_same_bits(top[w], pnp.dense_max(x, n), f'max, window {n}')
    if n == 1:
      for got in (mean[w], top[w]):
        pnp.assert_same_bits(got, x, 'window 1')
  if special != 'zeros':
    # (a field of zeros and -1 has most of its windows' maxima at zero)
    return
  assert np.signbit(top[top == 0]).any() and not np.signbit(top[top == 0]).all()


def test_leading_dims_are_slabs_of_their_own():
  x = cases.field((2, 3, 9, 12), np.float32, 'planted')
  for kind in cases.KINDS:
    whole = pooling.host_pool(x, (3, 5), kind)
    assert whole.shape == (2, 2, 3, 9, 12)
    for a in range(2):
      for b in range(3):
        pnp.assert_same_bits(whole[:, a, b],
                             pooling.host_pool(x[a, b], (3, 5), kind))


# ---------------------------------------------------------------------------
# 2. known answers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_a_field_of_ones_pools_to_ones(dtype, kind):
  x = np.ones((9, 12), dtype=dtype)
  out = pooling.host_pool(x, (1, 3, 5, 11), kind)
  np.testing.assert_array_equal(out, np.ones((4, 9, 12), dtype=dtype))


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('spike', [(4, 6), (0, 0), (8, 11), (1, 0)])
def test_a_unit_spike_spreads_over_its_window(spike, dtype):
  """mean: exactly 1 / N_i' at every point i', j' whose window holds the
  spike -- across column 0 and with the smaller N of the clipped rows --, 0
  elsewhere; max: 1 on the same points."""
  n_row, n_col = 9, 12
  x = np.zeros((n_row, n_col), dtype=dtype)
  x[spike] = 1.0
  windows = (3, 5, 11)
  mean = pooling.host_pool(x, windows, 'mean')
  top = pooling.host_pool(x, windows, 'max')
  for w, n in enumerate(windows):
    h = n // 2
    want = np.zeros((n_row, n_col), dtype=np.float64)
    for i in range(n_row):
      rows = min(n_row - 1, i + h) - max(0, i - h) + 1
      for j in range(n_col):
        near = abs(i - spike[0]) <= h and min(
            (j - spike[1]) % n_col, (spike[1] - j) % n_col) <= h
        if near:
          want[i, j] = 1.0 / float(n * rows)
    np.testing.assert_array_equal(mean[w], want.astype(dtype))
    np.testing.assert_array_equal(top[w], (want > 0).astype(dtype))
    assert (want > 0).sum() > n  # (the spike is seen from more than one row)


@pytest.mark.parametrize('n', [3, 5, 9])
@pytest.mark.parametrize('d', [1, 2, 4, 7, 12])
def test_two_spikes_d_apart_cost_twice_min_d_n_over_n(d, n):
  """The displacement error after mean pooling: the sum over the slab of
  |pool(f) - pool(o)| is 2 min(d, n) / n -- no double penalty once the window
  covers the displacement."""
  n_row, n_col = 21, 40
  f = np.zeros((n_row, n_col), dtype=np.float64)
  o = np.zeros((n_row, n_col), dtype=np.float64)
  f[10, 36] = 1.0           # (d columns apart, across the seam)
  o[10, (36 + d) % n_col] = 1.0
  pf = pooling.host_pool(f, (n,), 'mean')[0]
  po = pooling.host_pool(o, (n,), 'mean')[0]
  import math
  total = math.fsum(np.abs(pf - po).reshape(-1).tolist())
  assert abs(total - 2.0 * min(d, n) / n) <= 8 * U


# ---------------------------------------------------------------------------
# 3. pool(): Datasets and DataArrays
# ---------------------------------------------------------------------------
def test_pool_keeps_dims_order_dtype_and_the_other_variables():
  ens, truth = cases.ensemble(3, 2, 9, 12, np.float32)
  forecast, _ = cases.datasets(ens, truth)
  flipped, _ = cases.datasets(ens, truth, lonlat=True)
  forecast['level_weight'] = xl.DataArray(np.arange(2.0), ('time',))
  out = pooling.pool(forecast, (1, 5), 'mean')
  da = out[NAME]
  assert da.dims == (NB, 'realization', 'time', 'latitude', 'longitude')
  assert da.dtype == np.float32 and da.shape == (2, 3, 2, 9, 12)
  np.testing.assert_array_equal(out.coords[NB], [1, 5])
  assert out.coords[NB].dtype == np.int64
  assert out['level_weight'].dims == ('time',)
  np.testing.assert_array_equal(out['level_weight'].values, [0.0, 1.0])
  pnp.assert_same_bits(da.values, pooling.host_pool(ens, (1, 5), 'mean'))
  # a (longitude, latitude) variable: the same pools, its own dim order
  other = pooling.pool(flipped, (1, 5), 'mean')[NAME]
  assert other.dims == (NB, 'realization', 'time', 'longitude', 'latitude')
  pnp.assert_same_bits(np.swapaxes(other.values, -1, -2), da.values)
  # a DataArray in, a DataArray out
  one = pooling.pool(forecast[NAME], (5,), 'max')
  assert isinstance(one, xl.DataArray) and one.dims == da.dims
  pnp.assert_same_bits(one.values, pooling.host_pool(ens, (5,), 'max'))
  # nothing spatial: nothing pooled
  bare = xl.Dataset({'s': xl.DataArray(np.arange(3.0), ('time',))},
                    {'time': np.arange(3)})
  assert pooling.pool(bare, (3,))['s'].dims == ('time',)


# ---------------------------------------------------------------------------
# 4. the composition law
# ---------------------------------------------------------------------------
def _regions():
  return base.product_regions(base.oracle_regions())


def _metrics():
  ths = [ConstantThreshold(-0.25), ConstantThreshold(0.5)]
  return {'EventTable': events.EventTable(thresholds=ths),
          'ThresholdWeightedCRPS': tw.ThresholdWeightedCRPS(thresholds=ths),
          'CRPSTable': cd.CRPSTable()}


@functools.lru_cache(maxsize=None)
def _pair(nan=False):
  ens, truth = cases.ensemble(5, 3, 9, 12, np.float32, nan=nan)
  return cases.datasets(ens, truth)


def _window(ds, n, kind='mean'):
  return pooling.pool(ds, (n,), kind).isel(**{NB: 0})


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('name', sorted(_metrics()))
def test_pooled_is_the_metric_on_the_pooled_fields(name, kind):
  metric = _metrics()[name]
  forecast, truth = _pair(nan=(kind == 'max'))
  pooled = pooling.Pooled(metric, (3, 5, 1), kind)
  regions = _regions()
  for skipna in (False, True):
    chunk = pooled.compute_chunk(forecast, truth, skipna=skipna)
    one = pooled.compute_chunk(forecast, truth, region=regions['tropics'],
                               skipna=skipna)
    every = pooled.compute_chunk_regions(forecast, truth, regions, skipna)
    whole = pooled.compute(forecast, truth, skipna=skipna)
    means = pooled.compute_regions(forecast, truth, regions, skipna)
    for da in (chunk[NAME], every[NAME], whole[NAME]):
      assert da.dims[0] == NB
    assert every[NAME].dims[1] == 'region'
    np.testing.assert_array_equal(chunk.coords[NB], [3, 5, 1])
    for k, n in enumerate((3, 5, 1)):
      f, t = _window(forecast, n, kind), _window(truth, n, kind)
      pick = lambda ds: ds.isel(**{NB: k})
      cases.assert_same_dataset(
          pick(chunk), metric.compute_chunk(f, t, skipna=skipna))
      cases.assert_same_dataset(
          pick(one), metric.compute_chunk(f, t, region=regions['tropics'],
                                          skipna=skipna))
      cases.assert_same_dataset(
          pick(every), metric.compute_chunk_regions(f, t, regions, skipna))
      want = metric.compute(f, t, skipna=skipna)
      assert whole.attrs == {**want.attrs, 'pooling': kind}
      cases.assert_same_dataset(
          xl.Dataset(dict(pick(whole).data_vars), pick(whole).coords,
                     want.attrs), want)
      want = metric.compute_regions(f, t, regions, skipna)
      assert means.attrs == {**want.attrs, 'pooling': kind}
      np.testing.assert_array_equal(pick(means)[NAME].values,
                                    want[NAME].values)
    # window 1 is the metric on the raw input
    cases.assert_same_dataset(
        chunk.isel(**{NB: 2}),
        metric.compute_chunk(forecast, truth, skipna=skipna))
  if kind == 'max':
    # the NaN rule is the wrapped metric's, on the pooled fields: the planted
    # NaNs spread with the window
    plain = pooled.compute_chunk(forecast, truth, skipna=False)[NAME].values
    assert np.isnan(plain).any()


def test_the_regions_variant_pools_once_per_chunk(monkeypatch):
  """One `pool` call for the forecast and one for the truth, whatever the
  number of regions and windows."""
  forecast, truth = _pair()
  calls = []
  real = pooling.pool

  def counting(obj, neighborhoods, kind='mean'):
    calls.append(tuple(neighborhoods))
    return real(obj, neighborhoods, kind)
  monkeypatch.setattr(pooling, 'pool', counting)
  pooled = pooling.Pooled(_metrics()['EventTable'], (3, 5, 9))
  regions = _regions()
  assert len(regions) > 2
  pooled.compute_chunk_regions(forecast, truth, regions)
  assert calls == [(3, 5, 9)] * 2
  del calls[:]
  from weatherbench2_amd import config, evaluation
  cfg = config.Eval(metrics={'pooled': pooled}, regions=regions)
  loop = xl.as_dataset(evaluation._metric_and_region_loop(
      forecast, truth, cfg, False, compute_chunk=True))
  assert calls == [(3, 5, 9)] * 2
  want = pooled.compute_chunk_regions(forecast, truth, regions)[NAME]
  assert loop[NAME].dims == ('metric',) + want.dims
  np.testing.assert_array_equal(np.asarray(loop[NAME].values)[0], want.values)


def test_pooled_declares_the_generic_path():
  pooled = pooling.Pooled(_metrics()['EventTable'])
  assert tuple(pooled.neighborhoods) == (1, 3, 5, 9, 17)
  assert pooled.pooling == 'mean'
  for cls in (pooling.Pooled, pooling.PooledCRPS):
    assert not cls._fused_regions and not cls._reads_slabs_in_place


@pytest.mark.parametrize('kind', cases.KINDS)
def test_pooled_crps_is_the_twcrps_at_minus_infinity(kind):
  forecast, truth = _pair()
  plain = tw.ThresholdWeightedCRPS(
      thresholds=[ConstantThreshold(-float('inf'))], tail='upper')
  metric = pooling.PooledCRPS((1, 3, 5), kind)
  regions = _regions()
  table = metric.compute_chunk(forecast, truth)
  assert table[NAME].dims == (NB, 'time', 'term')
  assert 'quantile' not in table.coords
  every = metric.compute_chunk_regions(forecast, truth, regions)
  assert every[NAME].dims == (NB, 'region', 'time', 'term')
  whole = metric.compute(forecast, truth)
  assert whole[NAME].dims == (NB, 'term')
  assert whole.attrs['pooling'] == kind and whole.attrs['ensemble_size'] == 5
  for k, n in enumerate((1, 3, 5)):
    f, t = _window(forecast, n, kind), _window(truth, n, kind)
    want = plain.compute_chunk(f, t)
    assert table.attrs == want.attrs
    np.testing.assert_array_equal(table[NAME].values[k],
                                  want[NAME].values[0])
    np.testing.assert_array_equal(
        every[NAME].values[k],
        plain.compute_chunk_regions(f, t, regions)[NAME].values[:, 0])
    np.testing.assert_array_equal(whole[NAME].values[k],
                                  plain.compute(f, t)[NAME].values[0])
  score = pooling.pooled_crps(table)[NAME]
  assert score.dims == (NB, 'time')
  np.testing.assert_array_equal(
      score.values, table[NAME].values[..., 0] - table[NAME].values[..., 1])


def test_fair_pooled_crps_of_window_one_is_the_oracles_crps():
  ens, truth = base.arrays(7, 2, 5, 8, np.float64)
  oforecast, otruth = base.datasets(ens, truth)
  g = helpers.to_gpu_dataset
  regions = base.oracle_regions()
  table = pooling.PooledCRPS((1, 3)).compute_chunk_regions(
      g(oforecast), g(otruth), base.product_regions(regions))
  got = pooling.pooled_crps(table, fair=True)[base.NAME]
  assert got.dims == (NB, 'region', 'time')
  atol = tnp.fair_atol(ens, truth, 5 * 8)
  for r, (name, region) in enumerate(regions.items()):
    want = om.CRPS().compute_chunk(oforecast, otruth, region=region)[base.NAME]
    np.testing.assert_allclose(got.values[0, r], want.data, rtol=0, atol=atol,
                               err_msg=name)
  # pooling smooths: the score of window 3 differs
  assert not np.array_equal(got.values[0], got.values[1])


# ---------------------------------------------------------------------------
# 5. refusals
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


def test_pool_refuses_before_anything_is_pooled():
  ens, truth = cases.ensemble(2, 1, 9, 12, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  _refuses(lambda: pooling.pool(forecast, (3,), 'median'), "pooling='median'")
  for bad in ((2,), (0,), (13,), (257,), (3.0,), (True,), (3, 3), ()):
    _refuses(lambda: pooling.pool(forecast, bad), 'window')
  regional = xl.Dataset(dict(forecast.data_vars),
                        {**forecast.coords,
                         'longitude': np.arange(12) * 10.0})
  _refuses(lambda: pooling.pool(regional, (3,)), 'not cyclic')
  for dtype in (np.float16, np.int32):
    odd, _ = cases.datasets(ens.astype(dtype), truth)
    _refuses(lambda: pooling.pool(odd, (3,)), 'float32 and float64')
  # above max_window: the halo would not fit the LDS, on either path
  wide = np.zeros((1, 1, 3, 200))
  for dtype in cases.DTYPES:
    limit = engine.pool_geometry(torch.from_numpy(
        np.zeros(0, dtype=dtype)).dtype)['max_window']
    assert limit < nb.MAX_WINDOW
    big, _ = cases.datasets(wide.astype(dtype), wide[0].astype(dtype))
    _refuses(lambda: pooling.pool(big, (limit + 2,)), f'up to {limit}')
    assert pooling.pool(big, (limit,))[NAME].shape == (1, 1, 1, 3, 200)
  metric = pooling.Pooled(_metrics()['EventTable'], (3,), 'median')
  _refuses(lambda: metric.compute_chunk(forecast, tru), "pooling='median'")
  _refuses(lambda: pooling.Pooled(None, (3,)).compute_chunk(forecast, tru),
           'wraps a Metric')
  fractions = nb.FractionsTable(thresholds=[ConstantThreshold(0.0)],
                                neighborhoods=(3,))
  _refuses(lambda: pooling.Pooled(fractions, (3,)).compute_chunk(
      forecast, tru), 'dim of its own')


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_both_symbols_are_declared_and_exported(lib):
  h = lib.load()
  for name in ('wb2_pool_fields', 'wb2_pool_geometry'):
    assert hasattr(h, name) and name in lib.exported_symbols()
  from weatherbench2_amd import build
  assert 'pool.hip' in build.SOURCES


def _windows(*values):
  return (ctypes.c_int32 * len(values))(*values)


def test_entry_point_refuses_before_any_launch(lib):
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data

  def fields(dtype=lib.WB2_F32, src=b, n_member=1, stride=8, n_outer=2,
             n_row=2, n_col=4, windows=_windows(1, 3), n_window=2, kind=0,
             out=b):
    return h.wb2_pool_fields(dtype, src, None, n_member, stride, n_outer,
                             n_row, n_col, windows, n_window, kind, out, None)
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(kind=2), b'kind='),
      (dict(kind=-1), b'kind='), (dict(n_member=0), b'n_member='),
      (dict(n_member=129), b'n_member='), (dict(n_window=0), b'n_window='),
      (dict(windows=_windows(2, 3)), b'window=2'),
      (dict(windows=_windows(3, 0)), b'window=0'),
      (dict(windows=_windows(-1, 3)), b'window=-1'),
      (dict(windows=_windows(5, 3)), b'window=5'),       # > n_col = 4
      (dict(windows=_windows(257, 3), n_col=300), b'window=257'),
      (dict(windows=_windows(3, 255), n_col=300), b'max_window'),
      (dict(stride=-1), b'member_stride='), (dict(n_outer=-1), b'negative'),
      (dict(n_row=-1), b'negative'), (dict(n_col=-1), b'negative'),
      (dict(windows=None), b'null pointer'), (dict(src=None), b'null pointer'),
      (dict(out=None), b'null pointer'),
      (dict(n_outer=2 ** 33), b'grid')):
    assert fields(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0), dict(n_col=0)):
    assert fields(src=None, out=None, **empty) == 0, empty


def test_geometry_refuses_and_reports(lib):
  h = lib.load()
  outs = [ctypes.c_int32() for _ in range(6)]
  lds = ctypes.c_int64()

  def geometry(dtype=lib.WB2_F32, n_col=300, windows=_windows(3, 17),
               n_window=2, first=ctypes.byref(outs[0])):
    return h.wb2_pool_geometry(dtype, n_col, windows, n_window, first,
                               ctypes.byref(outs[1]), ctypes.byref(outs[2]),
                               ctypes.byref(lds), ctypes.byref(outs[3]),
                               ctypes.byref(outs[4]))
  for kwargs, words in (
      (dict(dtype=7), b'unknown dtype'), (dict(n_window=0), b'n_window='),
      (dict(n_col=-1), b'negative'), (dict(windows=None), b'null pointer'),
      (dict(windows=_windows(4, 3)), b'window=4'),
      (dict(n_col=16), b'window=17'),
      (dict(windows=_windows(3, 255)), b'max_window'),
      (dict(first=None), b'null pointer')):
    assert geometry(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  assert geometry() == 0
  for dtype, esz in ((torch.float32, 4), (torch.float64, 8)):
    limit = engine.pool_geometry(dtype)['max_window']
    # the formula of include/wb2hip.h
    stage = lambda rows, n: ((rows + n - 1) * (64 + n - 1) * esz + 7
                             ) // 8 * 8 + (rows + n - 1) * 64 * 8
    assert stage(8, limit) <= 160 * 1024 < stage(8, limit + 2)
    assert limit == {4: 123, 8: 87}[esz]
    tiles = set()
    for windows in ((1,), (3, 5, 9, 17), (5, 17, 65), (3, 5, 7, 9, 11, 13),
                    (limit - 14,), (limit,)):
      geo = engine.pool_geometry(dtype, 1440, windows)
      assert geo['tile_cols'] == 64 and geo['max_window'] == limit
      assert geo['windows_per_launch'] == min(len(windows), 4)
      rows = next(r for r in (32, 16, 8)
                  if stage(r, max(windows)) <= 160 * 1024)
      assert geo['tile_rows'] == rows
      tiles.add(rows)
      assert geo['lds_bytes'] == stage(rows, max(windows))
      assert geo['max_grid_outer'] == 32768
    assert tiles == {32, 16, 8}
  with pytest.raises(lib.Wb2HipError, match='max_window'):
    engine.pool_geometry(torch.float64, 1440, (89,))


def test_engine_refuses_bad_tables_and_sizes_on_the_host(lib):
  """Host tensors stand in for the operand: every refusal below comes from the
  host checks, before anything is uploaded or launched."""
  x = torch.zeros(4, 3, 8)
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def fields(x=x, stride=0, n_member=1, slabs=None, n_outer=4, windows=(3,),
             kind='mean'):
    return engine.pool_fields(x, stride, n_member, slabs, n_outer, 3, 8,
                              windows, kind)
  try:
    for kwargs, error, match in (
        (dict(kind='median'), ValueError, "kind='median'"),
        (dict(x=x.half()), TypeError, 'float32 or float64'),
        (dict(slabs=np.arange(4) + 1), IndexError, 'field slabs'),
        (dict(slabs=np.array([0, 1, 2, -1])), IndexError, 'field slabs'),
        (dict(slabs=np.arange(3)), ValueError, 'field slab table'),
        (dict(n_outer=5), IndexError, 'field slabs'),
        (dict(n_member=2, stride=3 * 24 + 1, n_outer=1), IndexError,
         'field slabs'),
        (dict(stride=-1), ValueError, 'bad sizes'),
        (dict(n_outer=-1), ValueError, 'bad sizes'),
        (dict(windows=()), ValueError, 'no windows')):
      with pytest.raises(error, match=match):
        fields(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
