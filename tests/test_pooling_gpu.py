"""Pooled verification on the device (-m gpu): K22 (csrc/pool.hip) against the
host path of weatherbench2_amd/pooling.py, bit for bit (NaN positions equal),
at the smallest shapes at which the kernel can go wrong, and the wrapper
metric on device-backed datasets."""
import numpy as np
import pytest
import torch

from tests import crps_decomposition_cases as base
from tests import pooling_cases as cases
from tests import pooling_np as pnp
from weatherbench2_amd import crps_decomposition as cd
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import metrics as gm
from weatherbench2_amd import pooling
from weatherbench2_amd import threshold_weighted as tw
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.neighborhood import ConstantThreshold

pytestmark = pytest.mark.gpu

NAME = cases.NAME
NB = pooling.NEIGHBORHOOD
_ID = lambda v: getattr(v, '__name__', None) or (
    'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_dataset(ds: xl.Dataset) -> xl.Dataset:
  """The same Dataset with its variables in HBM."""
  return xl.Dataset({k: xl.DataArray(_dev(v.values), v.dims)
                     for k, v in ds.items()}, ds.coords, ds.attrs)


def _torch_dtype(dtype):
  return torch.float32 if dtype == np.float32 else torch.float64


def _members(x, windows, kind):
  """Device pools of a contiguous host array [O, M, R, C] through the member
  stride (the table names member 0 of every outer index) -> numpy [W, O, M, R,
  C]."""
  n_outer, n_member, n_row, n_col = x.shape
  table = None if n_member == 1 else np.arange(n_outer) * n_member
  out = engine.pool_fields(_dev(x), n_row * n_col, n_member, table, n_outer,
                           n_row, n_col, windows, kind)
  assert tuple(out.shape) == (len(windows),) + x.shape
  assert out.dtype == _torch_dtype(x.dtype) and out.is_contiguous()
  return out.cpu().numpy()


# the tile of the small windows (the geometry's answer is asserted below): one
# row / column short of it, one over, exact multiples; then a wave-wide row of
# few rows, the CPU cases and two tiles and a bit in the columns
TILE = (32, 64)
SHAPES = ((31, 63), (33, 65), (32, 64), (64, 128), (5, 64), (9, 12), (7, 9),
          (37, 70), (33, 130))
# the windows of the CPU cases and 17; where all six fit they are more than
# one launch's four (the second launch is staged for 17 alone with 9)
ALL_WINDOWS = (1, 3, 5, 11, 9, 17)
# NaN / -0.0 on both sides of the tile borders
BORDER = ((31, 63), (31, 64), (32, 63), (32, 64), (0, 63), (0, 64))


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('shape', SHAPES, ids=_ID)
def test_device_pool_equals_the_host_path(shape, dtype, kind):
  a = SHAPES.index(shape)
  windows = tuple(n for n in ALL_WINDOWS if n <= shape[1])
  geo = engine.pool_geometry(_torch_dtype(dtype), shape[1], windows)
  assert (geo['tile_rows'], geo['tile_cols']) == TILE
  assert geo['windows_per_launch'] == 4 and len(windows) >= 4
  n_member = (1, 2, 7)[a % 3]
  special = cases.SPECIALS[(a + cases.DTYPES.index(dtype)) % 3]
  x = cases.field((2, n_member) + shape, dtype, special, seed=a, extra=BORDER)
  got = _members(x, windows, kind)
  pnp.assert_same_bits(got, pooling.host_pool(x, windows, kind),
                       f'{special}, {n_member} members')
  w1 = windows.index(1)
  pnp.assert_same_bits(got[w1], x, 'window 1')


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', [1, 2, 7])
def test_every_member_count_and_special_value(n_member, dtype, kind):
  for special in cases.SPECIALS:
    x = cases.field((3, n_member, 33, 65), dtype, special, extra=BORDER)
    got = _members(x, (3, 17), kind)
    pnp.assert_same_bits(got, pooling.host_pool(x, (3, 17), kind), special)


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_a_window_that_needs_a_smaller_tile(dtype):
  """Windows whose staging leaves the 32-row tile: 16 and 8 rows."""
  tdtype = _torch_dtype(dtype)
  limit = engine.pool_geometry(tdtype)['max_window']
  seen = set()
  # (the middle one: the first window whose staging needs the 16-row tile)
  for n in (65, 107 if dtype == np.float32 else 73, limit):
    geo = engine.pool_geometry(tdtype, 140, (3, n))
    assert geo['lds_bytes'] <= 160 * 1024
    seen.add(geo['tile_rows'])
    x = cases.field((1, 2, 19, 140), dtype, 'planted')
    for kind in cases.KINDS:
      pnp.assert_same_bits(_members(x, (3, n), kind),
                           pooling.host_pool(x, (3, n), kind), f'window {n}')
  assert seen == {32, 16, 8}


@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_the_16_byte_and_the_one_element_forms_agree(dtype, kind):
  """The same fields read through an aligned base (16-byte loads and stores)
  and through a base that is one element off (one element per access)."""
  for shape in ((33, 64), (5, 128), (37, 72)):
    x = cases.field((3,) + shape, dtype, 'planted', extra=BORDER)
    n = x.size
    aligned = _dev(x)
    assert aligned.data_ptr() % 16 == 0
    buf = torch.empty(n + 4, dtype=aligned.dtype, device='cuda')
    shifted = buf[1:1 + n].view(x.shape)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 16 != 0
    want = pooling.host_pool(x, (1, 5, 9), kind)
    for src in (aligned, shifted):
      got = engine.pool_fields(src, 0, 1, None, 3, *shape, (1, 5, 9), kind)
      pnp.assert_same_bits(got.cpu().numpy()[:, :, 0], want, _ID(shape))


def test_outer_indices_beyond_one_grid_row():
  n_outer, n_member = 4700, 7
  limit = engine.pool_geometry(torch.float32)['max_grid_outer']
  assert n_outer * n_member > limit
  x = cases.field((n_outer, n_member, 3, 8), np.float32)
  for kind in cases.KINDS:
    pnp.assert_same_bits(_members(x, (3,), kind),
                         pooling.host_pool(x, (3,), kind))


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_slab_tables_give_the_bits_of_the_materialised_input(dtype):
  n_row, n_col = 9, 12
  slab = n_row * n_col
  base_host = cases.field((12, n_row, n_col), dtype, 'planted')
  base_dev = _dev(base_host)
  windows = (3, 5)
  # a permuted table; three members at one stride of four slabs
  table = np.array([2, 0, 3, 1])
  got = engine.pool_fields(base_dev, 4 * slab, 3, table, 4, n_row, n_col,
                           windows, 'mean').cpu().numpy()
  picked = np.stack([np.stack([base_host[table[o] + 4 * m] for m in range(3)])
                     for o in range(4)])
  pnp.assert_same_bits(got, pooling.host_pool(picked, windows, 'mean'))
  # pool(): a contiguous tensor, a lead-sliced view and a SlabGather
  lat, lon = cases.grid(n_row, n_col)
  coords = {'time': np.arange(3), 'lead': np.arange(4), 'latitude': lat,
            'longitude': lon}
  dims = ('time', 'lead', 'latitude', 'longitude')
  whole = base_dev.view(3, 4, n_row, n_col)
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    for data, want in (
        (whole, base_host.reshape(3, 4, n_row, n_col)),
        (whole[:, 1:3], base_host.reshape(3, 4, n_row, n_col)[:, 1:3]),
        (xl.SlabGather(base_dev, np.array([[5, 1], [0, 11], [7, 7]])),
         base_host[np.array([[5, 1], [0, 11], [7, 7]])])):
      ds = xl.Dataset({NAME: xl.DataArray(data, dims)},
                      {**coords, 'lead': np.arange(want.shape[1])})
      del calls[:]
      out = pooling.pool(ds, windows, 'max')[NAME]
      # (one launch bracket and nothing else: no copy kernel of this package)
      assert [c[1] for c in calls] == ['pool_fields'] * 2
      assert out.data.is_cuda and out.dims == (NB,) + dims
      pnp.assert_same_bits(out.values, pooling.host_pool(
          np.ascontiguousarray(want), windows, 'max'))
  finally:
    engine.set_launch_hook(old)


def test_two_runs_are_bit_equal():
  x = cases.field((2, 7, 37, 70), np.float32, 'planted')
  for kind in cases.KINDS:
    first = _members(x, ALL_WINDOWS, kind)
    second = _members(x, ALL_WINDOWS, kind)
    np.testing.assert_array_equal(first.view(np.uint32),
                                  second.view(np.uint32))


# ---------------------------------------------------------------------------
# the wrapper on the device
# ---------------------------------------------------------------------------
def _regions():
  return base.product_regions(base.oracle_regions())


def _table_metrics():
  ths = [ConstantThreshold(-0.25), ConstantThreshold(0.5)]
  return {'EventTable': events.EventTable(thresholds=ths),
          'ThresholdWeightedCRPS': tw.ThresholdWeightedCRPS(thresholds=ths),
          'CRPSTable': cd.CRPSTable()}


def _pair(lonlat=False, nan=False, dtype=np.float32):
  ens, truth = cases.ensemble(5, 2, 9, 12, dtype, nan=nan)
  return cases.datasets(ens, truth, lonlat=lonlat)


@pytest.mark.parametrize('lonlat', [False, True], ids=['latlon', 'lonlat'])
@pytest.mark.parametrize('kind', cases.KINDS)
def test_pooled_on_the_device_equals_the_host_path(kind, lonlat):
  forecast, truth = _pair(lonlat, nan=True)
  f_dev, t_dev = _device_dataset(forecast), _device_dataset(truth)
  pooled = pooling.pool(f_dev, (1, 3, 5), kind)[NAME]
  assert pooled.data.is_cuda and pooled.dims == (NB,) + forecast[NAME].dims
  pnp.assert_same_bits(pooled.values,
                       pooling.pool(forecast, (1, 3, 5), kind)[NAME].values)
  regions = _regions()
  metrics = dict(_table_metrics())
  for name, metric in metrics.items():
    wrapped = pooling.Pooled(metric, (3, 5), kind)
    for skipna in (False, True):
      cases.assert_same_dataset(
          wrapped.compute_chunk(f_dev, t_dev, skipna=skipna),
          wrapped.compute_chunk(forecast, truth, skipna=skipna))
    cases.assert_same_dataset(
        wrapped.compute_chunk_regions(f_dev, t_dev, regions, True),
        wrapped.compute_chunk_regions(forecast, truth, regions, True))
  crps = pooling.PooledCRPS((1, 3, 5), kind)
  cases.assert_same_dataset(crps.compute(f_dev, t_dev, skipna=True),
                            crps.compute(forecast, truth, skipna=True))
  cases.assert_same_dataset(
      crps.compute_regions(f_dev, t_dev, regions, True),
      crps.compute_regions(forecast, truth, regions, True))


def _window(ds, n, kind='mean'):
  return pooling.pool(ds, (n,), kind).isel(**{NB: 0})


@pytest.mark.parametrize('name', ['MSE', 'CRPS', 'EventTable',
                                  'ThresholdWeightedCRPS', 'CRPSTable'])
def test_the_composition_law_on_the_device(name):
  metric = {'MSE': gm.MSE(), 'CRPS': gm.CRPS(), **_table_metrics()}[name]
  forecast, truth = _pair()
  f_dev, t_dev = _device_dataset(forecast), _device_dataset(truth)
  if name == 'MSE':  # a deterministic forecast
    f_dev = f_dev.isel(realization=0)
  regions = _regions()
  pooled = pooling.Pooled(metric, (3, 5, 1))
  chunk = pooled.compute_chunk(f_dev, t_dev)
  every = pooled.compute_chunk_regions(f_dev, t_dev, regions)
  whole = pooled.compute(f_dev, t_dev)
  assert chunk[NAME].dims[0] == NB and every[NAME].dims[:2] == (NB, 'region')
  for k, n in enumerate((3, 5, 1)):
    f, t = _window(f_dev, n), _window(t_dev, n)
    pick = lambda ds: ds.isel(**{NB: k})
    cases.assert_same_dataset(pick(chunk), xl.as_dataset(
        metric.compute_chunk(f, t)))
    cases.assert_same_dataset(pick(every), xl.as_dataset(
        metric.compute_chunk_regions(f, t, regions)))
    want = xl.as_dataset(metric.compute(f, t))
    assert whole.attrs == {**want.attrs, 'pooling': 'mean'}
    cases.assert_same_dataset(
        xl.Dataset(dict(pick(whole).data_vars), pick(whole).coords,
                   want.attrs), want)
  cases.assert_same_dataset(chunk.isel(**{NB: 2}), xl.as_dataset(
      metric.compute_chunk(f_dev, t_dev)))


def test_pooled_in_the_evaluation_loops():
  from weatherbench2_amd import config, evaluation
  forecast, truth = _pair()
  f_dev, t_dev = _device_dataset(forecast), _device_dataset(truth)
  regions = _regions()
  metrics = {'pooled_crps': pooling.PooledCRPS((1, 3)),
             'pooled_mse': pooling.Pooled(gm.MSE(), (1, 3), 'max')}
  f_det = f_dev.isel(realization=0)
  for name, metric in metrics.items():
    f = f_det if name == 'pooled_mse' else f_dev
    cfg = config.Eval(metrics={name: metric}, regions=regions)
    res = xl.as_dataset(evaluation._metric_and_region_loop(
        f, t_dev, cfg, False, compute_chunk=True))
    want = xl.as_dataset(metric.compute_chunk_regions(f, t_dev, regions))
    assert res[NAME].dims == ('metric',) + want[NAME].dims
    pnp.assert_same_bits(np.asarray(res[NAME].values)[0],
                         np.asarray(want[NAME].values))
    # chunk by chunk: the time mean of the chunks' results
    chunks = [(f.isel(time=slice(k, k + 1)), t_dev.isel(time=slice(k, k + 1)))
              for k in range(2)]
    mean = xl.as_dataset(evaluation.evaluate_chunks(chunks, cfg, False))
    parts = [np.asarray(xl.as_dataset(metric.compute_chunk_regions(
        cf, ct, regions))[NAME].values, dtype=np.float64)
             for cf, ct in chunks]
    t_ax = want[NAME].dims.index('time')
    direct = np.mean(np.concatenate(parts, axis=t_ax), axis=t_ax)
    got = np.asarray(mean[NAME].values, dtype=np.float64)
    # (the running mean is kept in the dtype of the chunk results: two of its
    # roundings)
    eps = np.finfo(np.asarray(mean[NAME].values).dtype).eps
    np.testing.assert_allclose(got.reshape(direct.shape), direct,
                               rtol=2 * eps, atol=0)


def test_device_backed_refusals_come_before_any_launch():
  forecast, truth = _pair()
  f_dev, t_dev = _device_dataset(forecast), _device_dataset(truth)
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    half = xl.Dataset({NAME: xl.DataArray(f_dev[NAME].data.half(),
                                          f_dev[NAME].dims)}, f_dev.coords)
    regional = xl.Dataset(dict(f_dev.data_vars),
                          {**f_dev.coords, 'longitude': np.arange(12) * 10.0})
    wide = xl.Dataset(
        {NAME: xl.DataArray(torch.zeros(1, 3, 200, device='cuda'),
                            ('time', 'latitude', 'longitude'))},
        {'time': np.arange(1), 'latitude': cases.grid(3, 200)[0],
         'longitude': cases.grid(3, 200)[1]})
    limit = engine.pool_geometry(torch.float32)['max_window']
    for call, match in (
        (lambda: pooling.pool(f_dev, (3,), 'median'), "pooling='median'"),
        (lambda: pooling.pool(f_dev, (4,)), 'window 4'),
        (lambda: pooling.pool(f_dev, (13,)), 'window 13'),
        (lambda: pooling.pool(f_dev, (3, 3)), 'duplicate'),
        (lambda: pooling.pool(regional, (3,)), 'not cyclic'),
        (lambda: pooling.pool(half, (3,)), 'float32 and float64'),
        (lambda: pooling.pool(wide, (limit + 2,)), f'up to {limit}'),
        (lambda: pooling.Pooled(gm.MSE(), (2,)).compute_chunk(
            f_dev.isel(realization=0), t_dev), 'window 2')):
      with pytest.raises(ValueError, match=match):
        call()
      assert not calls, match
    # the entry point's own refusals, with device operands
    x = f_dev[NAME].data
    for kwargs, match in ((dict(windows=(4,)), 'window=4'),
                          (dict(windows=(13,)), 'window=13'),
                          (dict(windows=(limit + 2,), n_col=200,
                                x=wide[NAME].data, n_outer=1, n_row=3),
                           'max_window'),
                          (dict(n_member=129), 'n_member=')):
      args = dict(x=x, n_member=1, n_outer=10, n_row=9, n_col=12,
                  windows=(3,))
      args.update(kwargs)
      with pytest.raises(engine._lib.Wb2HipError, match=match):
        engine.pool_fields(args['x'], 0, args['n_member'], None,
                           args['n_outer'], args['n_row'], args['n_col'],
                           args['windows'], 'mean')
    assert pooling.pool(wide, (limit,))[NAME].shape == (1, 1, 3, 200)
  finally:
    engine.set_launch_hook(old)
