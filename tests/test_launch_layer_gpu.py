"""The entry forms of the deterministic reduction against each other and the
NumPy oracle at the smallest grids the launch layer distinguishes: one launch
of K1 + K2 however it is spelled -- stream_reduce without and with slab
tables, stream_reduce_addr, SuiteStep by inputs and by address, PairSuiteStep
without pairs -- gives the SAME BITS, and those agree with oracle/metrics_np.py
(MSE, RMSE, MAE, Bias; ACC through a climatology for MODE_DET_ACC) at the
tolerance of tests/test_det_gpu.py."""
import functools

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

N_OUTER = 3
GRIDS = [(6, 7),   # float32: one full 4-wide vector + a shifted last lane
         (6, 3),   # one column per lane
         (5, 3)]
SUITE = ('mse', 'rmse', 'mae', 'bias')


def _coords(n_lat, n_lon):
  return np.linspace(-75, 75, n_lat), np.arange(n_lon) * (360.0 / n_lon)


@functools.lru_cache(maxsize=None)
def _data_and_oracle(n_lat, n_lon, dtype, land):
  """((f, t, c) host arrays, {metric: [n_region, N_OUTER]}, oracle regions):
  computed once per grid, shared by the modes."""
  from oracle import metrics_np as om
  from oracle import regions_np as oreg
  from oracle.named import DS, NA
  lat, lon = _coords(n_lat, n_lon)
  rs = np.random.RandomState(17 * n_lat + n_lon)
  f, t, c = (rs.normal(size=(N_OUTER, n_lat, n_lon)).astype(dtype)
             for _ in range(3))
  regions = {'global': oreg.SliceRegion(),
             'tropics': oreg.SliceRegion(lat_slice=slice(-20, 20)),
             'east': oreg.SliceRegion(lon_slice=slice(100, 300))}
  if land:
    lsm = (rs.uniform(size=(n_lat, n_lon)) > 0.4).astype(np.float32)
    regions['land'] = oreg.LandRegion(NA(lsm, ('latitude', 'longitude')), lat,
                                      lon)
  coords = {'level': np.arange(N_OUTER), 'latitude': lat, 'longitude': lon}
  dims = ('level', 'latitude', 'longitude')
  fd, td = (DS({'z': NA(x, dims)}, coords) for x in (f, t))
  # ACC as the reference computes it: the climatology selected at the valid
  # time's (dayofyear, hour)
  day = np.datetime64('2020-01-03T00', 'ns')
  tcoords = dict(coords, time=np.array([day]))
  ft, tt = (DS({'z': NA(x[None], ('time',) + dims)}, tcoords) for x in (f, t))
  clim = DS({'z': NA(np.stack([c + 1, c + 2, c, c - 1])[None],
                     ('hour', 'dayofyear') + dims)},
            dict(coords, hour=np.array([0]), dayofyear=np.arange(1, 5)))
  metrics = {'mse': om.MSE(), 'rmse': om.RMSESqrtBeforeTimeAvg(),
             'mae': om.MAE(), 'bias': om.Bias()}
  want = {m: np.stack([metric.compute_chunk(fd, td, region=r)['z'].data
                       for r in regions.values()])
          for m, metric in metrics.items()}
  want['acc'] = np.stack([
      om.ACC(clim).compute_chunk(ft, tt, region=r)['z'].data[0]
      for r in regions.values()])
  return (f, t, c), want, regions


@pytest.mark.parametrize('land', [False, True], ids=['global', 'land'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('mode_name', ['DET', 'DET_ACC'])
def test_entry_forms_give_the_same_bits_and_the_oracle(mode_name, grid, dtype,
                                                       land):
  import torch
  from weatherbench2_amd import _lib, engine, plan as plan_lib
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  dev = torch.device('cuda')
  mode = getattr(_lib, 'MODE_' + mode_name)
  tdt = getattr(torch, dtype)
  arrays, want, oregions = _data_and_oracle(*grid, dtype, land)
  pl = plan_lib.build_plan(
      *_coords(*grid), plan_lib.LATLON,
      {k: helpers.to_gpu_region(r) for k, r in oregions.items()}, dev,
      rows_per_chunk=5)
  assert (pl.wfield is not None) == land == (pl.wfield32 is not None)
  ins = [torch.as_tensor(x, device=dev)
         for x in arrays[:3 if mode == _lib.MODE_DET_ACC else 2]]
  ident = [torch.arange(N_OUTER, device=dev) for _ in ins]
  size = grid[0] * grid[1] * ins[0].element_size()
  addr = [x.data_ptr() + tab * size for x, tab in zip(ins, ident)]
  aligned = all(not bool((a % 16).any().item()) for a in addr)
  step = lambda **kw: engine.SuiteStep(pl, mode, tdt, False, N_OUTER, **kw)
  got = {
      'stream_reduce': engine.stream_reduce(
          pl, mode, ins, [None] * len(ins), N_OUTER, False)[0],
      'stream_reduce-slabs': engine.stream_reduce(
          pl, mode, ins, ident, N_OUTER, False)[0],
      'stream_reduce_addr': engine.stream_reduce_addr(
          pl, mode, tdt, addr, aligned, N_OUTER, False)[0],
      'SuiteStep.run': step().run(ins, ident).clone(),
      'SuiteStep.run-addr': step(aligned=aligned, by_address=True).run(
          None, addr).clone(),
      'PairSuiteStep-no-pairs': engine.PairSuiteStep(
          pl, mode, tdt, False, N_OUTER, 0).run(ins, ident)[0],
  }
  first = got['stream_reduce']
  assert first.shape == (_lib.NMETRIC, pl.n_region, N_OUTER)
  for name, value in got.items():
    assert torch.equal(torch.nan_to_num(value, nan=-7.0),
                       torch.nan_to_num(first, nan=-7.0)), name
  host = first.cpu().numpy()
  for m in SUITE + (('acc',) if mode == _lib.MODE_DET_ACC else ()):
    helpers.assert_close(host[_lib.METRIC_INDEX[m]], want[m], rtol=1e-9,
                         atol=1e-12, err_msg=m)
