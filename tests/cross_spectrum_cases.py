"""Shared cases of tests/test_cross_spectrum_cpu.py and
tests/test_cross_spectrum_gpu.py: seeded, all small.  Rows are N(0, 1) + 3
(a mean, so that bin 0 is not small) and the forecast is correlated with the
truth, member by member."""
import numpy as np

from oracle import regions_np as oreg
from oracle.named import DS, NA
from tests import helpers

NAME = 'geopotential'
DTYPES = (np.float32, np.float64)
DIMS = ('realization', 'time', 'latitude', 'longitude')


def grid(n_lat, n_lon):
  """Latitudes with both poles, a cyclic longitude axis."""
  return (np.linspace(-90.0, 90.0, n_lat),
          np.linspace(0.0, 360.0, n_lon, endpoint=False))


def arrays(n_member, n_time, n_lat, n_lon, dtype, seed=0):
  """(ens [M, T, lat, lon], truth [T, lat, lon]) of `dtype`."""
  rs = np.random.RandomState(seed + 31 * n_member + n_lon)
  truth = rs.normal(size=(n_time, n_lat, n_lon)) + 3.0
  ens = (0.8 * (truth - 3.0) + 3.0 +
         0.6 * rs.normal(size=(n_member, n_time, n_lat, n_lon)))
  return ens.astype(dtype), truth.astype(dtype)


def datasets(ens, truth, ensemble=True):
  """Oracle (forecast, truth) of such arrays; ensemble=False (one member):
  the forecast has no ensemble dim."""
  n_member, n_time, n_lat, n_lon = ens.shape
  lat, lon = grid(n_lat, n_lon)
  coords = {'latitude': lat, 'longitude': lon, 'time': np.arange(n_time)}
  tru = DS({NAME: NA(truth, DIMS[1:])}, dict(coords))
  if not ensemble:
    assert n_member == 1
    return DS({NAME: NA(ens[0], DIMS[1:])}, dict(coords)), tru
  coords['realization'] = np.arange(n_member)
  return DS({NAME: NA(ens, DIMS)}, coords), tru


def oracle_regions():
  """Latitude bands only: global, tropics and both extratropics."""
  every = helpers.predefined_regions(oracle=True)
  return {k: every[k] for k in ('global', 'tropics', 'northern-hemisphere',
                                'southern-hemisphere')}


def overlap_regions():
  """A latitude-slice list whose slices overlap (rows counted twice)."""
  return {'overlap': oreg.SliceRegion(lat_slice=[slice(None, 10),
                                                 slice(-10, None)]),
          'global': oreg.SliceRegion()}


def product_regions(regions):
  return {k: helpers.to_gpu_region(v) for k, v in regions.items()}
