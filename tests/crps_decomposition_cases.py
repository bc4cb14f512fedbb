"""Shared cases of tests/test_crps_decomposition_cpu.py and
tests/test_crps_decomposition_gpu.py: seeded, all small."""
import numpy as np

from oracle import regions_np as oreg
from oracle.named import DS, NA
from tests import helpers

NAME = 'geopotential'
GRIDS = ((5, 8), (19, 72))
MEMBERS = (1, 2, 3, 7, 33, 50, 64)
DTYPES = (np.float32, np.float64)
NANS = ('none', 'truth', 'member', 'both')
DIMS = ('realization', 'time', 'latitude', 'longitude')


def grid(n_lat, n_lon):
  return (np.linspace(-90.0, 90.0, n_lat),
          np.linspace(0.0, 360.0, n_lon, endpoint=False))


def arrays(n_member, n_time, n_lat, n_lon, dtype, nan='none', seed=0):
  """(ens [M, T, lat, lon], truth [T, lat, lon]) of `dtype`: values on a 0.25
  grid (ties occur by themselves) with NaNs in the truth, in one member of a
  point, or both."""
  rs = np.random.RandomState(seed + 17 * n_member + n_lat)
  ens = (np.round(rs.normal(size=(n_member, n_time, n_lat, n_lon)) * 4) / 4
         ).astype(dtype)
  truth = (np.round(rs.normal(size=(n_time, n_lat, n_lon)) * 5) / 4
           ).astype(dtype)
  if nan in ('truth', 'both'):
    truth[rs.rand(*truth.shape) < 0.08] = np.nan
  if nan in ('member', 'both'):
    hit = rs.rand(*truth.shape) < 0.08
    member = rs.randint(n_member, size=truth.shape)
    for idx in zip(*np.nonzero(hit)):
      ens[(member[idx],) + idx] = np.nan
  return ens, truth


def datasets(ens, truth):
  """Oracle (forecast, truth) of such arrays."""
  n_member, n_time, n_lat, n_lon = ens.shape
  lat, lon = grid(n_lat, n_lon)
  coords = {'latitude': lat, 'longitude': lon, 'time': np.arange(n_time),
            'realization': np.arange(n_member)}
  forecast = DS({NAME: NA(ens, DIMS)}, coords)
  coords = {k: v for k, v in coords.items() if k != 'realization'}
  return forecast, DS({NAME: NA(truth, DIMS[1:])}, coords)


def tie_case(dtype, n_lat=5, n_lon=8, n_member=4):
  """(ens, truth, below [T, lat, lon], above) with exact ties planted by hand:
  row 0 truth == an inner member, row 1 truth == the lowest member, row 2
  truth == the highest, row 3 duplicated members around the truth, row 4 all
  members equal (truth below, equal, above by column).  `below` / `above` are
  the hand-counted indicators."""
  ens = np.empty((n_member, 1, n_lat, n_lon), dtype=dtype)
  base = np.array([3.0, -1.0, 0.5, 2.0], dtype=dtype)[:n_member]
  ens[:] = base[:, None, None, None]
  truth = np.zeros((1, n_lat, n_lon), dtype=dtype)
  below = np.zeros(truth.shape, dtype=bool)
  above = np.zeros(truth.shape, dtype=bool)
  truth[0, 0] = 0.5    # equals an inner member: no outlier
  truth[0, 1] = -1.0   # equals the lowest: not below
  truth[0, 2] = 3.0    # equals the highest: not above
  ens[:, 0, 3] = np.array([1.0, 1.0, 2.0, 2.0], dtype=dtype)[:, None]
  truth[0, 3] = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 1.0, 2.0, 3.0], dtype=dtype)
  below[0, 3] = truth[0, 3] < 1.0
  above[0, 3] = truth[0, 3] > 2.0
  ens[:, 0, 4] = 1.25
  truth[0, 4] = np.array([1.0, 1.25, 1.5, 1.25, 0.0, 2.0, 1.25, 1.25],
                         dtype=dtype)
  below[0, 4] = truth[0, 4] < 1.25
  above[0, 4] = truth[0, 4] > 1.25
  return ens, truth, below, above


def oracle_regions():
  regions = dict(helpers.predefined_regions(oracle=True))
  regions['overlap'] = oreg.SliceRegion(lat_slice=[slice(None, 10),
                                                   slice(-10, None)])
  regions['extra-tropical'] = oreg.ExtraTropicalRegion()
  return regions


def product_regions(regions):
  return {k: helpers.to_gpu_region(v) for k, v in regions.items()}


def classes(n_col, n_class):
  """Column classes in runs, the first class wrapping round the row end (as
  `europe` does): class of column j = ((j + shift) % n_col) * n_class //
  n_col with a shift of a third of a run (at least one column)."""
  shift = max(1, n_col // (3 * n_class))
  return (((np.arange(n_col) + shift) % n_col) * n_class // n_col
          ).astype(np.int32)


def assert_same_dataset(got, want):
  """Dims, coordinates, dtypes, attributes and every bit of the data."""
  assert list(got.data_vars) == list(want.data_vars)
  assert got.attrs == want.attrs
  assert set(got.coords) == set(want.coords)
  for k in want.coords:
    a, b = got[k], want[k]
    assert a.dims == b.dims, k
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values),
                                  err_msg=k)
  for k in want.data_vars:
    a, b = got[k], want[k]
    assert a.dims == b.dims and a.dtype == b.dtype, k
    np.testing.assert_array_equal(
        np.asarray(a.values).view(np.uint64),
        np.asarray(b.values).view(np.uint64), err_msg=k)
