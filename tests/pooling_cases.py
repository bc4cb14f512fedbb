"""Shared cases of tests/test_pooling_cpu.py and tests/test_pooling_gpu.py:
seeded, all small."""
import numpy as np

from weatherbench2_amd import xarray_lite as xl

NAME = 'geopotential'
DTYPES = (np.float32, np.float64)
KINDS = ('mean', 'max')
# (slab shape, windows): 11 > n_row = 9 clips at both poles, 9 == n_col wraps
# the whole row
SLABS = (((9, 12), (1, 3, 5, 11)), ((7, 9), (9,)), ((37, 70), (3, 17)))
SPECIALS = ('none', 'planted', 'zeros')


def grid(n_lat, n_lon):
  return (np.linspace(-90.0, 90.0, n_lat),
          np.linspace(0.0, 360.0, n_lon, endpoint=False))


def field(shape, dtype, special='none', seed=0, extra=()):
  """A field [..., n_row, n_col] of `dtype`.  'planted': NaN in a corner, +inf
  in a pole row, -inf and -0.0 on either side of the longitude seam and NaN /
  -0.0 at the positions `extra` (tile borders), in every slab.  'zeros':
  -0.0, +0.0 and -1.0 at random, so that the sign of a zero maximum is at
  stake in most windows."""
  rs = np.random.RandomState(seed + 7 * shape[-1] + shape[-2])
  if special == 'zeros':
    return rs.choice(np.array([-0.0, 0.0, -1.0], dtype=dtype), size=shape)
  x = rs.normal(size=shape).astype(dtype)
  if special == 'planted':
    n_row, n_col = shape[-2:]
    x[..., 0, 0] = np.nan
    x[..., n_row - 1, n_col // 2] = np.inf
    x[..., n_row // 2, n_col - 1] = -np.inf
    x[..., n_row // 2 + 1, 0] = -0.0
    x[..., n_row // 2 + 1, n_col - 1] = -0.0
    for k, (i, j) in enumerate(extra):
      if i < n_row and j < n_col:
        x[..., i, j] = np.nan if k % 2 == 0 else -0.0
  return x


def ensemble(n_member, n_time, n_lat, n_lon, dtype, seed=0, nan=False):
  """(ens [M, T, lat, lon], truth [T, lat, lon]) on a 0.25 grid of values."""
  rs = np.random.RandomState(seed + 17 * n_member + n_lat)
  ens = (np.round(rs.normal(size=(n_member, n_time, n_lat, n_lon)) * 4) / 4
         ).astype(dtype)
  truth = (np.round(rs.normal(size=(n_time, n_lat, n_lon)) * 5) / 4
           ).astype(dtype)
  if nan:
    truth[0, n_lat // 2, 1] = np.nan
    ens[0, -1, 1, n_lon - 1] = np.nan
  return ens, truth


def datasets(ens, truth, lonlat=False):
  """Product (forecast, truth) of such arrays on the host; `lonlat`: the
  variables as (..., longitude, latitude)."""
  n_member, n_time, n_lat, n_lon = ens.shape
  lat, lon = grid(n_lat, n_lon)
  coords = {'latitude': lat, 'longitude': lon, 'time': np.arange(n_time),
            'realization': np.arange(n_member)}
  dims = ('realization', 'time', 'latitude', 'longitude')
  if lonlat:
    ens = np.ascontiguousarray(np.swapaxes(ens, -1, -2))
    truth = np.ascontiguousarray(np.swapaxes(truth, -1, -2))
    dims = dims[:2] + dims[:1:-1]
  forecast = xl.Dataset({NAME: xl.DataArray(ens, dims)}, coords)
  coords = {k: v for k, v in coords.items() if k != 'realization'}
  return forecast, xl.Dataset({NAME: xl.DataArray(truth, dims[1:])}, coords)


def assert_same_dataset(got, want, drop=()):
  """Dims, coordinates, dtypes, attributes and every bit of the data (NaNs
  as one pattern); `drop`: coordinates of `got` that `want` need not have."""
  from tests import pooling_np
  assert list(got.data_vars) == list(want.data_vars)
  assert got.attrs == want.attrs
  assert set(got.coords) - set(drop) == set(want.coords) - set(drop)
  for k in set(want.coords) - set(drop):
    a, b = got[k], want[k]
    assert a.dims == b.dims, k
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values),
                                  err_msg=k)
  for k in want.data_vars:
    a, b = got[k], want[k]
    assert a.dims == b.dims and a.dtype == b.dtype, (k, a.dims, b.dims)
    pooling_np.assert_same_bits(np.asarray(a.values), np.asarray(b.values), k)
