"""Shared cases of tests/test_neighborhood_cpu.py and
tests/test_neighborhood_gpu.py.

Values lie on a 0.1 grid so that ties with the threshold occur by themselves;
NaNs sit in the truth and in single members, and `edge_case` (the builder of
the event-table tests) adds a NaN threshold, +-inf and planted equalities."""
import numpy as np

from tests import events_cases
from weatherbench2_amd import xarray_lite as xl

NAME = events_cases.NAME
edge_case = events_cases.edge_case
classes = events_cases.classes
random_case = events_cases.random_case
oracle_regions = events_cases.oracle_regions
product_regions = events_cases.product_regions
product_thresholds = events_cases.product_thresholds
oracle_thresholds = events_cases.oracle_thresholds
dense_operands = events_cases.dense_operands
assert_same_dataset = events_cases.assert_same_dataset
FieldThreshold = events_cases.FieldThreshold
QUANTILES = events_cases.QUANTILES


def axes(n_row, n_col):
  """Increasing latitudes and a cyclic longitude axis."""
  lat = np.linspace(-80.0, 80.0, n_row)
  lon = np.arange(n_col) * (360.0 / n_col)
  return lat, lon


def code_plane(n_cell, n_row, n_col, n_member, seed=0, invalid=0.1):
  """A uint16 code plane [n_cell, n_row, n_col] as wb2_event_codes writes it:
  k in 0..n_member, the observed bit, `invalid` of the points invalid (code
  0x200), the corners among them, and one row without any event."""
  rs = np.random.RandomState(seed)
  k = rs.randint(0, n_member + 1, size=(n_cell, n_row, n_col))
  k[rs.rand(n_cell, n_row, n_col) < 0.3] = n_member  # the extreme is common
  obs = rs.randint(0, 2, size=k.shape)
  code = k | obs << 8
  code[:, n_row // 2] = 0
  bad = rs.rand(*k.shape) < invalid
  bad[:, 0, 0] = bad[:, -1, -1] = True
  return np.where(bad, 0x200, code).astype(np.uint16)


def small_case(n_member, n_row, n_col, n_time=2, dtype=np.float32, seed=0,
               nan_frac=0.1):
  """Host (forecast, truth, threshold field) Datasets of one variable 'x':
  forecast (realization, time, latitude, longitude) -- without the
  realization dim when n_member is None --, truth (time, latitude,
  longitude) and a threshold field (time, latitude, longitude)."""
  rs = np.random.RandomState(seed)
  lat, lon = axes(n_row, n_col)
  coords = {'time': np.arange(n_time).astype('datetime64[D]').astype(
      'datetime64[ns]'), 'latitude': lat, 'longitude': lon}
  m = n_member or 1
  full = np.round(rs.normal(size=(m, n_time, n_row, n_col)), 1).astype(dtype)
  tru = np.round(rs.normal(size=(n_time, n_row, n_col)), 1).astype(dtype)
  thr = np.round(rs.normal(size=(n_time, n_row, n_col)) * 0.5, 1).astype(dtype)
  tru[rs.rand(*tru.shape) < nan_frac / 2] = np.nan
  for t in range(n_time):  # NaNs in single members
    hit = rs.rand(n_row, n_col) < nan_frac / 2
    full[rs.randint(m), t][hit] = np.nan
  dims = ('time', 'latitude', 'longitude')
  if n_member is None:
    forecast = xl.Dataset({'x': xl.DataArray(full[0], dims)}, coords)
  else:
    forecast = xl.Dataset(
        {'x': xl.DataArray(full, ('realization',) + dims)},
        dict(coords, realization=np.arange(m)))
  truth = xl.Dataset({'x': xl.DataArray(tru, dims)}, coords)
  field = xl.Dataset({'x': xl.DataArray(thr, dims)}, coords)
  return forecast, truth, field


def single_events(n_row, n_col, row, jf, jo):
  """Deterministic (forecast, truth) Datasets of zeros with one event point
  (value 1) in the forecast at (row, jf) and one in the truth at (row, jo)."""
  lat, lon = axes(n_row, n_col)
  coords = {'time': np.array(['2020-01-01'], 'datetime64[ns]'),
            'latitude': lat, 'longitude': lon}
  dims = ('time', 'latitude', 'longitude')
  f = np.zeros((1, n_row, n_col))
  o = np.zeros((1, n_row, n_col))
  f[0, row, jf] = 1.0
  o[0, row, jo] = 1.0
  return (xl.Dataset({'x': xl.DataArray(f, dims)}, coords),
          xl.Dataset({'x': xl.DataArray(o, dims)}, coords))
