"""Shared cases of tests/test_bootstrap_cpu.py and tests/test_bootstrap_gpu.py:
seeded, all small."""
import functools

import numpy as np

from tests import pooling_cases
from weatherbench2_amd import bootstrap
from weatherbench2_amd import events
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.neighborhood import ConstantThreshold

NAME = pooling_cases.NAME
DTYPES = (np.float32, np.float64)
SPECIALS = ('none', 'planted')


def plan(n_rep, n_time, seed=0):
  """int32 [n_rep, n_time] counts of a block bootstrap with these edges: the
  counts of replicate 0 are all zero but one; the last replicate (if there is
  a second one) does not draw the last time."""
  counts = bootstrap.block_plan(n_time, n_rep, min(2, n_time), seed)
  counts[0] = 0
  counts[0, n_time // 2] = n_time
  if n_rep > 1 and n_time > 1:
    counts[-1, 0] += counts[-1, -1]
    counts[-1, -1] = 0
  return counts


def series(shape, dtype, special='none', seed=0):
  """[n_outer, n_time, n_point] of `dtype`.  'planted': at the LAST time (which
  replicate 0 and the last replicate of `plan` do not draw, others do) a NaN
  and a +inf, at the middle time (which replicate 0 draws) a -inf and a NaN,
  and a -0.0, each at another point where there are enough."""
  n_outer, n_time, n_point = shape
  rs = np.random.RandomState(seed + 31 * n_time + n_point)
  x = rs.normal(size=shape).astype(dtype)
  if special == 'planted':
    last, mid = n_time - 1, n_time // 2
    x[0, last, 0] = np.nan
    x[-1, last, n_point - 1] = np.inf
    x[0, mid, n_point // 2] = -np.inf
    x[-1, mid, (n_point - 1) // 3] = np.nan
    x[0, 0, (2 * n_point) // 3] = -0.0
  return x


def dataset(arrays: dict, dims: dict, coords: dict, attrs=None) -> xl.Dataset:
  return xl.Dataset({k: xl.DataArray(a, dims[k]) for k, a in arrays.items()},
                    coords, attrs)


THRESHOLDS = (ConstantThreshold(-0.25), ConstantThreshold(0.5))


@functools.lru_cache(maxsize=None)
def forecasts(n_time=6):
  """Two 4-member 8 x 16 forecasts and their truth, on the host."""
  ens, truth = pooling_cases.ensemble(4, n_time, 8, 16, np.float32)
  other, _ = pooling_cases.ensemble(4, n_time, 8, 16, np.float32, seed=5)
  forecast, tru = pooling_cases.datasets(ens, truth)
  rival, _ = pooling_cases.datasets(other, truth)
  return forecast, rival, tru


@functools.lru_cache(maxsize=None)
def event_tables(n_time=6):
  """Per-time `EventTable` tables of the two forecasts (host)."""
  forecast, rival, truth = forecasts(n_time)
  metric = events.EventTable(thresholds=list(THRESHOLDS))
  return (metric.compute_chunk(forecast, truth),
          metric.compute_chunk(rival, truth))


def assert_same_dataset(got, want):
  """Dims, coordinates, dtypes, attributes and every bit of the data (NaNs
  as one pattern)."""
  from tests import bootstrap_np
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
    assert a.dims == b.dims, (k, a.dims, b.dims)
    bootstrap_np.assert_same_bits(np.asarray(a.values), np.asarray(b.values),
                                  k)
