"""Shared cases of tests/test_events_cpu.py and tests/test_events_gpu.py."""
import dataclasses
import itertools

import numpy as np

from oracle import fixtures
from oracle import regions_np as oreg
from oracle import thresholds_np as oth
from tests import helpers
from tests.test_oracle_thresholds import _clim_like, _merge
from weatherbench2_amd import thresholds as gth
from weatherbench2_amd import xarray_lite as xl

NAME = 'geopotential'
QUANTILES = (0.2, 0.6)
SPATIAL = ('latitude', 'longitude')


def edge_case(n_member, n_thr, n_outer, n_row, n_col, dtype, seed=0):
  """(ens [M, O, R, C], truth [O, R, C], [thr [O, R, C]] * T) of `dtype`:
  values on a 0.1 grid (so equalities occur by themselves) with NaN in the
  truth, in one member and in the threshold, +-inf and planted equalities at
  the first and last columns of a row and around the 16-byte lane borders
  (columns 0..5 and the last four), cycling over rows and outer indices."""
  rs = np.random.RandomState(seed)
  grid = lambda shape, shift=0.0: (np.round(rs.normal(size=shape), 1) + shift
                                   ).astype(dtype)
  ens = grid((n_member, n_outer, n_row, n_col))
  truth = grid((n_outer, n_row, n_col))
  thrs = [grid((n_outer, n_row, n_col), 0.3 * t - 0.2) for t in range(n_thr)]
  cols = sorted({c for c in list(range(6)) + list(range(n_col - 4, n_col))
                 if 0 <= c < n_col})
  inf, nan = dtype(np.inf), dtype(np.nan)
  for n, (o, r, c) in enumerate(itertools.product(
      range(n_outer), range(n_row), cols)):
    kind, m, thr = n % 9, n % n_member, thrs[n % n_thr]
    if kind == 0:
      truth[o, r, c] = nan
    elif kind == 1:
      ens[m, o, r, c] = nan
    elif kind == 2:
      thr[o, r, c] = nan
    elif kind == 3:
      ens[m, o, r, c] = inf
    elif kind == 4:
      truth[o, r, c] = -inf
    elif kind == 5:
      ens[m, o, r, c] = thr[o, r, c] = inf  # equal at infinity: no exceedance
    elif kind == 6:
      ens[m, o, r, c] = thr[o, r, c]
    elif kind == 7:
      truth[o, r, c] = thr[o, r, c]
    else:
      truth[o, r, c] = thr[o, r, c] = nan
  return ens, truth, thrs


def classes(n_col, n_class):
  """Non-contiguous column classes: class = column mod n_class, rotated."""
  return ((np.arange(n_col) + 1) % n_class).astype(np.int32)


def random_case(ensemble_size=None, nan_frac=0.0, truth_only=False):
  """tests/test_thresholds_gpu.py::_random_case: oracle (truth, forecast,
  climatology) on a 10-degree grid, leads 0..2 days."""
  truth, forecast = fixtures.get_random_truth_and_forecast(
      ensemble_size=ensemble_size, spatial_resolution_in_degrees=10,
      lead_stop='2 day')
  doy = {'dayofyear': 1 + np.arange(366)}
  zero = truth.zeros_like()
  clim = _merge(_clim_like(zero + 0.1, doy),
                _clim_like(zero + 0.9, doy, {NAME: NAME + '_std'}))
  if nan_frac:
    if not truth_only:
      forecast = fixtures.insert_nan(forecast, nan_frac, seed=9)
    truth = fixtures.insert_nan(truth, nan_frac / 2, seed=10)
  return truth, forecast, clim


def oracle_regions():
  regions = dict(helpers.predefined_regions(oracle=True))
  regions['overlap'] = oreg.SliceRegion(lat_slice=[slice(None, 10),
                                                   slice(-10, None)])
  regions['extra-tropical'] = oreg.ExtraTropicalRegion()
  return regions


def product_regions(regions):
  return {k: helpers.to_gpu_region(v) for k, v in regions.items()}


def oracle_thresholds(clim):
  return [oth.GaussianQuantileThreshold(clim, q) for q in QUANTILES]


def product_thresholds(clim):
  return [gth.GaussianQuantileThreshold(
      climatology=helpers.to_gpu_dataset(clim), quantile=q) for q in QUANTILES]


def dense_operands(forecast, truth, threshold, ensemble_dim='realization'):
  """(outer dims, ens [M, outer..., lat, lon], truth, thr [outer..., lat,
  lon]) of oracle variables (NA): everything broadcast to the forecast's outer
  dims, in the forecast's order."""
  outer = tuple(d for d in forecast.dims
                if d != ensemble_dim and d not in SPATIAL)
  sizes = forecast.sizes

  def spread(na, lead=()):
    have = tuple(d for d in lead + outer + SPATIAL if d in na.dims)
    data = na.transpose(*have).data
    shape = [sizes[d] if d in na.dims else 1 for d in lead + outer + SPATIAL]
    full = [sizes[d] for d in lead + outer + SPATIAL]
    return np.broadcast_to(data.reshape(shape), full).astype(np.float64)

  if ensemble_dim in forecast.dims:
    ens = spread(forecast, (ensemble_dim,))
  else:
    ens = spread(forecast)[None]
  return outer, ens, spread(truth), spread(threshold)


@dataclasses.dataclass
class FieldThreshold(gth.Threshold):
  """A threshold that is a given Dataset of fields (`climatology`)."""

  def compute(self, truth):
    return self.climatology


def assert_same_dataset(got: xl.Dataset, want: xl.Dataset):
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
