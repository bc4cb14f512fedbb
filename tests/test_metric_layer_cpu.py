"""The shared pieces of the metric layer (weatherbench2_amd/metrics.py) that
need no device: dim ordering, the time-average dim, the common float dtype,
the ensemble outer layout and the per-class region dispatch."""
import itertools

import numpy as np
import pytest
import torch

from weatherbench2_amd import metrics as gm
from weatherbench2_amd import plan as plan_lib
from weatherbench2_amd import xarray_lite as xl

DIMS = ('region', 'time', 'lead_time', 'level', 'realization')


# --- _order_by against the three permutations that used to be written out ---
def _old_scalar(lead, dims, values, truth_dims):     # EnsembleMetric
  tdims = [d for d in truth_dims if d in dims]
  order = lead + tuple(
      tdims + [d for d in dims if d not in tdims and d not in lead])
  return order, np.transpose(values, [dims.index(d) for d in order])


def _old_map(dims, values, truth_dims):   # both Spatial* ensemble families
  tdims = [d for d in truth_dims if d in dims]
  order = tuple(tdims + [d for d in dims if d not in tdims])
  return order, np.transpose(values, [dims.index(d) for d in order])


def _truth_dim_sets(dims):
  """Subsets, reorderings and a set with a dim the result lacks."""
  missing = next((d for d in DIMS[1:] if d not in dims), 'hour')
  out = [(), dims, dims[::-1], dims[1:], dims[:1], dims[::2],
         (missing,) + dims[::-1], dims[:2] + (missing,)]
  return out


def _values(dims):
  shape = tuple(2 + i for i in range(len(dims)))
  return np.arange(int(np.prod(shape))).reshape(shape)


def test_order_by_equals_the_map_permutations():
  n = 0
  for k in (3, 4):
    for dims in itertools.permutations(DIMS, k):
      values = _values(dims)
      for tdims in _truth_dim_sets(dims):
        want = _old_map(dims, values, tdims)
        got = gm._order_by(dims, values, (tdims,))
        assert tuple(got[0]) == want[0], (dims, tdims)
        np.testing.assert_array_equal(got[1], want[1])
        n += 1
  assert n > 1000


def test_order_by_equals_the_scalar_permutation():
  """Precedence (lead, truth dims); `lead` is () or the new ('region',) dim,
  which the truth then cannot have: the result's other dims and the truth's
  are drawn from the remaining names."""
  for lead in ((), ('region',)):
    pool = DIMS if not lead else DIMS[1:]
    for k in (3, 4):
      for rest in itertools.permutations(pool, k - len(lead)):
        dims = lead + rest
        values = _values(dims)
        for tdims in _truth_dim_sets(rest):
          want = _old_scalar(lead, dims, values, tdims)
          got = gm._order_by(dims, values, (lead, tdims))
          assert tuple(got[0]) == want[0], (lead, dims, tdims)
          np.testing.assert_array_equal(got[1], want[1])


# --- the time-average dim ---------------------------------------------------
def _ds(dims, shape=None, dtype=np.float32):
  shape = shape or tuple(2 + i for i in range(len(dims)))
  coords = {d: np.arange(n) for d, n in zip(dims, shape)}
  return xl.Dataset({'z': xl.DataArray(np.zeros(shape, dtype), dims)}, coords)


def test_time_average_dim():
  assert gm._time_average_dim(_ds(('init_time', 'time'))) == 'time'
  assert gm._time_average_dim(_ds(('time', 'level'))) == 'time'
  assert gm._time_average_dim(_ds(('level', 'init_time'))) == 'init_time'
  ds = _ds(('level',))
  with pytest.raises(ValueError) as e:
    gm._time_average_dim(ds)
  assert str(e.value) == (
      f'Forecast has neither valid_time or init_time dimension {ds}')


# --- the common float dtype -------------------------------------------------
def _geo(n_lat=3, n_lon=4, layout=plan_lib.LATLON):
  return gm._Geometry(layout, ('time',), (2,), np.linspace(-60, 60, n_lat),
                      np.arange(n_lon) * 10.0)


@pytest.mark.parametrize('a,b,want', [
    (torch.float32, torch.float32, torch.float32),
    (torch.float32, torch.float64, torch.float64),
    (torch.float16, torch.float32, torch.float32),
    (torch.int32, torch.float32, torch.float32),
    (torch.int64, torch.int64, torch.float64),
    (torch.float16, torch.float16, torch.float64),
])
def test_common_float(a, b, want):
  x = torch.ones((2, 3, 4), dtype=a)
  y = torch.ones((2, 3, 4), dtype=b)
  (cx, cy), dtype = gm._common_float(_geo(), [x, y])
  assert dtype == want and cx.dtype == want and cy.dtype == want
  # only what differs is cast: an operand of the common dtype comes back as
  # the same object, no copy
  assert (cx is x) == (a == want) and (cy is y) == (b == want)
  assert torch.equal(cx, x.to(want)) and torch.equal(cy, y.to(want))


def test_common_float_checks_the_grid():
  x = torch.ones((2, 3, 4))
  with pytest.raises(ValueError) as e:
    gm._common_float(_geo(), [x, torch.ones((2, 4, 3))])
  assert str(e.value) == ('spatial shape (4, 3) does not match the '
                          'coordinates (3, 4)')
  gm._common_float(_geo(layout=plan_lib.LONLAT), [torch.ones((2, 4, 3))])


def test_geometry_declares_its_fields():
  geo = _geo()
  assert geo.region_wsum is None
  assert geo.spatial_dims == ('latitude', 'longitude')
  assert _geo(layout=plan_lib.LONLAT).spatial_dims == ('longitude', 'latitude')
  assert gm._spatial_dims(plan_lib.LATLON) == gm._SPATIAL


# --- the ensemble outer layout against brute force ----------------------------
N_LAT, N_LON = 3, 4
SIZES = {'realization': 3, 'time': 2, 'level': 4, 'lead_time': 5, 'extra': 2}


def _var(dims, sizes=SIZES):
  dims = tuple(dims) + ('latitude', 'longitude')
  shape = tuple(sizes[d] for d in dims[:-2]) + (N_LAT, N_LON)
  return xl.DataArray(np.zeros(shape, np.float32), dims)


def _forecast(fvar):
  coords = {'latitude': np.linspace(-60, 60, N_LAT),
            'longitude': np.arange(N_LON) * 10.0}
  return xl.Dataset({'z': fvar}, coords)


def _brute_force(fdims, other_dims, sizes):
  out_dims = [d for d in fdims if d != 'realization']
  for dims in other_dims:
    out_dims += [d for d in dims if d not in out_dims]
  out_shape = tuple(sizes[d] for d in out_dims)
  strides = {}
  for i, d in enumerate(fdims):
    strides[d] = int(np.prod([sizes[e] for e in fdims[i + 1:]], dtype=np.int64))
  table = [sum(idx[out_dims.index(d)] * strides[d] for d in fdims
               if d != 'realization') for idx in np.ndindex(*out_shape)]
  return tuple(out_dims), out_shape, strides, np.array(table, dtype=np.int64)


@pytest.mark.parametrize('fdims,others', [
    (('realization', 'time', 'level'), [('time', 'level')]),      # first
    (('time', 'realization', 'level'), [('time', 'level')]),      # middle
    (('time', 'level', 'realization'), [('time', 'level')]),      # last
    (('time', 'realization', 'level'), [('level', 'time')]),      # reordered
    (('time', 'realization'), [('time', 'extra')]),    # truth brings a dim
    (('time', 'realization', 'level'), [('time',)]),   # truth lacks a dim
    (('time', 'realization', 'level'), [('time', 'level'), ('level',)]),
    (('time', 'realization', 'level'), [('time', 'level'), ()]),
    (('lead_time', 'realization', 'time'), [('time',), ('extra', 'time')]),
    (('realization',), [()]),           # only the ensemble and spatial dims
    (('realization',), [('time',)]),
])
@pytest.mark.parametrize('n_member', [3, 1])
def test_ens_outer_layout_matches_brute_force(fdims, others, n_member):
  sizes = dict(SIZES, realization=n_member)
  fvar = _var(fdims, sizes)
  outer = gm._ens_outer_layout(_forecast(fvar), fvar,
                               [_var(d, sizes) for d in others], 'realization')
  out_dims, out_shape, strides, table = _brute_force(fdims, others, sizes)
  assert outer.geo.out_dims == out_dims and outer.geo.out_shape == out_shape
  assert outer.n_member == n_member
  assert outer.strides == strides
  got = outer.ens_table()
  assert got.dtype == np.int64 and got.flags.c_contiguous
  np.testing.assert_array_equal(got, table)
  assert [rest for _, rest in outer.prepared] == [fdims] + list(others)
  assert outer.geo.layout == plan_lib.LATLON
  # a strided view brings its own strides
  doubled = {d: 2 * s for d, s in strides.items()}
  np.testing.assert_array_equal(outer.ens_table(doubled), 2 * table)


def test_ens_outer_layout_errors():
  fvar = _var(('time', 'level'))
  with pytest.raises(ValueError) as e:
    gm._ens_outer_layout(_forecast(fvar), fvar, [_var(('time',))],
                         'realization')
  ensemble_dim = 'realization'
  assert str(e.value) == f'{ensemble_dim=} not found in {fvar.dims=}'
  fvar = _var(('time', 'realization'))
  with pytest.raises(ValueError) as e:
    gm._ens_outer_layout(_forecast(fvar), fvar,
                         [_var(('realization', 'time'))], 'realization')
  assert str(e.value) == "truth must not have the ensemble dim 'realization'"


# --- region dispatch ----------------------------------------------------------
def _chunk_result(forecast, value, lead=()):
  forecast = xl.as_dataset(forecast)
  out = xl.Dataset(coords={'time': forecast.coords['time']})
  if lead:
    out.coords['region'] = np.array(lead, dtype=object)
  n_time = forecast.sizes['time']
  data = np.full((len(lead),) * bool(lead) + (n_time,), float(value))
  dims = (('region',) if lead else ()) + ('time',)
  out.data_vars['z'] = xl.DataArray(data, dims, out.coords, 'z')
  return out


def _pair():
  dims = ('time', 'realization', 'latitude', 'longitude')
  shape = (2, 3, N_LAT, N_LON)
  coords = {'time': np.arange(2), 'realization': np.arange(3),
            'latitude': np.linspace(-60, 60, N_LAT),
            'longitude': np.arange(N_LON) * 10.0}
  forecast = xl.Dataset({'z': xl.DataArray(np.zeros(shape, np.float32), dims)},
                        coords)
  truth = xl.Dataset({'z': xl.DataArray(
      np.zeros((2, N_LAT, N_LON), np.float32), dims[:1] + dims[2:])},
                     {k: v for k, v in coords.items() if k != 'realization'})
  return forecast, truth


REGIONS = {'a': 'region-a', 'b': 'region-b', 'c': None}


def test_a_plain_subclass_is_called_once_per_region():
  calls = []

  class Fake(gm.Metric):
    def compute_chunk(self, forecast, truth, region=None, skipna=False):
      calls.append(region)
      return _chunk_result(forecast, len(calls))
  forecast, truth = _pair()
  out = Fake().compute_chunk_regions(forecast, truth, REGIONS)
  assert calls == list(REGIONS.values())
  assert out['z'].dims == ('region', 'time')
  assert list(out.coords['region']) == list(REGIONS)
  np.testing.assert_array_equal(out['z'].values, [[1, 1], [2, 2], [3, 3]])
  calls.clear()
  out = Fake().compute_regions(forecast, truth, REGIONS)
  assert calls == list(REGIONS.values()) and out['z'].dims == ('region',)
  np.testing.assert_array_equal(out['z'].values, [1, 2, 3])
  assert 'ensemble_size' not in out.attrs


def test_an_ensemble_subclass_without_the_declaration_fans_out():
  calls = []

  class Fake(gm.EnsembleMetric):          # no `regions` keyword at all
    def compute_chunk(self, forecast, truth, region=None, skipna=False):
      calls.append(region)
      return _chunk_result(forecast, len(calls))
  assert Fake._fused_regions is False and Fake._reads_slabs_in_place is False
  forecast, truth = _pair()
  out = Fake().compute_chunk_regions(forecast, truth, REGIONS)
  assert calls == list(REGIONS.values())
  np.testing.assert_array_equal(out['z'].values, [[1, 1], [2, 2], [3, 3]])
  assert Fake().compute(forecast, truth).attrs['ensemble_size'] == 3
  assert Fake().compute_regions(forecast, truth,
                                REGIONS).attrs['ensemble_size'] == 3

  class OnlyCompute(gm.CRPS):             # its own `compute`: fan-out too
    def compute(self, forecast, truth, region=None, skipna=False):
      calls.append(('compute', region))
      return _chunk_result(forecast, 7).mean('time')
  assert OnlyCompute._fused_regions is False
  calls.clear()
  out = OnlyCompute().compute_regions(forecast, truth, REGIONS)
  assert calls == [('compute', r) for r in REGIONS.values()]
  np.testing.assert_array_equal(out['z'].values, [7, 7, 7])


def test_a_declared_subclass_is_called_once_with_regions():
  calls = []

  class Fused(gm.EnsembleMetric):
    _fused_regions = True

    def compute_chunk(self, forecast, truth, region=None, skipna=False,
                      regions=None):
      calls.append((region, regions))
      return _chunk_result(forecast, 5, tuple(regions or ()))
  forecast, truth = _pair()
  out = Fused().compute_chunk_regions(forecast, truth, REGIONS)
  assert calls == [(None, REGIONS)] and calls[0][1] is REGIONS
  assert out['z'].dims == ('region', 'time')
  calls.clear()
  out = Fused().compute_regions(forecast, truth, REGIONS, skipna=True)
  assert calls == [(None, REGIONS)]
  assert out['z'].dims == ('region',) and out.attrs['ensemble_size'] == 3
  assert Fused().compute(forecast, truth).attrs['ensemble_size'] == 3
  # what inherits the class's compute_chunk inherits its declaration
  assert type('Sub', (Fused,), {})._fused_regions is True


def test_neither_time_dim_raises_before_any_chunk_work():
  class Fake(gm.Metric):
    _fused_regions = True

    def compute_chunk(self, forecast, truth, region=None, skipna=False,
                      regions=None):
      raise AssertionError('not reached')
  ds = _ds(('level',))
  for call in (lambda: Fake().compute(ds, ds),
               lambda: Fake().compute_regions(ds, ds, REGIONS)):
    with pytest.raises(ValueError, match='neither valid_time or init_time'):
      call()


# the value each public class has at the parent of the commit that introduced
# the declarations (there: class attributes, and a property comparing function
# identities on EnsembleMetric)
READS_SLABS_IN_PLACE = {
    True: ['MSE', 'RMSESqrtBeforeTimeAvg', 'MAE', 'Bias', 'WindVectorMSE',
           'WindVectorRMSESqrtBeforeTimeAvg', 'ACC', 'SEEPS', 'CRPS',
           'CRPSSpread', 'CRPSSkill', 'EnsembleStddevSqrtBeforeTimeAvg',
           'EnsembleVariance', 'EnsembleMeanRMSESqrtBeforeTimeAvg',
           'EnsembleMeanMSE', 'DebiasedEnsembleMeanMSE'],
    False: ['EnergyScore', 'EnergyScoreSpread', 'EnergyScoreSkill',
            'GaussianCRPS', 'GaussianVariance', 'GaussianBrierScore',
            'GaussianIgnoranceScore', 'GaussianRPS', 'EnsembleBrierScore',
            'DebiasedEnsembleBrierScore', 'EnsembleIgnoranceScore',
            'EnsembleRPS', 'SpatialMSE', 'SpatialMAE', 'SpatialBias',
            'SpatialCRPS', 'SpatialCRPSSpread', 'SpatialCRPSSkill',
            'SpatialEnsembleVariance', 'SpatialEnsembleMeanMSE',
            'DebiasedSpatialEnsembleMeanMSE', 'SpatialEnsembleBrierScore',
            'SpatialDebiasedEnsembleBrierScore',
            'SpatialEnsembleIgnoranceScore', 'SpatialEnsembleRPS',
            'SpatialSEEPS', 'RankHistogram'],
}
FUSED_REGIONS = READS_SLABS_IN_PLACE[True] + [
    'EnergyScore', 'EnergyScoreSpread', 'EnergyScoreSkill']


def test_reads_slabs_in_place_and_fused_regions_per_class():
  listed = READS_SLABS_IN_PLACE[True] + READS_SLABS_IN_PLACE[False]
  public = [n for n, c in vars(gm).items()
            if isinstance(c, type) and issubclass(c, gm.Metric)
            and not n.startswith('_')
            and n not in ('Metric', 'EnsembleMetric', 'ThresholdMetric')]
  assert sorted(public) == sorted(listed)
  for want, names in READS_SLABS_IN_PLACE.items():
    for name in names:
      cls = getattr(gm, name)
      assert getattr(cls, '_reads_slabs_in_place', False) is want, name
      assert cls._fused_regions is (name in FUSED_REGIONS), name
  wind = gm.WindVectorMSE('u', 'v', 'wind')
  assert wind._reads_slabs_in_place is True      # (read on an instance too)
  assert gm.CRPS()._reads_slabs_in_place is True
  assert gm.RankHistogram()._reads_slabs_in_place is False
