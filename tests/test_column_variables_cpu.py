"""CPU checks of the level-column derived variables: the committed fixtures
against the reference (where it is at hand), the test-side NumPy restatement
against the fixtures and against analytic answers, the module's structure
against the reference's names, and the entry point's argument checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import column_cases as cc
from tests import column_np
from weatherbench2_amd import derived_variables as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, 'weatherbench2'))


@pytest.fixture(scope='module')
def golden():
  out = cc.load_golden(GOLDEN_DIR)
  assert out, 'no reference_column_v1.*.npz shard found'
  return out


def test_one_shard_per_case_below_the_size_limit():
  paths = cc.golden_paths(GOLDEN_DIR)
  assert len(paths) == len(cc.cases()) + 1  # + the structure record
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path


@pytest.mark.skipif(not HAVE_REFERENCE,
                    reason='the reference checkout is only present in the '
                           'build container')
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
  env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1',
             WB2_COLUMN_OUT=str(tmp_path))
  done = subprocess.run(
      [sys.executable, os.path.join(GOLDEN_DIR, 'make_column_vectors.py')],
      env=env, capture_output=True, text=True)
  assert done.returncode == 0, done.stderr[-2000:]
  fresh = cc.load_golden(str(tmp_path))
  assert sorted(fresh) == sorted(golden)
  for key, want in golden.items():
    got = fresh[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    np.testing.assert_array_equal(got, want, err_msg=key)


def test_structure_equals_the_reference(golden):
  """Class names, dataclass fields and defaults, base_variables, core_dims --
  oddities included -- and the two dictionaries, against the record the
  generator took from the reference's module."""
  ref = json.loads(str(golden['structure/structure']))
  mine = cc.structure(dv, dv.COLUMN_VARIABLE_DICT)
  assert mine['labels'] == ref['labels']
  for label, record in mine['labels'].items():
    assert record['in_dict'] == (label in cc.DICT_KEYS), label
  assert sorted(dv.COLUMN_VARIABLE_DICT) == sorted(cc.DICT_KEYS)
  # both dictionaries, merged, in the reference's key order; the four
  # precipitation accumulations stay out
  left_out = [k for k in ref['keys'] if k not in dv.ALL_DERIVED_VARIABLES]
  assert left_out == ['total_precipitation_6hr', 'total_precipitation_24hr',
                      'total_precipitation_24hr_from_6hr',
                      'total_precipitation_24hr_from_12hr']
  assert list(dv.ALL_DERIVED_VARIABLES) == [k for k in ref['keys']
                                            if k not in left_out]
  for key, obj in dv.ALL_DERIVED_VARIABLES.items():
    home = (dv.COLUMN_VARIABLE_DICT if key in cc.DICT_KEYS
            else dv.DERIVED_VARIABLE_DICT)
    assert home[key] is obj
    assert dv.is_materialized(obj)
  assert not set(dv.COLUMN_VARIABLE_DICT) & set(dv.DERIVED_VARIABLE_DICT)
  # the committed list of names says the same
  for label, (name, _) in cc.CLASSES.items():
    assert ref['labels'][label]['fields'] == cc.REFERENCE_FIELDS[name]
  assert sorted({name for name, _ in cc.CLASSES.values()}) == \
      sorted(cc.CLASS_NAMES)
  # the reference's oddities, by name
  assert dv.IntegratedWaterTransport().core_dims == (
      (['level'], ['level']), [])
  assert len(dv.IntegratedWaterTransport().base_variables) == 3
  assert dv.EddyKineticEnergy().core_dims == (
      (['level', 'longitude'], ['level', 'longitude']), ['longitude'])


def _check(got, want, key):
  assert got.dtype == want.dtype and got.shape == want.shape, key
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=key)
  np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=key)
  ok = np.isfinite(want)
  rms = np.sqrt(np.mean(want[ok].astype(np.float64) ** 2))
  err = np.abs(got[ok].astype(np.float64) - want[ok]).max()
  assert err <= 1e-12 * rms, (key, err, rms)


@pytest.mark.parametrize('cname', list(cc.cases()))
def test_numpy_restatement_reproduces_the_reference(golden, cname):
  case = cc.cases()[cname]()
  assert int(golden[f'{cname}/seed']) == case['seed']
  assert tuple(golden[f'{cname}/shape']) == \
      case['vars']['u_component_of_wind'][1].shape
  level = golden[f'{cname}/level']
  assert level.dtype == case['coords']['level'].dtype
  np.testing.assert_array_equal(level, case['coords']['level'])
  for label in cc.CLASSES:
    name, fields = cc.fields_of(label)
    key = f'{cname}/{label}'
    if case['dtype'] == 'float32':
      dims, got = column_np.compute(name, fields, case['vars'], case['coords'])
      assert list(dims) == list(golden[f'{key}/dims'])
      _check(got, golden[f'{key}/ref32'], key + '/ref32')
      dims, got = column_np.compute(name, fields, cc.as_float64(case)['vars'],
                                    case['coords'])
    else:
      assert f'{key}/ref32' not in golden
      dims, got = column_np.compute(name, fields, case['vars'], case['coords'])
    assert list(dims) == list(golden[f'{key}/dims'])
    _check(got, golden[f'{key}/ref64'], key + '/ref64')
    # the results without `level` travel as surface variables
    assert ('level' in dims) == (label not in cc.INTEGRALS)
    assert ('level' in list(golden[f'{key}/coords'])) == ('level' in dims)


def test_result_dtypes_of_the_reference(golden):
  """NumPy's promotion: float32 fields with an int64 level coordinate give
  float64 integrals and a float32 lapse rate; with a float32 level coordinate
  the integrals are float32 too; the vertical velocity is float64 always."""
  for cname, build in cc.cases().items():
    case = build()
    if case['dtype'] != 'float32':
      continue
    f32_level = case['coords']['level'].dtype == np.float32
    assert f32_level == (cname == 'era5_levels_f32')
    for label in cc.CLASSES:
      if label == 'lapse_rate':
        want = np.float32
      elif label == 'vertical_velocity':
        want = np.float64
      else:
        want = np.float32 if f32_level else np.float64
      assert golden[f'{cname}/{label}/ref32'].dtype == want, (cname, label)
      assert golden[f'{cname}/{label}/ref64'].dtype == np.float64
  for label in cc.CLASSES:
    assert golden[f'latlon_f64/{label}/ref64'].dtype == np.float64


def test_zero_results_and_non_finite_counts_of_the_reference(golden):
  """Where the label slice selects fewer than two levels the reference gives
  exact zeros (compared as such, not skipped); the NaN patches reach 24 EKE
  points of 684 (the zonal mean skips NaN, the integral does not), 12 TCW, 36
  IVT, 44 vertical velocity and 48 lapse rate ones."""
  for cname, label in cc.ZERO:
    for which in ('ref32', 'ref64'):
      a = golden[f'{cname}/{label}/{which}']
      assert a.size == 684 and (a == 0).all() and not np.signbit(a).any()
  counts = {'eddy_kinetic_energy': 24, 'total_column_vapor': 12,
            'integrated_vapor_transport': 36, 'ivt_open': 36,
            'vertical_velocity': 44, 'lapse_rate': 48}
  for label, n in counts.items():
    for which in ('ref32', 'ref64'):
      a = golden[f'lonlat_nan/{label}/{which}']
      assert (~np.isfinite(a)).sum() == n, (label, which)
  for cname in cc.cases():
    if cname != 'lonlat_nan':
      for label in cc.CLASSES:
        assert np.isfinite(golden[f'{cname}/{label}/ref64']).all()
  # open bounds on the decreasing coordinate integrate with negative spacings
  assert (golden['decreasing/total_column_vapor/ref64'] < 0).all()
  assert (golden['era5_levels/total_column_vapor/ref64'] > 0).all()


# ---------------------------------------------------------------------------
# analytic answers of the restatement (tests/test_column_variables_gpu.py asks
# the same of the kernels)
# ---------------------------------------------------------------------------
def analytic_cases() -> dict:
  """{name: (class name, fields, variables, coords, expected dims, expected,
  relative tolerance; 0 = exact)}."""
  level = np.array(cc.ERA5_LEVELS, dtype=np.int64)
  lat = np.linspace(-80, 80, 9)
  lon = np.arange(16) * 22.5
  dims = ('level', 'latitude', 'longitude')
  shape = (len(level), len(lat), len(lon))
  coords = {'level': level, 'latitude': lat, 'longitude': lon}
  surface = dims[1:]
  out = {}
  q = np.full(shape, 4e-3)
  out['constant_q'] = (
      'TotalColumnWater', {'water_species_name': 'q'}, {'q': (dims, q)},
      coords, surface, np.full(shape[1:], 4e-3 * (1000 - 50) / 9.81), 1e-14)
  # T = T0 - gamma z with z = geopotential / g: dT/dz = -gamma everywhere,
  # whatever the (non-uniform) level spacing
  rs = np.random.RandomState(5)
  z = (7.0e4 * np.log(1050.0 / level))[:, None, None] \
      + 50.0 * rs.standard_normal(shape[1:])
  gamma = 6.5e-3
  out['linear_t'] = (
      'LapseRate', {'temperature_name': 't', 'geopotential_name': 'z'},
      {'t': (dims, 288.0 - gamma * z / 9.81), 'z': (dims, z)}, coords, dims,
      np.full(shape, -gamma), 1e-9)
  # a wind that depends on latitude and level alone has no eddies
  u = rs.standard_normal((shape[0], shape[1], 1)) * np.ones(shape)
  v = rs.standard_normal((shape[0], shape[1], 1)) * np.ones(shape)
  wind = {'u_name': 'u', 'v_name': 'v'}
  out['zonal_wind'] = (
      'EddyKineticEnergy', wind, {'u': (dims, u), 'v': (dims, v)}, coords,
      surface, np.zeros(shape[1:]), 0)
  # uniform zonal flow, no meridional flow: no divergence, omega = 0
  out['uniform_flow'] = (
      'VerticalVelocity', wind,
      {'u': (dims, np.full(shape, 7.0)), 'v': (dims, np.zeros(shape))}, coords,
      dims, np.zeros(shape), 0)
  return out


def check_analytic(name, got_dims, got):
  _, _, _, _, dims, expected, rtol = analytic_cases()[name]
  assert tuple(got_dims) == tuple(dims)
  assert got.shape == expected.shape and got.dtype == np.float64
  if rtol:
    np.testing.assert_allclose(got, expected, rtol=rtol, atol=0)
  else:
    np.testing.assert_array_equal(got, expected)


@pytest.mark.parametrize('name', list(analytic_cases()))
def test_analytic_answers_of_the_restatement(name):
  class_name, fields, variables, coords, _, _, _ = analytic_cases()[name]
  full = {**cc.REFERENCE_FIELDS[class_name], **fields}
  dims, got = column_np.compute(class_name, full, variables, coords)
  check_analytic(name, dims, got)


def test_level_range_follows_the_label_slice():
  """The host side of IntegratedWaterTransport: inclusive labels, open ends,
  pandas' reading of a decreasing index, a refusal where nothing defines the
  answer."""
  up = np.array(cc.ERA5_LEVELS)
  assert dv._level_range(up, 300, 1000) == (5, 13)  # 8 of the 13 levels
  assert dv._level_range(up, 500, 850) == (7, 11)
  assert dv._level_range(up, None, 850) == (0, 11)
  assert dv._level_range(up, 320, None) == (6, 13)
  assert dv._level_range(up, None, None) == (0, 13)
  assert dv._level_range(up, 1001, 2000) == (13, 13)
  assert dv._level_range(up.astype(np.float32), 300, 1000) == (5, 13)
  down = up[::-1]
  begin, end = dv._level_range(down, 300, 1000)
  assert begin == end
  assert dv._level_range(down, 1000, 300) == (0, 8)
  assert dv._level_range(down, None, None) == (0, 13)
  assert dv._level_range(np.array([500]), 300, 1000) == (0, 1)
  for level, lo, hi in ((up, 300, 1000), (up, 500, 850), (down, 300, 1000),
                        (down, 1000, 300), (down, None, 500),
                        (down, 500, None)):
    sel = column_np.level_slice(level, lo, hi)
    assert dv._level_range(level, lo, hi) == (sel.start, sel.stop)
  mixed = np.array([500, 300, 700, 1000, 850])
  assert dv._level_range(mixed, None, None) == (0, 5)
  with pytest.raises(ValueError, match='not monotonic'):
    dv._level_range(mixed, 300, 1000)


def test_level_range_equals_pandas_on_monotonic_indexes():
  pd = pytest.importorskip('pandas')
  up = np.array(cc.ERA5_LEVELS)
  for level in (up, up[::-1], up.astype(np.float32)):
    for lo, hi in ((300, 1000), (500, 850), (None, 850), (320, None),
                   (1000, 300), (40, 60), (1001, 2000)):
      sl = pd.Index(level).slice_indexer(lo, hi)
      n = len(range(*sl.indices(len(level))))
      begin, end = dv._level_range(level, lo, hi)
      assert end - begin == n, (level, lo, hi)
      if n:
        assert begin == sl.start


def test_entry_points_validate_their_arguments():
  import ctypes
  from weatherbench2_amd import build, _lib
  build.build(verbose=False)
  h = _lib.load()
  f32, f64 = _lib.WB2_F32, _lib.WB2_F64

  def call(mode, dtype, out_dtype, inputs, slabs, n_column, n_level, n_point,
           begin, end, spacing=None, coef=None, out=None):
    return h.wb2_derived_column(mode, dtype, out_dtype, inputs, slabs,
                                n_column, n_level, n_point, begin, end,
                                spacing, coef, 0, 1, 1, 1.0, out, None)

  # empty launches are no-ops whatever the pointers are
  assert call(0, f32, f64, None, None, 0, 13, 8, 0, 13) == 0
  assert call(0, f32, f64, None, None, 2, 13, 0, 0, 13) == 0
  rc = call(0, f32, f64, None, None, 2, 13, 8, 0, 13)
  assert rc < 0 and b'null pointer' in h.wb2_last_error()
  rc = call(5, f32, f64, None, None, 2, 13, 8, 0, 13)
  assert rc < 0 and b'unknown mode' in h.wb2_last_error()
  rc = call(-1, f32, f64, None, None, 2, 13, 8, 0, 13)
  assert rc < 0 and b'unknown mode' in h.wb2_last_error()
  rc = call(0, 7, f64, None, None, 2, 13, 8, 0, 13)
  assert rc < 0 and b'unknown dtype' in h.wb2_last_error()
  rc = call(0, f32, f64, None, None, -1, 13, 8, 0, 13)
  assert rc < 0 and b'negative' in h.wb2_last_error()
  # a level range outside the axis, a narrowing output dtype, one level for a
  # gradient: refused before the pointers are looked at or after, never run
  scratch = ctypes.create_string_buffer(256)
  addr = ctypes.addressof(scratch)
  ptrs = (ctypes.c_void_p * 4)(addr, addr, addr, addr)
  assert call(0, f32, f64, ptrs, ptrs, 1, 13, 8, 5, 14, addr, None,
              addr) < 0
  assert b'bad sizes' in h.wb2_last_error()
  assert call(0, f32, f64, ptrs, ptrs, 1, 13, 8, 6, 5, addr, None, addr) < 0
  assert b'bad sizes' in h.wb2_last_error()
  assert call(0, f64, f32, ptrs, ptrs, 1, 13, 8, 0, 13, addr, None,
              addr) < 0
  assert b'does not fit' in h.wb2_last_error()
  assert call(2, f32, f64, ptrs, ptrs, 1, 13, 8, 0, 13, None, addr,
              addr) < 0
  assert b'does not fit' in h.wb2_last_error()
  assert call(2, f32, f32, ptrs, ptrs, 1, 1, 8, 0, 1, None, addr, addr) < 0
  assert b'bad sizes' in h.wb2_last_error()
  assert call(2, f32, f32, ptrs, ptrs, 1, 13, 8, 0, 13, None, None,
              addr) < 0
  assert b'null pointer' in h.wb2_last_error()
  assert call(3, f32, f32, None, ptrs, 1, 13, 8, 0, 13, addr, None,
              addr) < 0
  assert b'does not fit' in h.wb2_last_error()
  # the zonal means and the geometry query
  assert h.wb2_derived_zonal_mean(f32, 1, None, None, 0, 4, 4, None,
                                  None) == 0
  rc = h.wb2_derived_zonal_mean(f32, 1, None, None, 3, 4, 4, None, None)
  assert rc < 0 and b'null pointer' in h.wb2_last_error()
  rc = h.wb2_derived_zonal_mean(9, 1, None, None, 3, 4, 4, None, None)
  assert rc < 0 and b'unknown dtype' in h.wb2_last_error()
  tile, ahead = ctypes.c_int32(), ctypes.c_int32()
  assert h.wb2_derived_column_geometry(f32, 1, ctypes.byref(tile),
                                       ctypes.byref(ahead)) == 0
  assert tile.value == 1024 and 1 <= ahead.value <= 13
  assert h.wb2_derived_column_geometry(f64, 1, ctypes.byref(tile),
                                       ctypes.byref(ahead)) == 0
  assert tile.value == 512
  assert h.wb2_derived_column_geometry(f64, 0, ctypes.byref(tile),
                                       ctypes.byref(ahead)) == 0
  assert tile.value == 256
  assert h.wb2_derived_column_geometry(f32, 1, None, None) < 0
  assert b'null pointer' in h.wb2_last_error()
