"""CPU checks of the lead-time derived variables (the precipitation
accumulations): the committed fixtures against the reference (where it is at
hand), the test-side NumPy restatement against the fixtures, the module's
structure and dictionaries against the reference's names, the host-side
checks of the classes, and the entry point's argument checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lead_cases as lc
from tests import lead_np
from weatherbench2_amd import derived_variables as dv
from weatherbench2_amd import xarray_lite as xl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, 'weatherbench2'))
LEAD = lc.LEAD


@pytest.fixture(scope='module')
def golden():
  out = lc.load_golden(GOLDEN_DIR)
  assert out, 'no reference_lead_v1.*.npz shard found'
  return out


def unit_roundoff(dtype) -> float:
  return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def check_against_reference(got, want, mag, w, key):
  """NaN and infinity positions equal; elsewhere |got - want| <= 2 w u
  sum_window |term| per point, in float64 (the standard bound for two
  summations of the same w terms in different orders); bit-equal where
  w = 1."""
  assert got.dtype == want.dtype and got.shape == want.shape, key
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=key)
  inf = np.isinf(want)
  np.testing.assert_array_equal(np.isinf(got), inf, err_msg=key)
  np.testing.assert_array_equal(got[inf], want[inf], err_msg=key)
  if w == 1:
    np.testing.assert_array_equal(got, want, err_msg=key)
    return 0.0
  ok = np.isfinite(want)  # (a clamped -inf is a finite 0.0: its bound is inf)
  assert not np.isnan(mag[ok]).any(), key
  err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
  bound = 2 * w * unit_roundoff(want.dtype) * mag[ok]
  assert (err <= bound).all(), (key, (err / np.maximum(bound, 1e-300)).max())
  return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def test_one_shard_per_case_below_the_size_limit():
  paths = lc.golden_paths(GOLDEN_DIR)
  assert len(paths) == len(lc.cases()) + 2  # + `known`, + the structure record
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path


@pytest.mark.skipif(not HAVE_REFERENCE,
                    reason='the reference checkout is only present in the '
                           'build container')
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
  env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1',
             WB2_LEAD_OUT=str(tmp_path))
  done = subprocess.run(
      [sys.executable, os.path.join(GOLDEN_DIR, 'make_lead_vectors.py')],
      env=env, capture_output=True, text=True)
  assert done.returncode == 0, done.stderr[-2000:]
  fresh = lc.load_golden(str(tmp_path))
  assert sorted(fresh) == sorted(golden)
  for key, want in golden.items():
    got = fresh[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    np.testing.assert_array_equal(got, want, err_msg=key)
    assert got.tobytes() == want.tobytes(), key


def test_structure_equals_the_reference(golden):
  """Class names, dataclass fields in order with their defaults,
  base_variables, core_dims and the four dictionary entries, against the
  record the generator took from the reference's module."""
  ref = json.loads(str(golden['structure/structure']))
  mine = lc.structure(dv, dv.LEAD_VARIABLE_DICT)
  assert mine['labels'] == ref['labels']
  for label, record in mine['labels'].items():
    assert record['in_dict'] == (label in lc.DICT_KEYS), label
  for label, (name, _) in lc.CLASSES.items():
    assert ref['labels'][label]['fields'] == lc.REFERENCE_FIELDS[name]
    assert ref['labels'][label]['field_order'] == list(
        lc.REFERENCE_FIELDS[name])
  assert sorted({name for name, _ in lc.CLASSES.values()}) == \
      sorted(lc.CLASS_NAMES)
  assert tuple(ref['keys']) == lc.REFERENCE_KEYS
  for cls in (dv.PrecipitationAccumulation,
              dv.AggregatePrecipitationAccumulation):
    assert issubclass(cls, dv._MaterializedVariable)
  obj = dv.PrecipitationAccumulation('tp', 6, lead_time_name='lead_time')
  assert obj.base_variables == ['tp']
  assert obj.core_dims == ((['lead_time'],), ['lead_time'])
  assert obj.all_input_core_dims == {'lead_time'}
  agg = dv.AggregatePrecipitationAccumulation(24)
  assert agg.base_variables == ['total_precipitation_6hr']
  assert agg.core_dims == ((['prediction_timedelta'],),
                           ['prediction_timedelta'])


def test_the_dictionaries(golden):
  ref = json.loads(str(golden['structure/structure']))
  assert list(dv.LEAD_VARIABLE_DICT) == list(lc.DICT_KEYS)
  assert list(dv.REFERENCE_DERIVED_VARIABLES) == ref['keys']
  assert len(dv.REFERENCE_DERIVED_VARIABLES) == 22
  for key, obj in dv.REFERENCE_DERIVED_VARIABLES.items():
    homes = [d for d in (dv.DERIVED_VARIABLE_DICT, dv.COLUMN_VARIABLE_DICT,
                         dv.LEAD_VARIABLE_DICT) if key in d]
    assert len(homes) == 1 and homes[0][key] is obj, key
    assert dv.is_materialized(obj)
  # the three older dictionaries are what they were
  assert len(dv.DERIVED_VARIABLE_DICT) == 11
  assert len(dv.COLUMN_VARIABLE_DICT) == 7
  assert list(dv.ALL_DERIVED_VARIABLES) == ref['keys'][:18]
  assert not set(dv.LEAD_VARIABLE_DICT) & set(dv.ALL_DERIVED_VARIABLES)
  for key, obj in dv.ALL_DERIVED_VARIABLES.items():
    home = (dv.COLUMN_VARIABLE_DICT if key in dv.COLUMN_VARIABLE_DICT
            else dv.DERIVED_VARIABLE_DICT)
    assert home[key] is obj


def test_known_answers_are_bit_equal(golden):
  """The reference's three known-answer tests: integer-valued, every sum is
  exact, so the reference, its expectation and the restatement agree bit for
  bit."""
  for label, known in lc.KNOWN_ANSWERS.items():
    ref = golden[f'known/{label}/ref']
    np.testing.assert_array_equal(ref, golden[f'known/{label}/expected'])
    np.testing.assert_array_equal(ref, known['expected'])
    name, fields = lc.fields_of(label)
    dims, got = lead_np.compute(name, fields, known['vars'], known['coords'])
    assert list(dims) == list(golden[f'known/{label}/dims']) == [LEAD]
    assert got.dtype == ref.dtype == np.float64
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize('cname', list(lc.cases()))
def test_numpy_restatement_reproduces_the_reference(golden, cname):
  case = lc.cases()[cname]()
  assert int(golden[f'{cname}/seed']) == case['seed']
  assert tuple(golden[f'{cname}/shape']) == \
      case['vars']['total_precipitation'][1].shape
  windows = set()
  for label in lc.CLASSES:
    key = f'{cname}/{label}'
    assert (f'{key}/ref' in golden) == (label in case['labels'])
    if label not in case['labels']:
      continue
    name, fields = lc.fields_of(label)
    dims, got, mag, w = lead_np.compute(name, fields, case['vars'],
                                        case['coords'], with_abs=True)
    want = golden[f'{key}/ref']
    assert list(dims) == list(golden[f'{key}/dims'])
    assert list(dims) == list(case['vars'][lc.input_name(label)][0])
    assert list(golden[f'{key}/coords']) == sorted(case['coords'])
    # float32 stays float32, float64 float64, integers become float64
    assert want.dtype == (np.float32 if case['dtype'] == 'float32'
                          else np.float64), key
    check_against_reference(got, want, mag, w, key)
    windows.add(w)
  hourly = cname.startswith('hourly')
  assert windows == ({6, 24} if hourly else {1, 2, 4})


def test_what_the_cases_cover(golden):
  """The clamp acts (zeros where the unclamped twin is negative, nothing
  negative left), NaN at single leads widens to the windows that see it, and
  infinities travel."""
  for cname, build in lc.cases().items():
    labels = build()['labels']
    for clamped, free in (('total_precipitation_6hr', 'tp6_unclamped'),
                          ('total_precipitation_24hr', 'tp24_unclamped')):
      a, b = golden[f'{cname}/{clamped}/ref'], golden[f'{cname}/{free}/ref']
      negative = b < 0
      assert negative.sum() > 10, (cname, free)
      assert (a[negative] == 0).all() and not (a < 0).any()
      same = ~negative
      np.testing.assert_array_equal(a[same], b[same])
    if 'nan' in cname:
      assert 'total_precipitation_24hr_from_6hr' in labels
  a = golden['lonlat_member_nan/total_precipitation_24hr_from_6hr/ref']
  lead_axis = 1
  complete = np.moveaxis(a, lead_axis, 0)[3:]
  assert 0 < np.isnan(complete).sum() <= 4 * 12
  assert np.isinf(golden['latlon_inf_f64/tp6_unclamped/ref']).sum() > 0
  assert golden['lead_last_int/total_precipitation_6hr/ref'].dtype == \
      np.float64


def _dataset(n_lead=7, name='total_precipitation', lead=None):
  if lead is None:
    lead = np.arange(n_lead) * np.timedelta64(6, 'h')
  data = np.zeros((len(lead), 3), dtype=np.float32)
  return xl.Dataset(
      {name: xl.DataArray(data, (LEAD, 'cell'))},
      {LEAD: lead.astype('timedelta64[ns]'), 'cell': np.arange(3)})


def test_host_side_checks_raise_before_any_device_work():
  """As in the reference: unequal steps and a window that is no whole number
  of steps are AssertionErrors with its messages.  Fewer than two leads: a
  ValueError that names the lead dimension (the reference dies with an
  IndexError there)."""
  tp24 = dv.LEAD_VARIABLE_DICT['total_precipitation_24hr']
  lead = np.arange(7) * np.timedelta64(6, 'h')
  lead[3] += np.timedelta64(1, 'h')
  with pytest.raises(AssertionError, match='All time steps must be equal.'):
    tp24.compute(_dataset(lead=lead))
  with pytest.raises(AssertionError,
                     match='Accumulation time must be multiple of timestep.'):
    dv.PrecipitationAccumulation('total_precipitation', 9).compute(_dataset())
  with pytest.raises(AssertionError,
                     match='Accumulation time must be multiple of timestep.'):
    dv.PrecipitationAccumulation('total_precipitation', 3).compute(_dataset())
  for n_lead in (1, 0):
    with pytest.raises(ValueError) as info:
      tp24.compute(_dataset(n_lead=n_lead))
    assert LEAD in str(info.value)
    assert 'whole lead axis in one chunk' in str(info.value)
  # the aggregate looks at the ratio of its two hour fields alone
  with pytest.raises(AssertionError,
                     match='Accumulation time must be multiple of timestep.'):
    dv.AggregatePrecipitationAccumulation(
        accumulation_hours=24, raw_accumulation_hours=9).compute(
            _dataset(name='total_precipitation_6hr'))
  # a field without the lead dim
  ds = xl.Dataset({'total_precipitation_6hr': xl.DataArray(
      np.zeros((3,), np.float32), ('cell',))}, {'cell': np.arange(3)})
  with pytest.raises(ValueError, match=LEAD):
    dv.AggregatePrecipitationAccumulation(24).compute(ds)


def test_restatement_window_rules():
  """NaN for an incomplete window, for exactly the windows that hold a NaN,
  recovery afterwards; w >= the lead count; the clamp keeps NaN and -0.0."""
  x = np.arange(10, dtype=np.float64) ** 2
  x[4] = np.nan
  got = lead_np.rolling_sum(x, 0, 3)
  assert np.isnan(got[:2]).all() and np.isnan(got[4:7]).all()
  assert got[2] == 5 and got[3] == 14 and got[7] == 25 + 36 + 49
  acc = lead_np.precipitation_accumulation(x, 0, 2)
  assert np.isnan(acc[:2]).all() and np.isnan(acc[4:7]).all()
  assert np.isfinite(acc[[2, 3, 7, 8, 9]]).all()
  assert np.isnan(lead_np.rolling_sum(x[:3], 0, 4)).all()
  assert np.isnan(lead_np.precipitation_accumulation(x[:3], 0, 3)).all()
  only = lead_np.rolling_sum(x[:3], 0, 3)
  assert np.isnan(only[:2]).all() and only[2] == 5
  y = np.array([0.0, 1.0, 0.5, 0.5, np.nan, 0.5])
  acc = lead_np.precipitation_accumulation(y, 0, 1)
  assert np.isnan(acc[0]) and acc[1] == 1 and acc[2] == 0
  assert acc[3] == 0 and np.isnan(acc[4:]).all()
  z = np.array([0.0, -0.0, -0.0])
  acc = lead_np.precipitation_accumulation(z, 0, 1)
  assert acc[1] == 0 and np.signbit(acc[1])
  free = lead_np.precipitation_accumulation(y, 0, 1, clamp=False)
  assert free[2] == -0.5
  assert lead_np.rolling_sum(np.arange(5, dtype=np.int32), 0, 2).dtype == \
      np.float64


def test_entry_points_validate_their_arguments():
  import ctypes
  from weatherbench2_amd import build, _lib
  build.build(verbose=False)
  h = _lib.load()
  f32, f64 = _lib.WB2_F32, _lib.WB2_F64

  def call(mode, dtype, n_outer, n_lead, n_point, window, src=None, out=None):
    return h.wb2_derived_lead_window(mode, dtype, src, None, n_outer, n_lead,
                                     n_point, window, 1, out, None)

  # empty launches are no-ops whatever the pointers are
  assert call(0, f32, 0, 13, 8, 4) == 0
  assert call(1, f64, 2, 0, 8, 4) == 0
  assert call(1, f64, 2, 13, 0, 4) == 0
  rc = call(0, f32, 2, 13, 8, 4)
  assert rc < 0 and b'null pointer' in h.wb2_last_error()
  for mode in (2, -1):
    rc = call(mode, f32, 2, 13, 8, 4)
    assert rc < 0 and b'unknown mode' in h.wb2_last_error()
  rc = call(0, 7, 2, 13, 8, 4)
  assert rc < 0 and b'unknown dtype' in h.wb2_last_error()
  rc = call(0, f32, -1, 13, 8, 4)
  assert rc < 0 and b'negative' in h.wb2_last_error()
  for window in (0, -3):
    rc = call(0, f32, 2, 13, 8, window)
    assert rc < 0 and b'bad sizes' in h.wb2_last_error()
  # the geometry query
  tile, ahead, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
  windows = ctypes.POINTER(ctypes.c_int32)()
  args = (ctypes.byref(tile), ctypes.byref(ahead), ctypes.byref(windows),
          ctypes.byref(n))
  assert h.wb2_derived_lead_geometry(f32, 1, *args) == 0
  assert tile.value == 1024 and ahead.value >= 1
  have = [windows[k] for k in range(n.value)]
  assert have == sorted(set(have)) and set(have) >= {1, 2, 4, 6, 8, 24}
  assert h.wb2_derived_lead_geometry(f64, 1, *args) == 0
  assert tile.value == 512
  assert h.wb2_derived_lead_geometry(f64, 0, *args) == 0
  assert tile.value == 256
  assert h.wb2_derived_lead_geometry(f32, 1, None, None, None, None) < 0
  assert b'null pointer' in h.wb2_last_error()
  rc = h.wb2_derived_lead_geometry(5, 1, *args)
  assert rc < 0 and b'unknown dtype' in h.wb2_last_error()
