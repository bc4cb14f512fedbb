"""CPU checks of the derived variables: the committed fixtures against the
reference (where it is at hand), the test-side NumPy restatement against the
fixtures, the np.gradient coefficient tables, and the module's structure
against the reference's names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import derived_cases as dc
from tests import derived_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, 'weatherbench2'))


@pytest.fixture(scope='module')
def golden():
  out = dc.load_golden(GOLDEN_DIR)
  assert out, 'no reference_derived_v1.*.npz shard found'
  return out


def test_no_shard_exceeds_the_size_limit():
  paths = dc.golden_paths(GOLDEN_DIR)
  assert len(paths) == 6
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path


@pytest.mark.skipif(not HAVE_REFERENCE,
                    reason='the reference checkout is only present in the '
                           'build container')
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
  env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1',
             WB2_DERIVED_OUT=str(tmp_path))
  done = subprocess.run(
      [sys.executable, os.path.join(GOLDEN_DIR, 'make_derived_vectors.py')],
      env=env, capture_output=True, text=True)
  assert done.returncode == 0, done.stderr[-2000:]
  fresh = dc.load_golden(str(tmp_path))
  assert sorted(fresh) == sorted(golden)
  for key, want in golden.items():
    got = fresh[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    np.testing.assert_array_equal(got, want, err_msg=key)


def test_structure_equals_the_reference(golden):
  """Class names, dataclass fields and defaults, base_variables, core_dims
  and the dictionary keys (minus the keys DESIGN.md section 7 leaves out),
  against the record the generator took from the reference's module."""
  from weatherbench2_amd import derived_variables as dv
  ref = json.loads(str(golden['known/structure']))
  mine = dc.structure(dv)
  assert mine['labels'] == ref['labels']
  assert all(v['in_dict'] for v in mine['labels'].values())
  assert tuple(ref['keys']) == tuple(
      k for k in ref['keys'] if k in dc.REFERENCE_KEYS)
  assert [k for k in ref['keys'] if k not in dc.LEFT_OUT_KEYS] == \
      [k for k in mine['keys']]
  assert set(dc.LEFT_OUT_KEYS) <= set(ref['keys'])
  # the committed list of names says the same
  for label, (name, _) in dc.CLASSES.items():
    assert ref['labels'][label]['fields'] == dc.REFERENCE_FIELDS[name]
  for label, obj in dv.DERIVED_VARIABLE_DICT.items():
    name, fields = dc.fields_of(label)
    assert type(obj).__name__ == name
    assert {k: getattr(obj, k) for k in fields} == fields


def _check(got, want, key):
  assert got.dtype == want.dtype and got.shape == want.shape, key
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=key)
  inf = np.isinf(want)
  np.testing.assert_array_equal(np.isinf(got), inf, err_msg=key)
  np.testing.assert_array_equal(np.sign(got[inf]), np.sign(want[inf]),
                                err_msg=key)
  ok = np.isfinite(want)
  rms = np.sqrt(np.mean(want[ok].astype(np.float64) ** 2))
  err = np.abs(got[ok].astype(np.float64) - want[ok]).max()
  assert err <= 1e-12 * rms, (key, err / rms)


@pytest.mark.parametrize('cname', list(dc.cases()))
def test_numpy_restatement_reproduces_the_reference(golden, cname):
  case = dc.cases()[cname]()
  assert int(golden[f'{cname}/seed']) == case['seed']
  assert tuple(golden[f'{cname}/shape']) == \
      case['vars']['u_component_of_wind'][1].shape
  for label in dc.CLASSES:
    name, fields = dc.fields_of(label)
    key = f'{cname}/{label}'
    if case['dtype'] == 'float32':
      dims, got = derived_np.compute(name, fields, case['vars'],
                                     case['coords'])
      assert list(dims) == list(golden[f'{key}/dims'])
      _check(got, golden[f'{key}/ref32'], key + '/ref32')
      dims, got = derived_np.compute(name, fields, dc.as_float64(case)['vars'],
                                     case['coords'])
    else:
      assert f'{key}/ref32' not in golden
      dims, got = derived_np.compute(name, fields, case['vars'],
                                     case['coords'])
    assert list(dims) == list(golden[f'{key}/dims'])
    _check(got, golden[f'{key}/ref64'], key + '/ref64')


def test_result_dtypes_of_the_reference(golden):
  """float32 inputs: float32 for WindSpeed, float64 wherever a float64
  coordinate enters the expression."""
  for cname, build in dc.cases().items():
    if build()['dtype'] != 'float32':
      continue
    for label in dc.CLASSES:
      want = np.float32 if 'wind_speed' in label and 'geo' not in label \
          else np.float64
      assert golden[f'{cname}/{label}/ref32'].dtype == want, (cname, label)
      assert golden[f'{cname}/{label}/ref64'].dtype == np.float64


def test_non_finite_counts_of_the_reference(golden):
  """On the pole-and-equator grid the reference is non-finite on exactly one
  latitude row of 19 (360 of 6 840 points) for the six geostrophic and
  ageostrophic classes and nowhere for the others; on the grid without poles
  and equator nowhere at all."""
  for label in dc.CLASSES:
    for which in ('ref32', 'ref64'):
      a = golden[f'lonlat_poles/{label}/{which}']
      bad = ~np.isfinite(a)
      if label in dc.GEOSTROPHIC:
        assert a.size == 6840 and bad.sum() == 360, label
        assert bad[..., 9].all() and not np.delete(bad, 9, axis=-1).any()
      else:
        assert not bad.any(), label
      assert np.isfinite(golden[f'latlon_linspace/{label}/{which}']).all()
  assert len(dc.GEOSTROPHIC) == 6


def test_known_answers_of_the_reference(golden):
  for label, known in dc.KNOWN_ANSWERS.items():
    name, fields = dc.fields_of(label)
    np.testing.assert_array_equal(golden[f'known/{label}/expected'],
                                  known['expected'])
    np.testing.assert_allclose(golden[f'known/{label}/ref'], known['expected'],
                               atol=known['atol'], rtol=0)
    _, got = derived_np.compute(name, fields, known['vars'], known['coords'])
    np.testing.assert_allclose(got, golden[f'known/{label}/ref'], rtol=1e-12)


@pytest.mark.parametrize('coord', [
    np.linspace(-90, 90, 19), np.linspace(-88, 88, 24),
    np.linspace(-90, 90, 721), np.linspace(-87.1875, 87.1875, 32),
    np.arange(1440) * 0.25, np.array([300., 500, 700, 850, 1000]),
    np.array([0., 1.0]), np.array([0, 10, 20, 30])],
    ids=lambda c: f'n{len(c)}')
def test_gradient_tables_equal_np_gradient(coord):
  from weatherbench2_amd import plan
  table, uniform = plan.gradient_tables(coord)
  d = np.diff(np.asarray(coord, dtype=np.float64))
  assert uniform == bool((d == d[0]).all())
  assert table.shape == (4, len(coord)) and table.dtype == np.float64
  rs = np.random.RandomState(len(coord))
  f = rs.standard_normal((len(coord), 7))
  want = np.gradient(f, coord, axis=0, edge_order=1)
  got = derived_np.apply_gradient_table(f, table, uniform, axis=0)
  scale = np.sqrt(np.mean(want ** 2))
  assert np.abs(got - want).max() <= 1e-12 * scale


def test_a_linspace_axis_can_be_non_uniform():
  from weatherbench2_amd import plan
  assert plan.gradient_tables(np.linspace(-90, 90, 19))[1]
  assert not plan.gradient_tables(np.linspace(-88, 88, 24))[1]
  for cname in ('latlon_linspace', 'latlon_f64'):
    lat = dc.cases()[cname]()['coords']['latitude']
    assert not plan.gradient_tables(lat)[1] and (lat != 0).all()
    assert (np.cos(np.deg2rad(lat)) > 1e-6).all()


def test_gradient_tables_need_two_points():
  from weatherbench2_amd import plan
  with pytest.raises(ValueError):
    plan.gradient_tables(np.array([1.0]))


def test_latitude_tables_are_numpy_expressions():
  from weatherbench2_amd import plan
  lat = np.linspace(-90, 90, 19)
  tab = plan.latitude_tables(lat)
  np.testing.assert_array_equal(tab[0], np.cos(np.deg2rad(lat)))
  np.testing.assert_array_equal(tab[1],
                                2 * 7.292e-5 * np.sin(np.deg2rad(lat)))
  assert tab[1][9] == 0.0 and (tab[0][[0, -1]] <= 1e-6).all()
  assert plan.METERS_PER_DEGREE == derived_np.METERS_PER_DEGREE


def test_new_entry_points_validate_their_arguments():
  import ctypes
  from weatherbench2_amd import build, _lib
  build.build(verbose=False)
  h = _lib.load()
  # empty launches are no-ops, the rest is checked before the device
  assert h.wb2_derived_pointwise(0, _lib.WB2_F32, _lib.WB2_F32, None, None,
                                 None, None, None, 0, 8, None, None) == 0
  rc = h.wb2_derived_pointwise(0, _lib.WB2_F32, _lib.WB2_F32, None, None, None,
                               None, None, 2, 8, None, None)
  assert rc < 0 and b'null pointer' in h.wb2_last_error()
  rc = h.wb2_derived_pointwise(0, _lib.WB2_F32, _lib.WB2_F64, None, None, None,
                               None, None, 2, 8, None, None)
  assert rc < 0
  rc = h.wb2_derived_pointwise(5, _lib.WB2_F32, _lib.WB2_F32, None, None, None,
                               None, None, 2, 8, None, None)
  assert rc < 0 and b'unknown mode' in h.wb2_last_error()
  assert h.wb2_derived_stencil(0, _lib.WB2_F32, 1, None, None, 0, 4, 4, None,
                               1, None, 1, None, None, 1.0, None, None) == 0
  rc = h.wb2_derived_stencil(0, _lib.WB2_F32, 1, None, None, 3, 4, 4, None, 1,
                             None, 1, None, None, 1.0, None, None)
  assert rc < 0 and b'null pointer' in h.wb2_last_error()
  rc = h.wb2_derived_stencil(9, _lib.WB2_F32, 1, None, None, 3, 4, 4, None, 1,
                             None, 1, None, None, 1.0, None, None)
  assert rc < 0 and b'unknown mode' in h.wb2_last_error()
  tile, rows = ctypes.c_int32(), ctypes.c_int32()
  assert h.wb2_derived_stencil_geometry(_lib.WB2_F32, 1, ctypes.byref(tile),
                                        ctypes.byref(rows)) == 0
  assert (tile.value, rows.value) == (256, 16)
  assert h.wb2_derived_stencil_geometry(_lib.WB2_F64, 0, ctypes.byref(tile),
                                        ctypes.byref(rows)) == 0
  assert (tile.value, rows.value) == (64, 16)
