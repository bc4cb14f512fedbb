"""Quantiles without a GPU: the NumPy restatement (tests/quantile_np.py)
against NumPy and against the committed reference fixtures, the host path of
`quantiles.quantile` / `compute_quantiles` against the fixtures in values,
dims, coordinates, dtypes and pass-through variables, the reference's two
errors, and the argument checks and geometry of the two K12 entry points.
Reference: scripts/compute_quantiles.py:168-183."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest

from tests import quantile_cases as qc
from tests import quantile_np as qn

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(qc.all_cases())
MODES = sorted(qc.MODES)


@pytest.fixture(scope='module')
def golden():
  return qc.load_golden(GOLDEN_DIR)


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def q_list(case) -> list:
  return [case['q']] if case['scalar'] else list(case['q'])


def restated(case, name, skipna) -> np.ndarray:
  """The restatement's result for variable `name`, shaped like xarray's."""
  _, array = case['vars'][name]
  out = qn.quantile(array, q_list(case), qc.reduced_axes(case, name), skipna)
  return out[0] if case['scalar'] else out


def to_lite(case, device=False):
  from weatherbench2_amd import xarray_lite as xl
  variables = {}
  for name, (dims, array) in case['vars'].items():
    data = array
    if device:
      import torch
      data = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    variables[name] = xl.DataArray(data, dims)
  return xl.Dataset(variables, dict(case['coords']))


def run_product(case, dataset, skipna):
  """`compute_quantiles` for a list of quantiles (what the reference's script
  runs), `quantile` for the scalar case."""
  from weatherbench2_amd import quantiles
  if case['scalar']:
    return quantiles.quantile(dataset, case['q'], case['dim'], skipna=skipna)
  return quantiles.compute_quantiles(dataset, case['q'], case['dim'],
                                     skipna=skipna,
                                     name_suffix=case['name_suffix'])


def check_against_fixture(res, case, cname, mode, golden, device=False):
  """Values (bit-equal), dims, coordinates, dtypes and pass-through variables
  of a product result against the fixture of (case, mode)."""
  from weatherbench2_amd import xarray_lite as xl
  structure = json.loads(str(golden['structure/structure']))[cname]
  assert sorted(res.data_vars) == sorted(structure['vars'])
  for name, (dims, array) in case['vars'].items():
    out_name = name + case['name_suffix']
    da = res[out_name]
    want = golden[f'{cname}/{mode}/{out_name}']
    assert list(da.dims) == structure['vars'][out_name]['dims'] == list(
        golden[f'{cname}/{mode}/{out_name}/dims'])
    if not qc.reduced_axes(case, name):  # passes through unchanged
      assert da.dtype == array.dtype or str(da.dtype) == 'torch.' + str(
          array.dtype)
      np.testing.assert_array_equal(da.values, array)
      np.testing.assert_array_equal(want, array)
      continue
    if device:
      import torch
      assert isinstance(da.data, torch.Tensor) and da.data.is_cuda
      assert da.data.dtype == torch.float64
    else:
      assert isinstance(da.data, np.ndarray)
    assert da.values.dtype.name == structure['vars'][out_name]['dtype']
    qn.assert_bit_equal(da.values, want, f'{cname}/{mode}/{out_name}')
  kept = sorted(k for k in res.coords)
  assert kept == structure['coords'] == list(golden[f'{cname}/{mode}/coords'])
  quantile = res.coords[qc.QUANTILE]
  quantile = np.asarray(quantile.values if isinstance(quantile, xl.DataArray)
                        else quantile)
  assert quantile.dtype.name == structure['quantile_dtype']
  assert quantile.ndim == structure['quantile_ndim']
  np.testing.assert_array_equal(quantile, golden[f'{cname}/{mode}/quantile'])
  for name, values in case['coords'].items():
    if name in kept:
      np.testing.assert_array_equal(np.asarray(res.coords[name]), values)
  assert res.attrs == {}


# ---------------------------------------------------------------------------
# fixtures and restatement
# ---------------------------------------------------------------------------
def test_fixture_shards_are_complete_and_small(golden):
  paths = qc.golden_paths(GOLDEN_DIR)
  assert len(paths) == len(qc.cases()) + 2  # + known + structure
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path
  structure = json.loads(str(golden['structure/structure']))
  assert sorted(structure) == CASES
  for cname, build in qc.all_cases().items():
    case = build()
    assert structure[cname] == qc.expected_structure(case), cname
    assert int(golden[f'{cname}/seed']) == case['seed']
    assert sum(a.size for _, a in case['vars'].values()) < 10000


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_restatement_is_numpy_bit_for_bit(cname, mode):
  case = qc.all_cases()[cname]()
  skipna = qc.MODES[mode]
  fn = np.nanquantile if skipna else np.quantile
  for name, (_, array) in case['vars'].items():
    axes = qc.reduced_axes(case, name)
    if not axes:
      continue
    with warnings.catch_warnings(), np.errstate(all='ignore'):
      warnings.simplefilter('ignore')
      want = fn(array, np.asarray(q_list(case), dtype=np.float64), axis=axes,
                method='linear')
    got = qn.quantile(array, q_list(case), axes, skipna)
    qn.assert_bit_equal(got, np.asarray(want), f'{cname}/{mode}/{name}')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_restatement_is_the_fixture_bit_for_bit(golden, cname, mode):
  case = qc.all_cases()[cname]()
  for name in case['vars']:
    if not qc.reduced_axes(case, name):
      continue
    want = golden[f'{cname}/{mode}/{name}{case["name_suffix"]}']
    qn.assert_bit_equal(restated(case, name, qc.MODES[mode]), want,
                        f'{cname}/{mode}/{name}')


def test_known_answer_cases_hold_the_reference_tests_expectation(golden):
  """scripts/compute_quantiles_test.py compares the script's output with
  `quantile` + `rename_vars` of its input: both are recorded and equal, and
  the suffix reaches the variable name."""
  for cname, build in qc.known_cases().items():
    case = build()
    name = 'precip' + case['name_suffix']
    for mode in MODES:
      ref = golden[f'{cname}/{mode}/{name}']
      assert ref.shape == (2, 3, 6)
      np.testing.assert_array_equal(
          ref, golden[f'{cname}/{mode}/expected/{name}'])
      assert list(golden[f'{cname}/{mode}/{name}/dims']) == [
          'quantile', 'time', 'timedelta']
  assert 'known_2_suffix/keepna/precip_quantile' in golden


def test_the_cases_cover_what_they_claim():
  """The edge cases are in the inputs (a changed seed cannot lose them)."""
  special = qc.all_cases()['specials_f32']()['vars']['field'][1]
  assert special.dtype == np.float32
  assert sorted(special[:, 0].tolist()) == [1, 2, 3, 4, np.inf]
  assert np.signbit(special[special == 0]).any()
  assert not np.signbit(special[special == 0]).all()
  tiny = np.finfo(np.float32).tiny
  assert ((np.abs(special) < tiny) & (special != 0)).any()  # denormals
  # a finite, b = +inf, t == 0 is NaN (NumPy's), its neighbours are not
  got = qn.quantile(special, [0.5, 0.75, 1.0], 0, False)[:, 0]
  assert got[0] == 3 and np.isnan(got[1]) and np.isnan(got[2])
  nan = qc.all_cases()['nan_f32']()['vars']['field'][1]
  count = (~np.isnan(nan)).sum(axis=0)
  assert count[3] == 20 and count[10] == 0 and count[11] == 1
  assert len(set(count[4:10].tolist())) == 6
  ties = qc.all_cases()['ties']()
  x, q = ties['vars']['precip'][1], ties['q']
  assert len(set(x[:, 0].tolist())) == 1
  assert ((x[:, 1:8] == 0).mean(axis=0) > 0.6).all()
  assert len(set(q)) < len(q) and q != sorted(q) and 0.0 in q and 1.0 in q
  even = qc.all_cases()['innermost_f32']()
  assert even['vars']['wind'][1].shape[-1] % 2 == 0 and 0.5 in even['q']
  lead = qc.all_cases()['leading_f32']()
  assert (0.25 * (lead['vars']['temperature'][1].shape[0] - 1)).is_integer()
  assert lead['vars']['counts'][1].dtype.kind == 'i'
  assert 'time' not in lead['vars']['orography'][0]
  assert len(qc.all_cases()['many_quantiles']()['q']) == 21


# ---------------------------------------------------------------------------
# the host path of the public interface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_host_path_matches_the_fixtures(golden, cname, mode):
  case = qc.all_cases()[cname]()
  before = {k: a.copy() for k, (_, a) in case['vars'].items()}
  res = run_product(case, to_lite(case), qc.MODES[mode])
  check_against_fixture(res, case, cname, mode, golden)
  for k, (_, a) in case['vars'].items():  # inputs are never modified
    assert a.tobytes() == before[k].tobytes()


def test_data_array_quantile_and_default_skipna(golden):
  from weatherbench2_amd import quantiles
  from weatherbench2_amd import xarray_lite as xl
  case = qc.all_cases()['nan_f32']()
  dims, array = case['vars']['field']
  da = xl.DataArray(array, dims, dict(case['coords']), 'field')
  res = quantiles.quantile(da, case['q'], 'time')  # skipna=None: skip floats
  assert res.dims == ('quantile', 'point') and res.name == 'field'
  assert sorted(res.coords) == ['point', 'quantile']
  qn.assert_bit_equal(res.values, golden['nan_f32/skipna/field'])
  one = quantiles.quantile(da, 0.5, ['time'], skipna=False)
  assert one.dims == ('point',)
  assert one.coords['quantile'].dims == ()
  assert float(one.coords['quantile'].values) == 0.5
  qn.assert_bit_equal(one.values, golden['nan_f32/keepna/field'][2])
  # every dim at once (dim=None), integers as float64
  counts = qc.all_cases()['leading_f32']()['vars']['counts']
  res = quantiles.quantile(xl.DataArray(counts[1], counts[0]), [0.5, 0.9])
  assert res.dims == ('quantile',)
  qn.assert_bit_equal(res.values,
                      qn.quantile(counts[1], [0.5, 0.9], (0, 1, 2), True))


def test_the_two_value_errors():
  from weatherbench2_amd import quantiles
  case = qc.known(0)
  ds = to_lite(case)
  for bad in ([-0.1], [0.5, 1.5]):
    with pytest.raises(ValueError, match=r'Expected all quantiles to be in '
                       r'\[0, 1\]'):
      quantiles.compute_quantiles(ds, bad, 'lat')
  with pytest.raises(ValueError):
    quantiles.compute_quantiles(ds, [0.5], 'latitude')  # no such dim
  with pytest.raises(ValueError):
    quantiles.quantile(ds, [0.5], ['lat', 'nowhere'])
  with pytest.raises(ValueError):
    quantiles.quantile(ds, 1.5, 'lat')


def test_result_feeds_the_quantile_threshold():
  """`name_suffix='_quantile'` over a sample axis gives what
  thresholds.QuantileThreshold reads."""
  from weatherbench2_amd import quantiles, thresholds
  from weatherbench2_amd import xarray_lite as xl
  climatology, truth, want = threshold_inputs()
  clim = quantiles.compute_quantiles(climatology, [0.1, 0.5, 0.9], 'sample',
                                     name_suffix='_quantile')
  assert list(clim.data_vars) == ['temperature_quantile']
  thr = thresholds.QuantileThreshold(clim, 0.9).compute(truth)
  assert thr['temperature'].dims == ('time', 'latitude', 'longitude')
  np.testing.assert_array_equal(thr['temperature'].values, want)
  assert isinstance(thr, xl.Dataset)


def threshold_inputs(device=False):
  """(samples (sample, dayofyear, latitude, longitude), a truth dataset, the
  0.9-quantile threshold at the truth's times from np.quantile)."""
  from weatherbench2_amd import xarray_lite as xl
  rs = np.random.RandomState(71)
  dims = ('sample', 'dayofyear', 'latitude', 'longitude')
  x = (rs.standard_normal((19, 6, 5, 8)) * 9 + 275).astype(np.float32)
  coords = {'dayofyear': np.arange(1, 7), 'latitude': np.linspace(-60, 60, 5),
            'longitude': np.arange(8) * 45.0}
  data = x
  if device:
    import torch
    data = torch.from_numpy(x).cuda()
  climatology = xl.Dataset({'temperature': xl.DataArray(data, dims)}, coords)
  times = (np.datetime64('2021-01-01', 'ns')
           + np.array([4, 0, 2]) * np.timedelta64(1, 'D'))
  truth = xl.Dataset(
      {'temperature': xl.DataArray(
          rs.standard_normal((3, 5, 8)).astype(np.float32),
          ('time', 'latitude', 'longitude'))},
      {'time': times, 'latitude': coords['latitude'],
       'longitude': coords['longitude']})
  want = np.quantile(x, np.array([0.9]), axis=0)[0][[4, 0, 2]]  # float64
  return climatology, truth, want


# ---------------------------------------------------------------------------
# the C ABI without a GPU
# ---------------------------------------------------------------------------
def test_entry_points_validate_their_arguments(lib):
  h = lib.load()
  buf = ctypes.create_string_buffer(256)
  ptr = ctypes.addressof(buf)
  q = (ctypes.c_double * 2)(0.5, 1.0)

  def select(dtype=lib.WB2_F32, inp=ptr, n_outer=1, n_red=4, n_inner=4, qs=q,
             n_q=2, out=ptr):
    return h.wb2_quantile_select(dtype, 0, inp, None, n_outer, n_red, n_inner,
                                 qs, n_q, out, None)

  assert select(dtype=7) < 0 and b'unknown dtype' in h.wb2_last_error()
  for null in ('inp', 'qs', 'out'):
    assert select(**{null: None}) < 0
    assert b'null pointer' in h.wb2_last_error()
  for count in ('n_outer', 'n_red', 'n_inner', 'n_q'):
    for value in (0, -1):
      assert select(**{count: value}) < 0
      assert b'bad sizes' in h.wb2_last_error()
  for bad in (-0.25, 1.5, float('nan'), float('inf')):
    assert select(qs=(ctypes.c_double * 2)(0.5, bad)) < 0
    assert b'not in [0, 1]' in h.wb2_last_error()
  vals = [ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(),
          ctypes.c_int32()]
  refs = [ctypes.byref(v) for v in vals]
  assert h.wb2_quantile_geometry(9, 0, *refs) < 0
  assert b'unknown dtype' in h.wb2_last_error()
  assert h.wb2_quantile_geometry(lib.WB2_F32, 0, None, *refs[1:]) < 0
  assert b'null pointer' in h.wb2_last_error()


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_geometry_is_sane(lib, dtype, wide):
  import torch
  from weatherbench2_amd import engine
  geo = engine.quantile_geometry(getattr(torch, dtype), wide)
  size = np.dtype(dtype).itemsize
  assert geo['tile_points'] >= 1
  assert geo['tile_points'] * size >= 64  # a row segment of a tile
  assert geo['max_resident'] >= 1464  # one year, 6-hourly
  assert geo['max_resident'] * geo['tile_points'] * size <= 160 * 1024
  assert 1 <= geo['targets_per_pass'] < 21
  assert 1 <= geo['key_bits_per_pass'] <= 4
  assert (8 * size) % geo['key_bits_per_pass'] == 0
