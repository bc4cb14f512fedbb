"""CPU checks of the regridding module: the committed fixtures against the
reference (where it is at hand), the module's structure and host helpers
against the reference's names and known answers, the dense weights and the
nearest-neighbour table against the fixtures, the test-side NumPy restatement
of K11 against the reference's results, the table rules, and the entry points'
argument checks.  None of these needs a device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import regrid_cases as rc
from tests import regrid_np
from weatherbench2_amd import regridding as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, 'weatherbench2'))
CASES = list(rc.cases())


@pytest.fixture(scope='module')
def golden():
  out = rc.load_golden(GOLDEN_DIR)
  assert out, 'no reference_regrid_v1.*.npz shard found'
  return out


@pytest.fixture(scope='module')
def built():
  """{case name: (case, source grid, target grid)} of the product."""
  out = {}
  for cname, build in rc.cases().items():
    case = build()
    out[cname] = (case, rc.make_grid(rg, case['source']),
                  rc.make_grid(rg, case['target']))
  return out


def test_the_module_imports():
  from weatherbench2_amd.regridding import (  # noqa: F401
      BilinearRegridder, ConservativeRegridder, Grid, LatitudeSpacing,
      LongitudeScheme, NearestRegridder, Regridder, latitude_values,
      longitude_values)


def test_one_shard_per_case_below_the_size_limit():
  paths = rc.golden_paths(GOLDEN_DIR)
  assert len(paths) == len(CASES) + 2  # + `known`, + the structure record
  for path in paths:
    assert os.path.getsize(path) < (1 << 20), path


@pytest.mark.skipif(not HAVE_REFERENCE,
                    reason='the reference checkout is only present in the '
                           'build container')
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
  env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1',
             WB2_REGRID_OUT=str(tmp_path))
  done = subprocess.run(
      [sys.executable, os.path.join(GOLDEN_DIR, 'make_regrid_vectors.py')],
      env=env, capture_output=True, text=True)
  assert done.returncode == 0, done.stderr[-2000:]
  fresh = rc.load_golden(str(tmp_path))
  assert sorted(fresh) == sorted(golden)
  for key, want in golden.items():
    got = fresh[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    np.testing.assert_array_equal(got, want, err_msg=key)
    assert got.tobytes() == want.tobytes(), key


def test_fixture_inputs_are_the_seeded_cases(golden, built):
  for cname, (case, _, _) in built.items():
    assert int(golden[f'{cname}/seed']) == case['seed']
    np.testing.assert_array_equal(golden[f'{cname}/field'], case['field'])
    for side in ('source', 'target'):
      np.testing.assert_array_equal(golden[f'{cname}/{side}/longitudes'],
                                    case[side]['longitudes'])
      np.testing.assert_array_equal(golden[f'{cname}/{side}/latitudes'],
                                    case[side]['latitudes'])
      assert list(golden[f'{cname}/{side}/flags']) == [
          case[side]['periodic'], case[side]['includes_poles']]
    # float32 numbers held as float64
    f = case['field']
    np.testing.assert_array_equal(f.astype(np.float32).astype(np.float64), f)


def test_structure_equals_the_reference(golden):
  ref = json.loads(str(golden['structure/structure']))
  assert rc.structure(rg) == ref
  assert ref['classes'] == ['Grid', 'Regridder'] + list(rc.CLASSES)
  assert ref['grid_fields'] == [['longitudes', True], ['latitudes', True],
                                ['periodic', True], ['includes_poles', True]]


def test_grid():
  lon, lat = np.arange(0.0, 360, 90), np.array([-45.0, 0.0, 45.0])
  grid = rg.Grid.from_degrees(lon, lat)
  assert grid.shape == (4, 3) and grid.periodic and grid.includes_poles
  same = rg.Grid(longitudes=lon.copy(), latitudes=lat.copy(), periodic=True,
                 includes_poles=True)
  assert grid == same and hash(grid) == hash(same) and len({grid, same}) == 1
  assert grid != rg.Grid(longitudes=lon, latitudes=lat, periodic=False,
                         includes_poles=True)
  with pytest.raises(TypeError):
    rg.Grid(lon, lat, True, True)  # keyword-only
  with pytest.raises(ValueError, match='not increasing'):
    rg.Grid.from_degrees(lon, lat[::-1])
  for name in ('lat', 'lon'):
    with pytest.raises(AttributeError, match='no longer supported'):
      getattr(grid, name)
  with pytest.raises(Exception):
    grid.periodic = False  # frozen
  np.testing.assert_array_equal(
      rg.latitude_values(rg.LatitudeSpacing.EQUIANGULAR_WITH_POLES, 5),
      [-90, -45, 0, 45, 90])
  np.testing.assert_allclose(
      rg.latitude_values(rg.LatitudeSpacing.EQUIANGULAR_WITHOUT_POLES, 4),
      [-67.5, -22.5, 22.5, 67.5])
  np.testing.assert_allclose(
      rg.longitude_values(rg.LongitudeScheme.START_AT_ZERO, 4),
      [0, 90, 180, 270])
  np.testing.assert_allclose(
      rg.longitude_values(rg.LongitudeScheme.CENTER_AT_ZERO, 4),
      [-135, -45, 45, 135])
  with pytest.raises(ValueError):
    rg.latitude_values(rg.LatitudeSpacing.CUSTOM, 4)


def test_reference_known_answers_of_the_host_helpers():
  """regridding_test.py:252-311: the latitude weights, the two longitude
  weight tests, the six phase triples and the 2/3-point ValueError."""
  ka = rc.LATITUDE_WEIGHTS
  got = rg._conservative_latitude_weights(
      ka['source'], ka['target'], source_includes_poles=True,
      target_includes_poles=True)
  assert got.dtype == np.float64
  np.testing.assert_almost_equal(ka['expected'], got)
  for ka in rc.LONGITUDE_WEIGHTS:
    got = rg._conservative_longitude_weights(
        ka['source'], ka['target'], source_periodic=True, target_periodic=True)
    np.testing.assert_allclose(ka['expected'], got, atol=1e-5)
  for x, y, expected in rc.ALIGN_PHASE:
    assert rg._align_phase_with(x, y, period=10) == expected
  assert rg._align_phase_with(7, 0, None) == 7
  source = np.linspace(0, 360, 12, endpoint=False)
  for n in (1, 2):
    with pytest.raises(ValueError, match='Need 3 or more target points'):
      rg._conservative_longitude_weights(
          source, np.linspace(0, 360, n, endpoint=False), True, True)
  rg._conservative_longitude_weights(
      source, np.linspace(0, 360, 3, endpoint=False), True, True)
  # not periodic: two target points are fine
  rg._conservative_longitude_weights(source, np.array([100.0, 160.0]), True,
                                     False)


@pytest.mark.parametrize('cname', CASES)
def test_dense_weights_equal_the_reference(golden, built, cname):
  _, source, target = built[cname]
  lon_w, lat_w = rg.ConservativeRegridder(source, target).weights
  for got, key in ((lon_w, 'lon_weights'), (lat_w, 'lat_weights')):
    want = golden[f'{cname}/{key}']
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)


def test_what_the_cases_cover(golden, built):
  """Each case does what it is there for."""
  wrap = regrid_np.csr(golden['wrap/lon_weights'], wrap=True)
  bands = [wrap[1][wrap[0][k]:wrap[0][k + 1]] for k in range(len(wrap[3]))]
  seam = [k for k, band in enumerate(bands) if band[0] > band[-1]]
  assert seam == [9], 'CENTER_AT_ZERO: the cell of -9 degrees ends at the seam'
  assert bands[9].tolist() == [46, 47, 0]
  plain = regrid_np.csr(golden['global/lon_weights'], wrap=True)
  first = plain[1][plain[0][0]:plain[0][1]]
  assert first[0] > first[-1]  # START_AT_ZERO: cell 0 reaches back over 360
  lat = regrid_np.csr(golden['custom_lat/lat_weights'])
  assert len(set(np.diff(lat[0]).tolist())) > 1, 'band lengths differ'
  for key in ('lon_weights', 'lat_weights'):
    w = golden[f'uncovered/{key}']
    rows = np.isnan(w).any(axis=1)
    assert 0 < rows.sum() < len(rows)
  up = regrid_np.csr(golden['upsample/lat_weights'])
  assert set(np.diff(up[0]).tolist()) <= {1, 2}
  for key in ('lon_weights', 'lat_weights'):
    np.testing.assert_allclose(golden[f'identity/{key}'], np.eye(
        golden[f'identity/{key}'].shape[0]), atol=1e-12)
  f = golden['nan_patches/field']
  ref = golden['nan_patches/conservative/ref']
  assert np.isnan(f).sum() > 50 and np.isnan(ref[3, 7])
  # the cell (3, 7) is NaN by 0 / 0 alone: its neighbours hold numbers
  assert np.isfinite(ref[2, 7]) and np.isfinite(ref[4, 7])
  assert np.isfinite(ref[3, 6]) and np.isfinite(ref[3, 8])
  assert golden['batch/field'].shape == (3, 2, 48, 25)
  for cname in CASES:  # no infinity anywhere
    assert not np.isinf(golden[f'{cname}/field']).any()


@pytest.mark.parametrize('cname', CASES)
def test_tables_round_trip_and_agree(golden, built, cname):
  """CSR -> dense gives the matrix back; the product's tables are the
  restatement's; bilinear tables hold two taps per target index."""
  _, source, target = built[cname]
  cons = rg.ConservativeRegridder(source, target)
  for dense_w, wrap, mine, n_src in (
      (cons.weights[0], bool(source.periodic), cons.axis_tables[0],
       source.shape[0]),
      (cons.weights[1], False, cons.axis_tables[1], source.shape[1])):
    table = regrid_np.csr(dense_w, wrap)
    np.testing.assert_array_equal(regrid_np.dense(table, n_src), dense_w)
    for got, want in zip((mine.ptr, mine.idx, mine.w, mine.nan), table):
      np.testing.assert_array_equal(got, want)
    assert mine.idx.dtype == np.int32 and mine.w.dtype == np.float64
    assert mine.nan.dtype == np.uint8 and mine.ptr.dtype == np.int32
    # ascending position within the band: at most one descent, at the seam
    for k in range(len(table[3])):
      band = table[1][table[0][k]:table[0][k + 1]]
      assert (np.diff(band) < 0).sum() <= (1 if wrap else 0)
  bil = rg.BilinearRegridder(source, target)
  for mine, table in zip(bil.axis_tables, regrid_np.tables(bil)):
    for got, want in zip((mine.ptr, mine.idx, mine.w, mine.nan), table):
      np.testing.assert_array_equal(got, want)
    assert (np.diff(mine.ptr) == 2).all()
    assert ((mine.w >= 0) & (mine.w < 1)).all()


@pytest.mark.parametrize('cname', CASES)
def test_numpy_restatement_is_within_the_bound_of_the_reference(golden, built,
                                                                cname):
  """`regrid_np` (the header's order) on the reference's own dense weights and
  on the product's tables against the reference's results, float64 and
  float32, within regrid_np.reference_bound; nearest: the gather by the
  reference's table is the reference, bit for bit."""
  case, source, target = built[cname]
  field = case['field']
  ref = golden[f'{cname}/conservative/ref']
  theirs = (regrid_np.csr(golden[f'{cname}/lon_weights'],
                          bool(source.periodic)),
            regrid_np.csr(golden[f'{cname}/lat_weights']))
  k = regrid_np.longest(theirs[0]) + regrid_np.longest(theirs[1])
  for dtype in (np.float64, np.float32):
    out, a, count = regrid_np.nanmean(field.astype(dtype), *theirs,
                                      with_abs=True)
    assert out.dtype == dtype
    regrid_np.assert_within_reference(out, ref, a, count, k,
                                      f'{cname} conservative {dtype}')
    for cls, label in ((rg.ConservativeRegridder, 'conservative'),
                       (rg.BilinearRegridder, 'bilinear')):
      out, a, count, kk = regrid_np.run(cls(source, target),
                                        field.astype(dtype), with_abs=True)
      regrid_np.assert_within_reference(
          out, golden[f'{cname}/{label}/ref'], a, count, kk,
          f'{cname} {label} {dtype}')
  got = regrid_np.gather(field, golden[f'{cname}/nearest/indices'],
                         target.shape)
  np.testing.assert_array_equal(got, golden[f'{cname}/nearest/ref'])


@pytest.mark.parametrize('cname', CASES)
def test_nearest_table_against_the_reference(golden, built, cname):
  """Off ties the brute-force table is BallTree's.  Everywhere the chosen
  node is at the least distance of the full brute-force table, and no node of
  a lower flat index ties with it in both keys of the rule (sin^2(dlon / 2),
  then the distance).  Ties lie where geometry puts them: pole rows of the
  target, rows / columns midway between two source nodes."""
  case, source, target = built[cname]
  mine = rg.NearestRegridder(source, target).indices
  theirs = golden[f'{cname}/nearest/indices']
  ties = golden[f'{cname}/nearest/ties']
  assert mine.shape == theirs.shape == ties.shape
  assert mine.dtype == np.int64
  np.testing.assert_array_equal(mine[~ties], theirs[~ties])
  cols, rows = rc.tie_rows_and_columns(case['source'], case['target'])
  allowed = np.zeros(target.shape, dtype=bool)
  allowed[sorted(cols), :] = True
  allowed[:, sorted(rows)] = True
  assert not (ties.reshape(target.shape) & ~allowed).any()
  assert ties.mean() <= 1 / 3
  dist = regrid_np.haversine_matrix(case['source'], case['target'])
  at = np.arange(len(mine))
  np.testing.assert_array_equal(dist[at, mine], dist.min(axis=1))
  n_lat = source.shape[1]
  s_lon = np.deg2rad(np.asarray(source.longitudes, dtype=np.float64))
  t_lon = np.repeat(np.deg2rad(np.asarray(target.longitudes,
                                          dtype=np.float64)), target.shape[1])
  key_lon = np.sin((t_lon[:, None] - np.repeat(s_lon, n_lat)[None, :]) / 2) ** 2
  same = (dist == dist[at, mine][:, None]) & (
      key_lon == key_lon[at, mine][:, None])
  np.testing.assert_array_equal(np.argmax(same, axis=1), mine)


def test_known_answers_through_the_tables(golden):
  """The reference's known-answer tests (regridding_test.py:313-330, 495-591,
  593-618): the reference gave what is written there, and so do the product's
  tables through the restatement."""
  for kname, (cls, src, tgt, field, expected) in rc.known_answers().items():
    ref = golden[f'known/{kname}/ref']
    regridder = getattr(rg, cls)(rc.make_grid(rg, src), rc.make_grid(rg, tgt))
    if cls == 'NearestRegridder':
      got = regrid_np.gather(field, regridder.indices, regridder.target.shape)
    else:
      got = regrid_np.run(regridder, field.astype(np.float64))
    if expected is None:
      assert golden[f'known/{kname}/expected'].all()
      assert np.isfinite(got).all(), kname
    else:
      np.testing.assert_array_equal(golden[f'known/{kname}/expected'],
                                    expected)
      np.testing.assert_allclose(ref, expected, atol=rc.KNOWN_ATOL)
      np.testing.assert_allclose(got, expected, atol=rc.KNOWN_ATOL)


def test_restatement_rules():
  """0 / 0 -> NaN, NaN skipped, infinity local, node coincidence, clamping."""
  eye = regrid_np.csr(np.eye(3))
  pair = regrid_np.csr(np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5]]))
  f = np.array([[1.0, np.nan, 3.0], [np.nan, np.nan, 5.0],
                [np.inf, 2.0, 4.0]])
  out = regrid_np.nanmean(f, eye, pair)
  np.testing.assert_array_equal(out, [[1.0, 3.0], [np.nan, 5.0],
                                      [np.inf, 3.0]])
  tap = regrid_np.taps([0.0, 10.0, 20.0], [0.0, 5.0, 10.0, 20.0, 25.0], True)
  one = regrid_np.taps([0.0], [0.0], True)
  g = np.array([[1.0, np.nan, 3.0]])
  np.testing.assert_array_equal(regrid_np.linear(g, one, tap),
                                [[1.0, np.nan, np.nan, 3.0, 3.0]])
  tap = regrid_np.taps([0.0, 10.0, 20.0], [-1.0, 20.0, 21.0], False)
  np.testing.assert_array_equal(tap[3], [True, False, True])
  wrap = regrid_np.taps([0.0, 90.0, 180.0, 270.0], [315.0, -45.0], False, 360)
  np.testing.assert_array_equal(wrap[1], [3, 0, 3, 0])
  np.testing.assert_array_equal(wrap[2][0::2], [0.5, 0.5])


def test_host_side_argument_checks():
  source = rg.Grid.from_degrees(np.arange(0.0, 360, 45),
                                np.linspace(-90, 90, 5))
  target = rg.Grid.from_degrees(np.arange(0.0, 360, 90),
                                np.linspace(-90, 90, 3))
  for cls in (rg.NearestRegridder, rg.BilinearRegridder,
              rg.ConservativeRegridder):
    with pytest.raises(ValueError, match='to match'):
      cls(source, target).regrid_array(np.zeros((5, 8)))
    with pytest.raises(ValueError, match='to match'):
      cls(source, target).regrid_array(np.zeros((2, 8, 4)))
  with pytest.raises(NotImplementedError):
    rg.Regridder(source, target)._device_regrid(None, None, 0, True, False)


def test_entry_points_validate_their_arguments():
  from weatherbench2_amd import build, _lib
  build.build(verbose=False)
  h = _lib.load()
  f32, f64 = _lib.WB2_F32, _lib.WB2_F64
  buf = ctypes.create_string_buffer(64)
  p = ctypes.addressof(buf)

  def call(mode, dtype, n_slab, src=(4, 3), tgt=(2, 2), ptrs=p):
    return h.wb2_regrid_separable(
        mode, dtype, 1, ptrs, None, n_slab, src[0], src[1], tgt[0], tgt[1],
        ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, None)

  # empty launches are no-ops whatever the pointers are
  assert call(0, f32, 0, ptrs=None) == 0
  assert call(1, f64, 3, tgt=(0, 2), ptrs=None) == 0
  assert call(1, f64, 3, tgt=(2, 0), ptrs=None) == 0
  rc_ = call(0, f32, 2, ptrs=None)
  assert rc_ < 0 and b'null pointer' in h.wb2_last_error()
  for mode in (2, -1):
    assert call(mode, f32, 2) < 0 and b'unknown mode' in h.wb2_last_error()
  assert call(0, 7, 2) < 0 and b'unknown dtype' in h.wb2_last_error()
  assert call(0, f32, -1) < 0 and b'negative' in h.wb2_last_error()
  assert call(0, f32, 2, src=(0, 3)) < 0 and b'bad sizes' in h.wb2_last_error()
  # the gather
  g = h.wb2_regrid_gather
  assert g(4, None, None, 0, 12, None, 4, None, None) == 0
  assert g(4, None, None, 2, 12, None, 0, None, None) == 0
  assert g(4, None, None, 2, 12, None, 4, None, None) < 0
  assert b'null pointer' in h.wb2_last_error()
  for size in (0, 3, 16):
    assert g(size, p, None, 2, 12, p, 4, p, None) < 0
    assert b'bad sizes' in h.wb2_last_error()
  assert g(4, p, None, 2, 0, p, 4, p, None) < 0
  assert g(4, p, None, 2, 1 << 31, p, 4, p, None) < 0
  # the geometry query
  vals = [ctypes.c_int32() for _ in range(5)]
  refs = [ctypes.byref(v) for v in vals]
  assert h.wb2_regrid_geometry(f32, 1, 1, *refs) == 0
  tile, run, band, contig, slabs = (v.value for v in vals)
  assert tile == 1024 and run >= 1 and band >= 2 and slabs >= 1
  assert contig >= 1440, 'a 0.25-degree row fits the workgroup kernel'
  assert h.wb2_regrid_geometry(f64, 0, 1, *refs) == 0
  assert vals[0].value == 512 and vals[3].value >= 721
  assert h.wb2_regrid_geometry(f64, 0, 0, *refs) == 0
  assert vals[0].value == 256
  assert h.wb2_regrid_geometry(f32, 1, 1, None, None, None, None, None) < 0
  assert b'null pointer' in h.wb2_last_error()
  assert h.wb2_regrid_geometry(5, 1, 1, *refs) < 0
  assert b'unknown dtype' in h.wb2_last_error()
  from weatherbench2_amd import engine
  import torch
  geo = engine.regrid_geometry(torch.float32, True, True)
  assert geo['tile'] == tile and geo['max_contig'] == contig
