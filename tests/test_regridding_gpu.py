"""The regridders on the MI355X (K11, csrc/regrid.hip): every fixture case
through `regrid_array` and `regrid_dataset`, bit for bit against the NumPy
restatement of the header (tests/regrid_np.py) and within the derived bound of
the reference; the reference's known answers; the kernels at their geometry
edges (taken from wb2_regrid_geometry) on hand-made tables; views, gathers and
a decreasing latitude read where they lie; and a regridded chunk through a
metric.

The bound against the reference (regrid_np.reference_bound) is derived, not
measured.  Both sides form the same two nested sums of at most K = (longest
longitude band + longest latitude band) products in float64, with weights that
agree to 1e-12 and in a different order.  With gamma = (K + 4) 2^-53 and A the
same sums over |field| with |w|: |hip64 - ref| <= 4 gamma A / |count| +
1e-12 A, |hip32 - ref| <= the same + 2^-24 |ref|; NaN positions are equal.
(A is the sum, not the mean: the tightest reading of that bound.)
"""
import ctypes
import os

import numpy as np
import pytest

from tests import regrid_cases as rc
from tests import regrid_np

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = list(rc.cases())
SEPARABLE = (('ConservativeRegridder', 'conservative'),
             ('BilinearRegridder', 'bilinear'))


@pytest.fixture(scope='module')
def golden():
  return rc.load_golden(GOLDEN_DIR)


@pytest.fixture(scope='module')
def built():
  from weatherbench2_amd import regridding as rg
  out = {}
  for cname, build in rc.cases().items():
    case = build()
    out[cname] = (case, rc.make_grid(rg, case['source']),
                  rc.make_grid(rg, case['target']))
  return out


_EXPECTED: dict = {}


def _expected(built, cname, cls, dtype):
  """(out, A, count, K) of the restatement, computed once and left alone."""
  from weatherbench2_amd import regridding as rg
  key = (cname, cls, np.dtype(dtype).name)
  if key not in _EXPECTED:
    case, source, target = built[cname]
    res = regrid_np.run(getattr(rg, cls)(source, target),
                        case['field'].astype(dtype), with_abs=True)
    for a in res[:3]:
      a.setflags(write=False)
    _EXPECTED[key] = res
  return _EXPECTED[key]


def _bit_equal(got, want, msg):
  """The same bits wherever the value is a number (NaN payloads and signs
  are the hardware's: NaN positions must be equal)."""
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), msg
  assert got[~nan].tobytes() == want[~nan].tobytes(), msg


def _torch_dtype(dtype):
  import torch
  return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def test_the_module_and_its_entry_points_exist():
  from weatherbench2_amd import _lib
  from weatherbench2_amd.regridding import (  # noqa: F401
      BilinearRegridder, ConservativeRegridder, Grid, NearestRegridder)
  h = _lib.load()
  for name in ('wb2_regrid_separable', 'wb2_regrid_gather',
               'wb2_regrid_geometry'):
    assert hasattr(h, name) and name in _lib.exported_symbols()


# ---------------------------------------------------------------------------
# every fixture case through `regrid_array` and `regrid_dataset`
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('cname', CASES)
def test_regrid_array_matches_restatement_and_reference(golden, built, cname,
                                                        dtype):
  import torch
  from weatherbench2_amd import regridding as rg
  case, source, target = built[cname]
  field = case['field'].astype(dtype)
  for cls, label in SEPARABLE:
    want, a, count, k = _expected(built, cname, cls, dtype)
    regridder = getattr(rg, cls)(source, target)
    dev = regridder.regrid_array(torch.from_numpy(field).cuda())
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert dev.dtype == _torch_dtype(dtype)
    host = regridder.regrid_array(field)
    assert isinstance(host, np.ndarray)
    for got in (dev.cpu().numpy(), host):
      _bit_equal(got, want, (cname, label))
      regrid_np.assert_within_reference(
          got, golden[f'{cname}/{label}/ref'], a, count, k, (cname, label))
  nearest = rg.NearestRegridder(source, target)
  want = regrid_np.gather(field, nearest.indices, target.shape)
  got = nearest.regrid_array(torch.from_numpy(field).cuda())
  _bit_equal(got.cpu().numpy(), want, (cname, 'nearest'))
  _bit_equal(nearest.regrid_array(field), want, (cname, 'nearest host'))
  ties = golden[f'{cname}/nearest/ties'].reshape(target.shape)
  ref = golden[f'{cname}/nearest/ref'].astype(dtype)
  np.testing.assert_array_equal(want[..., ~ties], ref[..., ~ties])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('cname', CASES)
def test_regrid_dataset_in_both_layouts(golden, built, cname, dtype):
  """(.., latitude, longitude) and (.., longitude, latitude) variables of one
  dataset, device-backed and host-backed: the same bits as `regrid_array`'s
  restatement, the target's coordinates, every variable in its own dimension
  order; a variable without the horizontal dims passes through."""
  import torch
  from weatherbench2_amd import regridding as rg
  from weatherbench2_amd import xarray_lite as xl
  case, source, target = built[cname]
  field = case['field'].astype(dtype)
  lead = tuple(f'd{i}' for i in range(field.ndim - 2))
  lonlat = lead + ('longitude', 'latitude')
  latlon = lead + ('latitude', 'longitude')
  swapped = np.ascontiguousarray(np.swapaxes(field, -1, -2))
  extra = np.arange(3.0)
  for on_device in (True, False):
    put = (lambda a: torch.from_numpy(a).cuda()) if on_device else (lambda a: a)
    ds = xl.Dataset(
        {'a': xl.DataArray(put(field), lonlat),
         'b': xl.DataArray(put(swapped), latlon),
         'c': xl.DataArray(extra, ('other',))},
        {'longitude': case['source']['longitudes'],
         'latitude': case['source']['latitudes'], 'other': np.arange(3)})
    for cls, label in SEPARABLE + (('NearestRegridder', 'nearest'),):
      regridder = getattr(rg, cls)(source, target)
      if cls == 'NearestRegridder':
        want = regrid_np.gather(field, regridder.indices, target.shape)
      else:
        want, a, count, k = _expected(built, cname, cls, dtype)
      out = regridder.regrid_dataset(ds)
      assert out['a'].dims == lonlat and out['b'].dims == latlon
      assert isinstance(out['a'].data, torch.Tensor) == on_device
      np.testing.assert_array_equal(out.coords['latitude'], target.latitudes)
      np.testing.assert_array_equal(out.coords['longitude'],
                                    target.longitudes)
      _bit_equal(out['a'].values, want, (cname, label, 'lonlat'))
      _bit_equal(np.swapaxes(out['b'].values, -1, -2), want,
                 (cname, label, 'latlon'))
      np.testing.assert_array_equal(out['c'].values, extra)
      if cls != 'NearestRegridder':
        regrid_np.assert_within_reference(
            np.swapaxes(out['b'].values, -1, -2),
            golden[f'{cname}/{label}/ref'], a, count, k, (cname, label))


@pytest.mark.parametrize('lead', rc.BATCH_LEADS)
def test_leading_dims(built, lead):
  import torch
  from weatherbench2_amd import regridding as rg
  case, source, target = built['batch']
  field = np.ascontiguousarray(rc.batch_view(case['field'], lead))
  assert field.shape[:-2] == lead
  for cls in ('ConservativeRegridder', 'BilinearRegridder'):
    regridder = getattr(rg, cls)(source, target)
    got = regridder.regrid_array(torch.from_numpy(field).cuda())
    assert tuple(got.shape) == lead + target.shape
    _bit_equal(got.cpu().numpy(), regrid_np.run(regridder, field), (cls, lead))
  nearest = rg.NearestRegridder(source, target)
  got = nearest.regrid_array(torch.from_numpy(field).cuda())
  _bit_equal(got.cpu().numpy(),
             regrid_np.gather(field, nearest.indices, target.shape), lead)


def test_known_answers_on_the_device(golden):
  """regridding_test.py:313-330, 495-591, 593-618 through the kernels."""
  import torch
  from weatherbench2_amd import regridding as rg
  for kname, (cls, src, tgt, field, expected) in rc.known_answers().items():
    regridder = getattr(rg, cls)(rc.make_grid(rg, src), rc.make_grid(rg, tgt))
    got = regridder.regrid_array(torch.from_numpy(field).cuda()).cpu().numpy()
    if cls == 'NearestRegridder':
      assert got.dtype == field.dtype  # integers stay integers
    else:
      assert got.dtype == np.float64  # integers are computed as float64
    if expected is None:
      assert np.isfinite(got).all(), kname
    else:
      np.testing.assert_allclose(got, expected, atol=rc.KNOWN_ATOL,
                                 err_msg=kname)
      np.testing.assert_allclose(got, golden[f'known/{kname}/ref'],
                                 atol=1e-12, err_msg=kname)


def test_dtypes_of_the_nearest_gather(built):
  """Elements of 1, 2, 4 and 8 bytes keep their dtype and their bits."""
  import torch
  from weatherbench2_amd import regridding as rg
  case, source, target = built['global']
  nearest = rg.NearestRegridder(source, target)
  rs = np.random.RandomState(3)
  for dtype in (np.bool_, np.uint8, np.int16, np.float16, np.int32, np.int64,
                np.float64):
    field = rs.randint(0, 2 if dtype is np.bool_ else 100,
                       size=(2,) + source.shape).astype(dtype)
    got = nearest.regrid_array(torch.from_numpy(field).cuda()).cpu().numpy()
    want = regrid_np.gather(field, nearest.indices, target.shape)
    assert got.dtype == want.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------
# geometry edges on hand-made tables
# ---------------------------------------------------------------------------
def _random_table(rs, n_target, n_source, max_band, wrap=False, nan_at=()):
  """A banded table with bands of 1 .. max_band entries (the longest one is
  used at least once), as the restatement's tuple."""
  ptr, idx, w, nan = [0], [], [], np.zeros(n_target, dtype=bool)
  for k in range(n_target):
    if k in nan_at:
      nan[k] = True
    else:
      n = min(n_source, max_band if k == 0 else rs.randint(1, max_band + 1))
      start = rs.randint(0, n_source) if wrap else rs.randint(
          0, n_source - n + 1)
      band = (start + np.arange(n)) % n_source
      weights = rs.random_sample(n) + 0.1
      idx += band.tolist()
      w += (weights / weights.sum()).tolist()
    ptr.append(len(idx))
  return (np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int64),
          np.array(w, dtype=np.float64), nan)


def _random_taps(rs, n_target, n_source, nan_at=()):
  ptr = 2 * np.arange(n_target + 1, dtype=np.int64)
  i0 = rs.randint(0, n_source, size=n_target)
  i1 = (i0 + 1) % n_source
  t = rs.random_sample(n_target)
  t[::3] = 0.0  # node coincidence
  i1 = np.where(t == 0, i0, i1)
  nan = np.zeros(n_target, dtype=bool)
  nan[list(nan_at)] = True
  idx = np.stack([i0, i1], axis=1).ravel().astype(np.int64)
  return ptr, idx, np.stack([t, np.zeros_like(t)], axis=1).ravel(), nan


def _device_tables(lon_table, lat_table):
  import torch
  out = []
  for ptr, idx, w, nan in (lon_table, lat_table):
    out += [torch.from_numpy(ptr.astype(np.int32)).cuda(),
            torch.from_numpy(idx.astype(np.int32)).cuda(),
            torch.from_numpy(w).cuda(),
            torch.from_numpy(nan.astype(np.uint8)).cuda()]
  return out


def _field(rs, shape, dtype, nan_share=0.1):
  f = (rs.standard_normal(shape) * 10 + 3).astype(dtype)
  f[rs.random_sample(shape) < nan_share] = np.nan
  return f


def _run_tables(mode, field, lat_rows, lon_table, lat_table, misalign=False):
  """`field` is (slab, lon, lat); the device reads it in the asked layout."""
  import torch
  from weatherbench2_amd import engine
  n_slab, s_lon, s_lat = field.shape
  t_lon, t_lat = len(lon_table[3]), len(lat_table[3])
  laid = np.ascontiguousarray(np.swapaxes(field, 1, 2)) if lat_rows else field
  if misalign:
    buf = torch.empty(laid.size + 1, dtype=_torch_dtype(field.dtype),
                      device='cuda')
    buf[1:] = torch.from_numpy(laid).cuda().reshape(-1)
    x = buf[1:].view(laid.shape)
    assert x.data_ptr() % 16 != 0
  else:
    x = torch.from_numpy(laid).cuda()
    assert x.data_ptr() % 16 == 0
  out = engine.regrid_separable(mode, x, None, n_slab, lat_rows,
                                (s_lon, s_lat), (t_lon, t_lat),
                                _device_tables(lon_table, lat_table))
  out = out.cpu().numpy().reshape(
      (n_slab, t_lat, t_lon) if lat_rows else (n_slab, t_lon, t_lat))
  return np.swapaxes(out, 1, 2) if lat_rows else out


def _check_tables(mode, field, lat_rows, lon_table, lat_table, msg,
                  misalign=False):
  fn = regrid_np.nanmean if mode == 'nanmean' else regrid_np.linear
  want = fn(field, lon_table, lat_table)
  got = _run_tables(mode, field, lat_rows, lon_table, lat_table, misalign)
  _bit_equal(got, want, msg)


@pytest.mark.parametrize('wide', [True, False])
@pytest.mark.parametrize('lat_rows', [True, False])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_contiguous_axis_at_the_tile_edges(dtype, lat_rows, wide):
  """Contiguous-axis lengths of one tile less a vector (an element on the
  scalar path), one tile, one tile more, and a single element; the wide path
  is taken when the length is a multiple of the vector and the base aligned,
  the scalar path by an odd length or a base one element in."""
  from weatherbench2_amd import engine
  geo = engine.regrid_geometry(_torch_dtype(dtype), lat_rows, wide)
  vec = geo['tile'] // engine.regrid_geometry(_torch_dtype(dtype), lat_rows,
                                              False)['tile']
  assert vec == ((4 if dtype == np.float32 else 2) if wide else 1)
  rs = np.random.RandomState(11)
  lengths = [geo['tile'] - vec, geo['tile'], geo['tile'] + vec]
  if not wide:
    lengths.append(1)
  for n in lengths:
    assert n <= geo['max_contig']
    other = 5
    s_lon, s_lat = (n, other) if lat_rows else (other, n)
    field = _field(rs, (2, s_lon, s_lat), dtype)
    for mode in ('nanmean', 'linear'):
      if mode == 'nanmean':
        lon = _random_table(rs, 7, s_lon, min(3, s_lon), wrap=True, nan_at=(2,))
        lat = _random_table(rs, 4, s_lat, min(3, s_lat), nan_at=(1,))
      else:
        lon = _random_taps(rs, 7, s_lon, nan_at=(2,))
        lat = _random_taps(rs, 4, s_lat, nan_at=(1,))
      # an even length on the scalar path: the base one element in
      misalign = not wide and n % (4 if dtype == np.float32 else 2) == 0
      _check_tables(mode, field, lat_rows, lon, lat,
                    (mode, n, lat_rows, wide), misalign=misalign)


@pytest.mark.parametrize('lat_rows', [True, False])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bands_runs_and_target_tiles(dtype, lat_rows):
  """Bands of exactly what a thread holds, one more, and two pieces and a
  rest, on both axes; target-row counts of one run and one more (one less is
  the empty launch); more target latitudes than one workgroup's threads in
  the (lon, lat) layout."""
  import torch
  from weatherbench2_amd import engine
  geo = engine.regrid_geometry(_torch_dtype(dtype), lat_rows, True)
  band, run = geo['band'], geo['run']
  rs = np.random.RandomState(12)
  s_lon, s_lat = 40, 36
  field = _field(rs, (3, s_lon, s_lat), dtype)
  for longest in (band, band + 1, 2 * band + 3):
    for n_rows in (run, run + 1):
      t_lon, t_lat = (9, n_rows) if lat_rows else (n_rows, 9)
      lon = _random_table(rs, t_lon, s_lon, longest, wrap=True)
      lat = _random_table(rs, t_lat, s_lat, longest)
      assert regrid_np.longest(lon) == regrid_np.longest(lat) == longest
      _check_tables('nanmean', field, lat_rows, lon, lat,
                    (longest, n_rows, lat_rows))
  # one run less: nothing to do, nothing written
  x = torch.from_numpy(field).cuda()
  lon = _random_table(rs, 0 if not lat_rows else 9, s_lon, 3)
  lat = _random_table(rs, 0 if lat_rows else 9, s_lat, 3)
  out = engine.regrid_separable(
      'nanmean', x, None, 3, lat_rows, (s_lon, s_lat),
      (len(lon[3]), len(lat[3])), _device_tables(lon, lat))
  assert out.numel() == 0
  # 257 target latitudes: two workgroups per target longitude in (lon, lat)
  lon = _random_table(rs, 3, s_lon, 4, wrap=True)
  lat = _random_table(rs, 257, s_lat, 4, nan_at=(256,))
  _check_tables('nanmean', field, lat_rows, lon, lat, ('257', lat_rows))
  _check_tables('linear', field, lat_rows, _random_taps(rs, 3, s_lon),
                _random_taps(rs, 257, s_lat, nan_at=(0,)), ('257 linear',))


@pytest.mark.parametrize('lat_rows', [True, False])
def test_misaligned_base_falls_back_to_scalar_loads(lat_rows):
  """A view that starts one element in: the same bits as the aligned copy."""
  rs = np.random.RandomState(13)
  for dtype in (np.float32, np.float64):
    field = _field(rs, (2, 24, 16), dtype)
    lon = _random_table(rs, 5, 24, 9, wrap=True)
    lat = _random_table(rs, 6, 16, 9)
    for misalign in (False, True):
      _check_tables('nanmean', field, lat_rows, lon, lat, (dtype, misalign),
                    misalign=misalign)


@pytest.mark.parametrize('lat_rows', [True, False])
def test_slab_counts_at_the_grid_edge(lat_rows):
  """One slab, and one more than a full grid row of workgroups."""
  import torch
  from weatherbench2_amd import engine
  geo = engine.regrid_geometry(torch.float32, lat_rows, False)
  rs = np.random.RandomState(14)
  lon = _random_table(rs, 2, 3, 2, wrap=True)
  lat = _random_table(rs, 1, 2, 2)
  for n_slab in (1, geo['grid_slabs'] + 1):
    field = _field(rs, (n_slab, 3, 2), np.float32)
    got = _run_tables('nanmean', field, lat_rows, lon, lat)
    _bit_equal(got, regrid_np.nanmean(field, lon, lat), n_slab)
  # the gather counts its slabs the same way
  index = torch.tensor([5, 0, 3], dtype=torch.int32, device='cuda')
  flat = field.reshape(n_slab, 6)
  got = engine.regrid_gather(torch.from_numpy(flat).cuda(), None, n_slab, 6,
                             index)
  _bit_equal(got.cpu().numpy(), flat[:, [5, 0, 3]], 'gather')


@pytest.mark.parametrize('lat_rows', [True, False])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_contiguous_axis_beyond_the_workgroup_kernels(dtype, lat_rows):
  """One vector more than the LDS of the workgroup kernels holds: the kernel
  of one thread per cell gives the same values."""
  from weatherbench2_amd import engine
  geo = engine.regrid_geometry(_torch_dtype(dtype), lat_rows, True)
  n = geo['max_contig'] + 4
  rs = np.random.RandomState(15)
  s_lon, s_lat = (n, 3) if lat_rows else (3, n)
  field = _field(rs, (2, s_lon, s_lat), dtype)
  lon = _random_table(rs, 5, s_lon, 3, wrap=True, nan_at=(4,))
  lat = _random_table(rs, 4, s_lat, 3)
  _check_tables('nanmean', field, lat_rows, lon, lat, ('cell', n))
  _check_tables('linear', field, lat_rows, _random_taps(rs, 5, s_lon),
                _random_taps(rs, 4, s_lat, nan_at=(3,)), ('cell linear', n))


def test_infinity_reaches_only_the_cells_it_overlaps(built):
  """Documented difference: the reference's dense contraction makes every
  other cell of the slab NaN (0 * inf)."""
  import torch
  from weatherbench2_amd import regridding as rg
  case, source, target = built['global']
  field = case['field'].copy()
  field[10, 12] = np.inf
  regridder = rg.ConservativeRegridder(source, target)
  got = regridder.regrid_array(torch.from_numpy(field).cuda()).cpu().numpy()
  _bit_equal(got, regrid_np.run(regridder, field), 'inf')
  assert 1 <= np.isinf(got).sum() <= 4 and not np.isnan(got).any()


# ---------------------------------------------------------------------------
# views, gathers, a decreasing latitude: read where they lie
# ---------------------------------------------------------------------------
def test_views_gathers_and_reversed_latitude_are_read_in_place(built,
                                                               monkeypatch):
  import torch
  from weatherbench2_amd import engine
  from weatherbench2_amd import regridding as rg
  from weatherbench2_amd import xarray_lite as xl
  case, source, target = built['global']
  n_lon, n_lat = source.shape
  rs = np.random.RandomState(16)
  host = _field(rs, (3, 7, n_lat, n_lon), np.float32, nan_share=0.02)
  full = torch.from_numpy(host).cuda()
  dims = ('time', 'lead', 'latitude', 'longitude')
  coords = {'latitude': case['source']['latitudes'],
            'longitude': case['source']['longitudes']}
  regridder = rg.ConservativeRegridder(source, target)
  expect = lambda a: np.swapaxes(
      regrid_np.run(regridder, np.swapaxes(a, -1, -2)), -1, -2)
  calls = []
  real = engine.regrid_separable

  def spy(mode, x, slab, *a, **k):
    calls.append((x.data_ptr(), None if slab is None
                  else slab.cpu().numpy().copy()))
    return real(mode, x, slab, *a, **k)
  monkeypatch.setattr(engine, 'regrid_separable', spy)
  copies = []
  real_c = torch.Tensor.contiguous
  monkeypatch.setattr(torch.Tensor, 'contiguous',
                      lambda self, *a, **k: (copies.append(
                          self.is_contiguous()), real_c(self, *a, **k))[1])
  # the contiguous tensor
  ds = xl.Dataset({'t': xl.DataArray(full, dims)}, coords)
  whole = regridder.regrid_dataset(ds)['t']
  assert calls[-1] == (full.data_ptr(), None)
  _bit_equal(whole.values, expect(host), 'contiguous')
  # a lead-sliced view: every other lead of every time
  view = full[:, ::2]
  assert not view.is_contiguous()
  got = regridder.regrid_dataset(
      xl.Dataset({'t': xl.DataArray(view, dims)}, coords))['t']
  ptr, table = calls[-1]
  assert ptr == full.data_ptr() and all(copies)
  assert np.array_equal(table, (np.arange(3)[:, None] * 7
                                + 2 * np.arange(4)[None, :]).ravel())
  _bit_equal(got.values, np.ascontiguousarray(whole.values[:, ::2]), 'view')
  # a gather through the slab table
  base = full.reshape(-1, n_lat, n_lon)
  index = np.stack([rs.permutation(7) + t * 7 for t in (2, 0)])
  materialized = []
  real_m = xl.SlabGather.materialize
  monkeypatch.setattr(xl.SlabGather, 'materialize',
                      lambda self, *a, **k: (materialized.append(1),
                                             real_m(self, *a, **k))[1])
  got = regridder.regrid_dataset(xl.Dataset(
      {'t': xl.DataArray(xl.SlabGather(base, index), dims)}, coords))['t']
  ptr, table = calls[-1]
  assert ptr == base.data_ptr() and not materialized and all(copies)
  assert np.array_equal(table, index.ravel())
  _bit_equal(got.values, whole.values.reshape((-1,) + whole.shape[2:])[index],
             'gather')
  # a decreasing latitude: the same tensor read in reverse through the table
  flipped = torch.from_numpy(np.ascontiguousarray(host[:, :, ::-1])).cuda()
  got = regridder.regrid_dataset(xl.Dataset(
      {'t': xl.DataArray(flipped, dims)},
      {'latitude': case['source']['latitudes'][::-1],
       'longitude': coords['longitude']}))
  assert calls[-1] == (flipped.data_ptr(), None) and all(copies)
  np.testing.assert_array_equal(got.coords['latitude'], target.latitudes)
  _bit_equal(got['t'].values, whole.values, 'decreasing latitude')
  for cls in (rg.BilinearRegridder, rg.NearestRegridder):
    a = cls(source, target).regrid_dataset(ds)['t'].values
    b = cls(source, target).regrid_dataset(xl.Dataset(
        {'t': xl.DataArray(flipped, dims)},
        {'latitude': case['source']['latitudes'][::-1],
         'longitude': coords['longitude']}))['t'].values
    _bit_equal(b, a, cls.__name__)
  assert np.array_equal(full.cpu().numpy(), host, equal_nan=True)


# ---------------------------------------------------------------------------
# end to end: a regridded chunk goes into a metric without leaving the device
# ---------------------------------------------------------------------------
def test_regridded_chunk_through_a_metric(built):
  import torch
  from weatherbench2_amd import metrics as gm
  from weatherbench2_amd import regridding as rg
  from weatherbench2_amd import xarray_lite as xl
  case, source, target = built['global']
  n_lon, n_lat = source.shape
  rs = np.random.RandomState(17)
  forecast = (280 + 5 * rs.standard_normal((4, n_lat, n_lon))).astype(
      np.float32)
  truth = (280 + 5 * rs.standard_normal((4,) + target.shape[::-1])).astype(
      np.float32)
  dims = ('time', 'latitude', 'longitude')
  time = np.arange(4) * np.timedelta64(6, 'h') + np.datetime64('2020-01-01',
                                                               'ns')
  regridder = rg.ConservativeRegridder(source, target)
  fine = xl.Dataset(
      {'temperature': xl.DataArray(torch.from_numpy(forecast).cuda(), dims)},
      {'time': time, 'latitude': case['source']['latitudes'],
       'longitude': case['source']['longitudes']})
  coarse = regridder.regrid_dataset(fine)
  assert coarse['temperature'].data.is_cuda
  coords = {'time': time, 'latitude': np.asarray(target.latitudes),
            'longitude': np.asarray(target.longitudes)}
  truth_ds = xl.Dataset({'temperature': xl.DataArray(
      torch.from_numpy(truth).cuda(), dims)}, coords)
  got = gm.MSE().compute_chunk(coarse, truth_ds)['temperature']
  regridded = np.swapaxes(regrid_np.run(
      regridder, np.swapaxes(forecast, -1, -2)), -1, -2)
  host_ds = xl.Dataset({'temperature': xl.DataArray(regridded, dims)}, coords)
  truth_host = xl.Dataset({'temperature': xl.DataArray(truth, dims)}, coords)
  want = gm.MSE().compute_chunk(host_ds, truth_host)['temperature']
  assert got.dims == want.dims
  np.testing.assert_allclose(got.values, want.values, rtol=1e-9, atol=1e-12)
