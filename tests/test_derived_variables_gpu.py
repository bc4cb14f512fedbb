"""The materialising derived variables on the GPU (csrc/derived_fields.hip):
WindSpeed bit for bit against NumPy, every other class against the
reference's fixture with a tolerance taken from the reference's own float32
noise, non-finite values compared (never skipped), the kernels' geometry
against the NumPy restatement, and `evaluate_chunks` keeping its chunk
programs and windows when a config uses these classes.
Reference: weatherbench2/derived_variables.py:76-338, 433-468;
evaluation.py:402-405."""
import dataclasses
import os

import numpy as np
import pytest

from tests import derived_cases as dc
from tests import derived_np
from tests import helpers, official_chunks as oc

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WIND = ('wind_speed', '10m_wind_speed')
F32_CASES = [c for c, b in dc.cases().items() if b()['dtype'] == 'float32']


@pytest.fixture(scope='module')
def golden():
  return dc.load_golden(GOLDEN_DIR)


def _dataset(variables, coords, device=True):
  import torch
  from weatherbench2_amd import xarray_lite as xl
  return xl.Dataset(
      {k: xl.DataArray(torch.from_numpy(np.ascontiguousarray(a)).cuda()
                       if device else a, d) for k, (d, a) in variables.items()},
      dict(coords))


def _make(label):
  from weatherbench2_amd import derived_variables as dv
  name, kwargs = dc.CLASSES[label]
  return getattr(dv, name)(**kwargs)


def _same_non_finite(got, want, msg):
  """NaN positions, infinity positions and the sign of every infinity."""
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
  inf = np.isinf(want)
  np.testing.assert_array_equal(np.isinf(got), inf, err_msg=msg)
  np.testing.assert_array_equal(np.sign(got[inf]), np.sign(want[inf]),
                                err_msg=msg)


# ---------------------------------------------------------------------------
# 5. WindSpeed: bit-identical
# ---------------------------------------------------------------------------
def test_the_classes_are_importable():
  from weatherbench2_amd.derived_variables import WindSpeed  # noqa: F401


@pytest.mark.parametrize('device', [True, False])
@pytest.mark.parametrize('cname', list(dc.cases()))
def test_wind_speed_equals_numpy_on_the_golden_cases(golden, cname, device):
  import torch
  case = dc.cases()[cname]()
  which = 'ref32' if case['dtype'] == 'float32' else 'ref64'
  ds = _dataset(case['vars'], case['coords'], device)
  for label in WIND:
    res = _make(label).compute(ds)
    want = golden[f'{cname}/{label}/{which}']
    assert isinstance(res.data, torch.Tensor) == device
    got = res.values
    assert got.dtype == want.dtype and got.shape == want.shape
    assert list(res.dims) == list(golden[f'{cname}/{label}/dims'])
    assert sorted(res.coords) == list(golden[f'{cname}/{label}/coords'])
    assert np.array_equal(got, want, equal_nan=True), (cname, label)
    assert np.isnan(want).sum() == np.isnan(got).sum()
    if case['dtype'] == 'float32':  # and float64 inputs of the same values
      res64 = _make(label).compute(
          _dataset(dc.as_float64(case)['vars'], case['coords'], device))
      assert np.array_equal(res64.values, golden[f'{cname}/{label}/ref64'],
                            equal_nan=True)


def _wind(shape, dtype, seed=0, nan=True):
  rs = np.random.RandomState(seed)
  u = (10 * rs.standard_normal(shape)).astype(dtype)
  v = (10 * rs.standard_normal(shape)).astype(dtype)
  if nan and u.size > 4:
    u.ravel()[rs.randint(0, u.size, 3)] = np.nan
    v.ravel()[rs.randint(0, v.size, 3)] = np.nan
  # exact zeros, tiny and huge values: the rounding of each step shows
  u.ravel()[0], v.ravel()[0] = 0.0, 0.0
  if u.size > 2:
    u.ravel()[1], v.ravel()[1] = dtype(3e-20), dtype(4e-20)
    u.ravel()[2], v.ravel()[2] = dtype(3e18), dtype(-4e18)
  return u, v


def _wind_speed(u, v, dims, coords=None):
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import xarray_lite as xl
  ds = xl.Dataset({'u': xl.DataArray(u, dims), 'v': xl.DataArray(v, dims)},
                  coords or {})
  return dv.WindSpeed('u', 'v').compute(ds)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_wind_speed_full_launch_and_odd_shapes(dtype):
  import torch
  dims = ('level', 'latitude', 'longitude')
  shapes = [(13, 721, 1440), (3, 1440, 721), (2, 5, 37), (2, 9, 1), (4, 1, 33),
            (1, 1, 1)]
  for shape in shapes:
    u, v = _wind(shape, dtype, seed=len(shape) + shape[-1])
    with np.errstate(all='ignore'):
      want = np.sqrt(u**2 + v**2)
    res = _wind_speed(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(),
                      dims)
    assert isinstance(res.data, torch.Tensor) and res.data.is_cuda
    got = res.values
    assert got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=True), shape
  # strided device views: every other slab (read in place through a slab
  # table), a column slice (copied), a transposed pair of spatial dims
  u, v = _wind((6, 19, 36), dtype, seed=5)
  gu, gv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
  with np.errstate(all='ignore'):
    want = np.sqrt(u**2 + v**2)
  for view in (lambda x: x[::2], lambda x: x[:, :, 1::3], lambda x: x[1:, 2:],
               lambda x: x[:, 3]):
    got = _wind_speed(view(gu), view(gv), dims[:view(gu).dim()]).values
    assert np.array_equal(got, view(want), equal_nan=True)
  # u and v in different dim orders: the result follows u
  res = _wind_speed_orders(gu, gv)
  assert res.dims == dims
  assert np.array_equal(res.values, want, equal_nan=True)


def _wind_speed_orders(gu, gv):
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import xarray_lite as xl
  ds = xl.Dataset({
      'u': xl.DataArray(gu, ('level', 'latitude', 'longitude')),
      'v': xl.DataArray(gv.permute(2, 0, 1).contiguous(),
                        ('longitude', 'level', 'latitude'))})
  return dv.WindSpeed('u', 'v').compute(ds)


def test_known_answers_of_the_reference(golden):
  for device in (True, False):
    for label, known in dc.KNOWN_ANSWERS.items():
      res = _make(label).compute(_dataset(known['vars'], known['coords'],
                                          device))
      want = golden[f'known/{label}/ref']
      assert res.values.dtype == want.dtype
      assert list(res.dims) == list(golden[f'known/{label}/dims'])
      np.testing.assert_allclose(res.values, known['expected'],
                                 atol=known['atol'], rtol=0)
      np.testing.assert_allclose(res.values, want, rtol=1e-12)


# ---------------------------------------------------------------------------
# 6, 7. every other class against the reference's fixture
# ---------------------------------------------------------------------------
OTHERS = [k for k in dc.CLASSES if k not in WIND]


@pytest.mark.parametrize('label', OTHERS)
@pytest.mark.parametrize('cname', list(dc.cases()))
def test_classes_against_the_reference(golden, cname, label):
  """float32 inputs: with noise = max |ref32 - ref64| over the finite points
  (the reference's own float32 error), max |hip - ref64| <= 4 noise; the
  margin is for an equally valid float32 evaluation order falling on the
  other side of the exact value.  float64 inputs: 1e-9 of the rms.  The
  ratio is printed (DESIGN.md section 4 records it)."""
  case = dc.cases()[cname]()
  key = f'{cname}/{label}'
  ref64 = golden[f'{key}/ref64']
  ok = np.isfinite(ref64)
  rms = np.sqrt(np.mean(ref64[ok] ** 2))
  if case['dtype'] == 'float32':
    ref32 = golden[f'{key}/ref32']
    res = _make(label).compute(_dataset(case['vars'], case['coords']))
    got = res.values
    assert got.dtype == ref32.dtype and got.shape == ref32.shape
    _same_non_finite(got, ref32, key)
    noise = np.abs(ref32[ok].astype(np.float64) - ref64[ok]).max()
    err = np.abs(got[ok].astype(np.float64) - ref64[ok]).max()
    print(f'RATIO {key}: max|hip - ref64| / noise = {err / noise:.3f} '
          f'(noise / rms = {noise / rms:.2e}, bit-equal to ref32: '
          f'{np.array_equal(got, ref32, equal_nan=True)})')
    assert err <= 4 * noise, (key, err / noise)
    case = dc.as_float64(case)
  res = _make(label).compute(_dataset(case['vars'], case['coords']))
  got = res.values
  assert got.dtype == ref64.dtype and got.shape == ref64.shape
  assert list(res.dims) == list(golden[f'{key}/dims'])
  assert sorted(res.coords) == list(golden[f'{key}/coords'])
  _same_non_finite(got, ref64, key)
  err = np.abs(got[ok] - ref64[ok]).max()
  assert err <= 1e-9 * rms, (key, err / rms)


def test_non_finite_counts(golden):
  """Exactly the equator row of the pole-and-equator grid for the six
  geostrophic / ageostrophic classes (360 of 6 840 points), nowhere else: a
  kernel cannot pass by producing NaNs, nor by hiding the reference's."""
  poles = dc.cases()['lonlat_poles']()
  mid = dc.cases()['latlon_linspace']()
  for label in dc.CLASSES:
    got = _make(label).compute(_dataset(poles['vars'],
                                        poles['coords'])).values
    bad = ~np.isfinite(got)
    if label in dc.GEOSTROPHIC:
      assert got.size == 6840 and bad.sum() == 360, label
      assert bad[..., 9].all()
    else:
      assert not bad.any(), label
    got = _make(label).compute(_dataset(mid['vars'], mid['coords'])).values
    assert np.isfinite(got).all(), label


# ---------------------------------------------------------------------------
# 8. geometry, against the NumPy restatement
# ---------------------------------------------------------------------------
def _stencil_case(dims, sizes, dtype, seed, latitude):
  rs = np.random.RandomState(seed)
  shape = tuple(sizes[d] for d in dims)
  variables = {
      'u_component_of_wind': (dims, 10.0 * rs.standard_normal(shape)),
      'v_component_of_wind': (dims, 8.0 * rs.standard_normal(shape)),
      'geopotential': (dims, 5e4 + 1e3 * rs.standard_normal(shape)),
  }
  variables = {k: (d, a.astype(dtype)) for k, (d, a) in variables.items()}
  coords = {'level': np.arange(sizes.get('level', 1)) * 100.0 + 300,
            'latitude': latitude,
            'longitude': np.arange(sizes['longitude'])
                         * (360.0 / sizes['longitude'])}
  return variables, coords


def _check_against_numpy(label, variables, coords, dtype):
  name, fields = dc.fields_of(label)
  res = _make(label).compute(_dataset(variables, coords))
  got = res.values
  as64 = {k: (d, a.astype(np.float64)) for k, (d, a) in variables.items()}
  dims, np64 = derived_np.compute(name, fields, as64, coords)
  assert res.dims == tuple(dims) and got.shape == np64.shape
  ok = np.isfinite(np64)
  if dtype == np.float32:
    _, np32 = derived_np.compute(name, fields, variables, coords)
    assert got.dtype == np32.dtype
    _same_non_finite(got, np32, label)
    noise = np.abs(np32[ok].astype(np.float64) - np64[ok]).max()
    err = np.abs(got[ok].astype(np.float64) - np64[ok]).max()
    assert err <= 4 * noise, (label, err / noise)
  else:
    assert got.dtype == np64.dtype
    _same_non_finite(got, np64, label)
    rms = np.sqrt(np.mean(np64[ok] ** 2))
    assert np.abs(got[ok] - np64[ok]).max() <= 1e-9 * rms, label


def _edge_sizes(dtype, wide):
  import torch
  from weatherbench2_amd import engine
  tile, rows = engine.stencil_geometry(
      torch.float32 if dtype == np.float32 else torch.float64, wide)
  return tile, rows


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('layout', ['latlon', 'lonlat'])
def test_stencil_tile_and_chunk_edges(dtype, layout):
  """Both slab layouts; row counts one below, at and one above the row chunk
  (and two chunks), column counts around the tile of the scalar and of the
  16-byte path.  The first / last row and column take the one-sided formula,
  rows at a chunk seam and columns at a tile seam read their neighbours from
  the other workgroup's part."""
  width = 4 if dtype == np.float32 else 2
  tile1, rows = _edge_sizes(dtype, False)
  tilew, _ = _edge_sizes(dtype, True)
  assert (tile1, tilew, rows) == (64, 64 * width, 16)
  n_rows = [rows - 1, rows, rows + 1, 2 * rows + 1]
  n_cols = [tile1 - 1, tile1 + 1, tilew - width, tilew, tilew + width, 2, 3]
  seed = 0
  for n_row in n_rows:
    for n_col in n_cols:
      seed += 1
      if layout == 'latlon':
        dims = ('level', 'latitude', 'longitude')
        sizes = dict(level=2, latitude=n_row, longitude=n_col)
      else:
        dims = ('level', 'longitude', 'latitude')
        sizes = dict(level=2, longitude=n_row, latitude=n_col)
      # poles and (for odd counts) the equator are on the grid
      latitude = np.linspace(-90, 90, sizes['latitude'])
      variables, coords = _stencil_case(dims, sizes, dtype, seed, latitude)
      for label in ('divergence', 'ageostrophic_wind_speed'):
        _check_against_numpy(label, variables, coords, dtype)


@pytest.mark.parametrize('label', [k for k in OTHERS
                                   if k != 'relative_humidity'])
def test_every_mode_on_both_layouts_and_a_non_uniform_axis(label):
  for dims in (('level', 'latitude', 'longitude'),
               ('level', 'longitude', 'latitude')):
    for dtype in (np.float32, np.float64):
      sizes = dict(level=3, latitude=37, longitude=40)
      latitude = np.sort(np.random.RandomState(3).uniform(-89, 89, 37))
      variables, coords = _stencil_case(dims, sizes, dtype, 9, latitude)
      _check_against_numpy(label, variables, coords, dtype)


def test_spatial_dims_that_are_not_last_and_strided_inputs():
  """A level axis between the spatial dims (the fields are gathered into
  slabs, the result comes back in the input's dim order) and inputs that are
  strided views of whole slabs (read in place)."""
  import torch
  from weatherbench2_amd import xarray_lite as xl
  dims = ('latitude', 'level', 'longitude')
  sizes = dict(level=3, latitude=19, longitude=36)
  variables, coords = _stencil_case(dims, sizes, np.float32, 4,
                                    np.linspace(-90, 90, 19))
  for label in ('vorticity', 'u_component_of_geostrophic_wind'):
    _check_against_numpy(label, variables, coords, np.float32)
  dims = ('time', 'level', 'latitude', 'longitude')
  sizes = dict(time=4, level=3, latitude=19, longitude=36)
  variables, coords = _stencil_case(dims, sizes, np.float32, 5,
                                    np.linspace(-90, 90, 19))
  full = _dataset(variables, coords)
  view = xl.Dataset({k: xl.DataArray(v.data[1::2, ::2], dims)
                     for k, v in full.data_vars.items()},
                    dict(coords, level=coords['level'][::2]))
  assert not view['geopotential'].data.is_contiguous()
  sub = {k: (d, a[1::2, ::2]) for k, (d, a) in variables.items()}
  for label in ('divergence', 'v_component_of_ageostrophic_wind'):
    name, fields = dc.fields_of(label)
    got = _make(label).compute(view)
    assert isinstance(got.data, torch.Tensor)
    want = _make(label).compute(_dataset(sub, view.coords)).values
    assert np.array_equal(got.values, want, equal_nan=True)


def test_an_axis_of_one_point_raises_like_np_gradient():
  dims = ('level', 'latitude', 'longitude')
  variables, coords = _stencil_case(
      dims, dict(level=1, latitude=1, longitude=8), np.float32, 1,
      np.array([10.0]))
  with pytest.raises(ValueError):
    _make('divergence').compute(_dataset(variables, coords))


def test_relative_humidity_reads_the_pressure_coordinate_by_name():
  """`level` anywhere among the dims, an integer and a float32 pressure
  coordinate (the latter keeps a float32 result, like NumPy)."""
  rs = np.random.RandomState(2)
  for dims in (('level', 'latitude', 'longitude'),
               ('latitude', 'level', 'longitude'),
               ('latitude', 'longitude', 'level')):
    sizes = dict(level=4, latitude=5, longitude=7)
    shape = tuple(sizes[d] for d in dims)
    for level in (np.array([300, 500, 850, 1000]),
                  np.array([300, 500, 850, 1000], dtype=np.float32)):
      variables = {
          'temperature': (dims, (250 + 40 * rs.random_sample(shape)
                                 ).astype(np.float32)),
          'specific_humidity': (dims, (1e-3 + 9e-3 * rs.random_sample(shape)
                                       ).astype(np.float32))}
      coords = {'level': level}
      name, fields = dc.fields_of('relative_humidity')
      _, np32 = derived_np.compute(name, fields, variables, coords)
      as64 = {k: (d, a.astype(np.float64)) for k, (d, a) in variables.items()}
      _, np64 = derived_np.compute(name, fields, as64, coords)
      res = _make('relative_humidity').compute(_dataset(variables, coords))
      got = res.values
      assert res.dims == dims and got.dtype == np32.dtype
      noise = np.abs(np32.astype(np.float64) - np64).max()
      assert np.abs(got.astype(np.float64) - np64).max() <= 4 * noise


# ---------------------------------------------------------------------------
# more slabs than one grid row holds
# ---------------------------------------------------------------------------
# One slab more than the 32768 outer indices of a grid row
# (csrc/launch_common.hpp; these kernels' geometry calls do not report it):
# the last slab lies in the second grid plane.  3 points: narrow, with a tail;
# 4 float32 points: one 16-byte lane.  Every slab holds its own random data, so
# a plane that reads or writes the slabs of plane 0 is caught.
SPLIT_SLABS = 32769
SPLIT_CASES = [(np.float32, 3), (np.float32, 4), (np.float64, 3)]
SPLIT_CHECKED = (0, 32767, 32768, SPLIT_SLABS - 1)


@pytest.mark.parametrize('dtype,n_point', SPLIT_CASES)
def test_pointwise_slabs_beyond_one_grid_row(dtype, n_point):
  """WindSpeed straight through the launch (the class folds contiguous slabs
  into one), bit for bit; RelativeHumidity, whose pressure is one value per
  slab, through the class with the tolerance of its neighbours."""
  import torch
  from weatherbench2_amd import engine
  dims = ('level', 'cell')
  u, v = _wind((SPLIT_SLABS, n_point), dtype, seed=n_point)
  _, want = derived_np.compute('WindSpeed', {'u_name': 'u', 'v_name': 'v'},
                               {'u': (dims, u), 'v': (dims, v)}, {})
  got = engine.derived_pointwise(
      'wind_speed', torch.from_numpy(u).cuda(), None,
      torch.from_numpy(v).cuda(), None, SPLIT_SLABS, n_point).cpu().numpy()
  assert got.dtype == want.dtype and got.shape == want.shape
  for o in SPLIT_CHECKED:
    assert np.array_equal(got[o], want[o], equal_nan=True), o
  assert np.array_equal(got, want, equal_nan=True)
  rs = np.random.RandomState(n_point)
  shape = (SPLIT_SLABS, 1, n_point)
  dims = ('level', 'latitude', 'longitude')
  variables = {
      'temperature': (dims, (250 + 40 * rs.random_sample(shape)).astype(dtype)),
      'specific_humidity': (dims, (1e-3 + 9e-3 * rs.random_sample(shape)
                                   ).astype(dtype))}
  coords = {'level': np.linspace(300.0, 1000.0, SPLIT_SLABS)}
  name, fields = dc.fields_of('relative_humidity')
  as64 = {k: (d, a.astype(np.float64)) for k, (d, a) in variables.items()}
  _, np64 = derived_np.compute(name, fields, as64, coords)
  _, np_in = derived_np.compute(name, fields, variables, coords)
  res = _make('relative_humidity').compute(_dataset(variables, coords))
  got = res.values
  assert res.dims == dims and got.dtype == np_in.dtype
  for o in SPLIT_CHECKED + (slice(None),):
    err = np.abs(got[o].astype(np.float64) - np64[o]).max()
    if dtype == np.float32:
      noise = np.abs(np_in[o].astype(np.float64) - np64[o]).max()
      assert err <= 4 * noise, (o, err / noise)
    else:
      assert err <= 1e-9 * np.sqrt(np.mean(np64[o] ** 2)), o


@pytest.mark.parametrize('dtype,n_lon', SPLIT_CASES)
def test_stencil_slabs_beyond_one_grid_row(dtype, n_lon):
  """Slabs of 2 x n_lon, the smallest np.gradient accepts, on both layouts."""
  for dims in (('level', 'latitude', 'longitude'),
               ('level', 'longitude', 'latitude')):
    sizes = dict(level=SPLIT_SLABS, latitude=2, longitude=n_lon)
    variables, coords = _stencil_case(dims, sizes, dtype, n_lon,
                                      np.array([-30.0, 40.0]))
    for label in ('divergence', 'ageostrophic_wind_speed'):
      _check_against_numpy(label, variables, coords, dtype)
      at = (0, 32767, 32768, SPLIT_SLABS - 1)
      few = {k: (d, a[list(at)]) for k, (d, a) in variables.items()}
      got = _make(label).compute(_dataset(variables, coords)).values[list(at)]
      want = _make(label).compute(_dataset(
          few, dict(coords, level=coords['level'][list(at)]))).values
      assert np.array_equal(got, want, equal_nan=True), (label, dims)


# ---------------------------------------------------------------------------
# 9. evaluate_chunks keeps windows and programs
# ---------------------------------------------------------------------------
def _derived():
  from weatherbench2_amd import derived_variables as dv
  return {
      'wind_speed': dv.WindSpeed(u_name='u_component_of_wind',
                                 v_name='v_component_of_wind'),
      '10m_wind_speed': dv.WindSpeed(u_name='10m_u_component_of_wind',
                                     v_name='10m_v_component_of_wind'),
      # two stencil classes (the level-column family is not in this build)
      'divergence': dv.WindDivergence(),
      'vorticity': dv.WindVorticity(),
  }


def _eval_setup(**kw):
  from weatherbench2_amd import config, evaluation, metrics as gm
  forecast, truth, _ = oc.make(**kw)
  lat, lon = forecast.coords['latitude'], forecast.coords['longitude']
  lsm = oc.land_sea_mask(len(lat), len(lon))
  oregions = oc.oracle_regions(lat, lon, lsm)
  gregions = {k: helpers.to_gpu_region(v) for k, v in oregions.items()}
  hf, ht = (helpers.to_gpu_dataset(x) for x in (forecast, truth))
  gf, gt = (evaluation.make_resident(x) for x in (hf, ht))
  wv = [gm.WindVectorMSE(u_name=u, v_name=v, vector_name=n)
        for u, v, n in oc.WIND]
  cfg = config.Eval(metrics={'mse': gm.MSE(wind_vector_mse=wv),
                             'mae': gm.MAE(), 'bias': gm.Bias()},
                    regions=gregions, derived_variables=_derived())
  return forecast, truth, oregions, hf, ht, gf, gt, cfg


def _same(a, b):
  assert sorted(a.data_vars) == sorted(b.data_vars)
  for name in a.data_vars:
    x, y = np.asarray(a[name].values), np.asarray(b[name].values)
    assert a[name].dims == b[name].dims and x.dtype == y.dtype, name
    assert np.array_equal(x, y, equal_nan=True), name


def _count_runs(monkeypatch):
  from weatherbench2_amd import program
  calls = []
  real = program.ChunkProgram.run

  def run(self, *a, **k):
    calls.append(1)
    return real(self, *a, **k)
  monkeypatch.setattr(program.ChunkProgram, 'run', run)
  return calls


@pytest.mark.parametrize('several', [False, True])
def test_evaluate_chunks_is_bit_identical_on_every_path(several, monkeypatch):
  from weatherbench2_amd import evaluation
  _, _, _, hf, ht, gf, gt, cfg = _eval_setup(n_init=4, n_lead=3, n_lat=31,
                                             n_lon=72)
  configs = ({'mean': cfg,
              'series': dataclasses.replace(cfg, temporal_mean=False)}
             if several else cfg)
  chunks = oc.chunk_pairs(gf, gt)
  fed = [(h, t) for (h, _), (_, t) in zip(oc.chunk_pairs(hf, ht), chunks)]
  before = [(sorted(f.data_vars), sorted(t.data_vars)) for f, t in chunks]
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = evaluation.evaluate_chunks(chunks, configs, False, prefetch=0,
                                    batch_chunks=1)
  compare = ((lambda a, b: [_same(a[k], b[k]) for k in b]) if several
             else _same)
  first = want['mean'] if several else want
  for name in _derived():
    assert name in first.data_vars
  monkeypatch.setattr(evaluation, '_STAGE_MIN_BYTES', 1024)
  for how in ('0', '1', 'verify'):
    monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', how)
    for batch in (1, 3, 8, None):
      kwargs = {} if batch is None else {'batch_chunks': batch}
      got = evaluation.evaluate_chunks(chunks, configs, False, prefetch=0,
                                       **kwargs)
      compare(got, want)
      got = evaluation.evaluate_chunks(fed, configs, False, prefetch=2,
                                       **kwargs)
      compare(got, want)
  # the caller's chunk Datasets hold no new variables
  assert before == [(sorted(f.data_vars), sorted(t.data_vars))
                    for f, t in chunks]
  assert all('wind_speed' not in f.data_vars for f, _ in fed)
  # the same configs WITHOUT derived variables over chunks into which
  # dv.compute was assigned beforehand
  assigned = []
  for f, t in chunks:
    f2, t2 = f.copy(), t.copy()
    for name, dv in _derived().items():
      f2[name] = dv.compute(f2)
      t2[name] = dv.compute(t2)
    assigned.append((f2, t2))
  strip = lambda c: dataclasses.replace(c, derived_variables={})
  plain = ({k: strip(c) for k, c in configs.items()} if several
           else strip(configs))
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  got = evaluation.evaluate_chunks(assigned, plain, False, prefetch=0)
  compare(got, want)


def test_the_fast_path_is_taken(monkeypatch):
  """Programs on: every chunk after the first of its structure is replayed
  (chunk by chunk), and a window holds more than one chunk (one fused launch
  for several chunks) -- neither happens for a config with derived variables
  on the generic path."""
  from weatherbench2_amd import engine, evaluation, program
  _, _, _, _, _, gf, gt, cfg = _eval_setup(n_init=4, n_lead=3, n_lat=31,
                                           n_lon=72)
  chunks = oc.chunk_pairs(gf, gt)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  calls = _count_runs(monkeypatch)
  evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0, batch_chunks=1)
  assert len(calls) == len(chunks) - 1, program.REASONS
  seen = []
  old = engine.set_launch_hook(lambda when, kernel: seen.append(kernel)
                               if when == 'begin' else None)
  try:
    evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                               batch_chunks=len(chunks))
  finally:
    engine.set_launch_hook(old)
  # one derived launch per class, chunk and dataset; far fewer fused passes
  # than chunks: the whole job is one window
  assert seen.count('derived_pointwise') == 2 * 2 * len(chunks), seen
  assert seen.count('derived_stencil') == 2 * 2 * len(chunks), seen
  assert 1 <= seen.count('stream_partials') < len(chunks) / 2, seen


def test_derived_mse_equals_the_oracles(monkeypatch):
  """MSE of the derived wind speed against the oracle's MSE of the NumPy wind
  speed (1e-9): per-chunk values averaged over init_time."""
  from oracle import evaluation_np as oe
  from oracle import metrics_np as om
  from oracle.named import DS, NA
  from weatherbench2_amd import evaluation
  forecast, truth, oregions, _, _, gf, gt, cfg = _eval_setup(
      n_init=3, n_lead=2, n_lat=19, n_lon=36)
  got = evaluation.evaluate_chunks(oc.chunk_pairs(gf, gt), cfg, False,
                                   prefetch=0)

  def with_speed(ds):
    out = dict(ds.items())
    for name, u, v in (('wind_speed', 'u_component_of_wind',
                        'v_component_of_wind'),
                       ('10m_wind_speed', '10m_u_component_of_wind',
                        '10m_v_component_of_wind')):
      out[name] = NA(np.sqrt(ds[u].data ** 2 + ds[v].data ** 2), ds[u].dims)
    return DS(out, ds.coords)
  per_chunk = oe.metric_and_region_loop(
      with_speed(forecast), with_speed(truth), {'mse': om.MSE()}, oregions,
      False, compute_chunk=True)
  metric_labels = list(got.coords['metric'])
  region_labels = list(got.coords['region'])
  checked = 0
  for (mname, rname), ds in per_chunk.items():
    mi, ri = metric_labels.index(mname), region_labels.index(rname)
    for var in ('wind_speed', '10m_wind_speed'):
      want = np.asarray(ds[var].data, dtype=np.float64)
      dims = tuple(ds[var].dims)
      want = want.mean(axis=dims.index('init_time'))
      dims = tuple(d for d in dims if d != 'init_time')
      order = [d for d in got[var].dims if d not in ('metric', 'region')]
      vals = np.transpose(got[var].values[mi, ri],
                          [order.index(d) for d in dims])
      helpers.assert_close(vals, want, rtol=1e-9, atol=1e-12,
                           err_msg=f'{rname}/{var}')
      checked += 1
  assert checked == 2 * len(oregions)


class _Doubled:  # a foreign, duck-typed derived variable
  base_variables = ['geopotential']

  def compute(self, dataset):
    return dataset['geopotential'] * 2.0


def test_a_foreign_derived_variable_keeps_the_old_path(monkeypatch):
  """WindSpeed mixed with a duck-typed object: the loop computes and assigns
  both per chunk, as before -- no program runs -- and the values are those of
  the fast path."""
  from weatherbench2_amd import config, evaluation, metrics as gm
  _, _, _, _, _, gf, gt, cfg = _eval_setup(n_init=3, n_lead=2, n_lat=19,
                                           n_lon=36)
  ws = {'wind_speed': _derived()['wind_speed']}
  metrics = {'mse': gm.MSE(), 'mae': gm.MAE()}
  fast = config.Eval(metrics=metrics, derived_variables=ws)
  mixed = config.Eval(metrics=metrics,
                      derived_variables=dict(ws, doubled=_Doubled()))
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  want = evaluation.evaluate_chunks(oc.chunk_pairs(gf, gt), fast, False,
                                    prefetch=0, batch_chunks=1)
  calls = _count_runs(monkeypatch)
  fresh = oc.chunk_pairs(gf, gt)  # (the old path assigns into the chunks)
  got = evaluation.evaluate_chunks(fresh, mixed, False, prefetch=0,
                                   batch_chunks=4)
  assert not calls
  assert 'doubled' in got.data_vars
  for name in want.data_vars:
    assert np.array_equal(got[name].values, want[name].values,
                          equal_nan=True), name
  # differing dicts across configs: the old path as well
  both = evaluation.evaluate_chunks(
      oc.chunk_pairs(gf, gt), {'a': fast, 'b': config.Eval(metrics=metrics)},
      False, prefetch=0, batch_chunks=1)
  assert 'wind_speed' in both['a'].data_vars
  assert 'wind_speed' not in both['b'].data_vars
  for name in want.data_vars:
    assert np.array_equal(both['a'][name].values, want[name].values,
                          equal_nan=True), name


def test_metric_and_region_loop_assigns_in_place_like_the_reference():
  from weatherbench2_amd import config, evaluation, metrics as gm
  _, _, _, _, _, gf, gt, _ = _eval_setup(n_init=1, n_lead=1, n_lat=19,
                                         n_lon=36)
  cfg = config.Eval(metrics={'mse': gm.MSE()},
                    derived_variables={'wind_speed': _derived()['wind_speed']})
  evaluation._metric_and_region_loop(gf, gt, cfg, False, compute_chunk=True)
  assert 'wind_speed' in gf.keys() and 'wind_speed' in gt.keys()
