"""Quantiles on the GPU (csrc/quantile.hip): every fixture case through the
public interface, the C ABI over the sizes at which the kernels change path
(tile edges, the resident / streaming threshold from wb2_quantile_geometry,
unaligned buffers), the slab table (views, gathers, permuted samples),
isolation of NaN and inf between the points of a tile, and the result handed
to thresholds.QuantileThreshold.  "Bit-equal" is NaN in the same places and
the same bytes elsewhere, +0.0 and -0.0 counting as equal
(tests/quantile_np.assert_bit_equal).
Reference: scripts/compute_quantiles.py:168-183."""
import os

import numpy as np
import pytest

from tests import quantile_cases as qc
from tests import quantile_np as qn
from tests import test_quantiles_cpu as cpu

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = cpu.CASES
MODES = cpu.MODES
# 0, 1, an exact middle, duplicates, unsorted; more than share a streaming pass
Q = [0.5, 0.0, 1.0, 0.37, 0.9, 0.37, 0.999]


@pytest.fixture(scope='module')
def golden():
  return qc.load_golden(GOLDEN_DIR)


def _torch_dtype(dtype):
  import torch
  return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _geometry(dtype):
  from weatherbench2_amd import engine
  return engine.quantile_geometry(_torch_dtype(dtype))


def _series(shape, dtype, seed):
  """[n_outer, n_red, n_inner] of mixed sign: every third point rounded to
  whole numbers (ties), NaNs scattered over every fourth point, an all-NaN
  point and a +-inf pair where the shape has room."""
  rs = np.random.RandomState(seed)
  x = (rs.standard_normal(shape) * 10).astype(dtype)
  x[..., ::3] = np.round(x[..., ::3])
  holes = rs.random_sample(shape) < 0.1
  holes[..., [i for i in range(shape[-1]) if i % 4 != 1]] = False
  x[holes] = np.nan
  if shape[-1] > 6:
    x[..., 6] = np.nan
  if shape[-1] > 2 and shape[1] > 2:
    x[0, 0, 2], x[0, shape[1] - 1, 2] = np.inf, -np.inf
  return x


def _select(x, q, skipna, slab=None, shape=None):
  """wb2_quantile_select on a device tensor -> NumPy [n_q, n_outer, n_inner]."""
  import torch
  from weatherbench2_amd import engine
  n_outer, n_red, n_inner = shape or x.shape
  table = None if slab is None else torch.from_numpy(
      np.ascontiguousarray(slab, dtype=np.int64)).cuda()
  out = engine.quantile_select(x, table, n_outer, n_red, n_inner, q, skipna)
  assert out.dtype == torch.float64 and out.is_cuda
  assert tuple(out.shape) == (len(q), n_outer, n_inner)
  return out.cpu().numpy()


# ---------------------------------------------------------------------------
# every fixture case through `quantile` / `compute_quantiles`
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cname', CASES)
def test_fixture_cases_on_device_and_host_inputs(golden, cname, mode):
  case = qc.all_cases()[cname]()
  skipna = qc.MODES[mode]
  before = {k: a.copy() for k, (_, a) in case['vars'].items()}
  on_device = cpu.to_lite(case, device=True)
  res = cpu.run_product(case, on_device, skipna)
  cpu.check_against_fixture(res, case, cname, mode, golden, device=True)
  for name in case['vars']:
    if qc.reduced_axes(case, name):
      qn.assert_bit_equal(res[name + case['name_suffix']].values,
                          cpu.restated(case, name, skipna), name)
  for k, da in on_device.data_vars.items():  # inputs are never modified
    assert da.data.cpu().numpy().tobytes() == before[k].tobytes()
  host = cpu.run_product(case, cpu.to_lite(case), skipna)
  cpu.check_against_fixture(host, case, cname, mode, golden)
  for k, (_, a) in case['vars'].items():
    assert a.tobytes() == before[k].tobytes()


def test_data_array_scalar_and_all_dims_on_device():
  import torch
  from weatherbench2_amd import quantiles
  from weatherbench2_amd import xarray_lite as xl
  case = qc.all_cases()['leading_f32']()
  dims, array = case['vars']['temperature']
  da = xl.DataArray(torch.from_numpy(array).cuda(), dims, dict(case['coords']))
  one = quantiles.quantile(da, 0.3, 'time')
  assert one.dims == ('latitude', 'longitude') and one.data.is_cuda
  assert one.coords['quantile'].dims == ()
  qn.assert_bit_equal(one.values, qn.quantile(array, [0.3], 0, True)[0])
  every = quantiles.quantile(da, [0.3, 0.8])  # every dim: one long series
  assert every.dims == ('quantile',)
  qn.assert_bit_equal(every.values,
                      qn.quantile(array, [0.3, 0.8], (0, 1, 2), True))


# ---------------------------------------------------------------------------
# the C ABI over the sizes at which the kernels change path
# ---------------------------------------------------------------------------
def _red_sizes(dtype):
  m = _geometry(dtype)['max_resident']
  return [1, 2, 3, 5, 63, 64, 65, m - 1, m, m + 1, 2 * m + 3]


def _inner_sizes(dtype):
  p = _geometry(dtype)['tile_points']
  return [1, 3, p - 1, p, p + 1, 2 * p + 5]


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_c_abi_over_series_lengths_tiles_and_outer_counts(dtype, skipna):
  import torch
  geo = _geometry(dtype)
  assert len(Q) > geo['targets_per_pass']
  seed = 0
  for n_red in _red_sizes(dtype):
    for n_inner in _inner_sizes(dtype):
      for n_outer in (1, 3):
        seed += 1
        host = _series((n_outer, n_red, n_inner), dtype, seed)
        got = _select(torch.from_numpy(host).cuda(), Q, skipna)
        qn.assert_bit_equal(got, qn.quantile(host, Q, 1, skipna),
                            f'n_red={n_red} n_inner={n_inner} '
                            f'n_outer={n_outer}')


@pytest.mark.parametrize('dtype,n_inner', [(np.float32, 3), (np.float32, 4),
                                           (np.float64, 3)])
def test_c_abi_outer_indices_beyond_one_grid_row(dtype, n_inner):
  """One outer index more than the 32768 of a grid row
  (csrc/launch_common.hpp; the quantile geometry call does not report it): the
  last one lies in the second grid plane.  Series of two samples of 3 points
  (narrow, with a tail) or 4 float32 points (one 16-byte lane); every outer
  index holds its own random data, so a plane that reads or writes the series
  of plane 0 is caught.  (The resident kernel: a streaming series over this
  many outer indices would be a gigabyte.)"""
  import torch
  n_outer = 32769
  host = _series((n_outer, 2, n_inner), dtype, n_inner)
  for skipna in (False, True):
    got = _select(torch.from_numpy(host).cuda(), Q, skipna)
    want = qn.quantile(host, Q, 1, skipna)
    for o in (0, 32767, 32768, n_outer - 1):
      qn.assert_bit_equal(got[:, o], want[:, o], f'outer index {o}')
    qn.assert_bit_equal(got, want, 'every outer index')


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_c_abi_long_streaming_series(dtype, skipna):
  import torch
  assert 20000 > _geometry(dtype)['max_resident']
  host = _series((1, 20000, 37), dtype, 77)
  got = _select(torch.from_numpy(host).cuda(), Q, skipna)
  qn.assert_bit_equal(got, qn.quantile(host, Q, 1, skipna), 'n_red=20000')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_c_abi_base_offset_by_one_element(dtype):
  """A buffer that starts one element past a 16-byte boundary admits no
  16-byte load, whatever n_inner is; the aligned tensor of the same values
  takes them.  Both regimes."""
  import torch
  geo = _geometry(dtype)
  p, m = geo['tile_points'], geo['max_resident']
  for n_red in (7, 66, m + 2):
    for n_inner in (p, 2 * p, 4, 2 * p + 4):
      host = _series((2, n_red, n_inner), dtype, n_red + n_inner)
      buf = torch.empty(host.size + 1, dtype=_torch_dtype(dtype), device='cuda')
      assert buf.data_ptr() % 16 == 0
      buf[1:] = torch.from_numpy(host).cuda().reshape(-1)
      view = buf[1:].view(host.shape)
      assert view.data_ptr() % 16 != 0 and view.is_contiguous()
      want = qn.quantile(host, Q, 1, True)
      qn.assert_bit_equal(_select(view, Q, True), want, 'offset')
      qn.assert_bit_equal(_select(torch.from_numpy(host).cuda(), Q, True),
                          want, 'aligned')


def test_more_quantiles_than_one_launch_holds():
  """The kernel arguments hold 64 quantiles: 150 are served in groups."""
  import torch
  rs = np.random.RandomState(5)
  q = rs.random_sample(150).tolist()
  for n_red in (33, _geometry(np.float32)['max_resident'] + 1):
    host = _series((2, n_red, 21), np.float32, 5)
    got = _select(torch.from_numpy(host).cuda(), q, True)
    qn.assert_bit_equal(got, qn.quantile(host, q, 1, True), f'n_red={n_red}')


# ---------------------------------------------------------------------------
# the slab table
# ---------------------------------------------------------------------------
def test_views_and_gathers_are_read_in_place(monkeypatch):
  """A time-sliced view and a SlabGather reach the kernel as the resident
  tensor's own pointer with a slab table: no copy of the input is made."""
  import torch
  from weatherbench2_amd import engine, quantiles
  from weatherbench2_amd import xarray_lite as xl
  dims = ('member', 'time', 'latitude', 'longitude')
  sizes = {'member': 2, 'time': 23, 'latitude': 5, 'longitude': 12}
  host = _series((2, 23, 60), np.float32, 9).reshape(2, 23, 5, 12)
  full = torch.from_numpy(host).cuda()
  calls = []
  real = engine.quantile_select

  def spy(x, slab, *a, **k):
    calls.append((x.data_ptr(), None if slab is None
                  else slab.cpu().numpy().copy()))
    return real(x, slab, *a, **k)
  monkeypatch.setattr(engine, 'quantile_select', spy)
  copies = []
  real_c = torch.Tensor.contiguous
  monkeypatch.setattr(torch.Tensor, 'contiguous',
                      lambda self, *a, **k: (copies.append(self.is_contiguous()),
                                             real_c(self, *a, **k))[1])
  q = [0.1, 0.5, 0.9]
  # the contiguous tensor: no table at all
  ds = xl.Dataset({'t': xl.DataArray(full, dims)})
  got = quantiles.quantile(ds, q, 'time', skipna=True)
  assert calls[-1] == (full.data_ptr(), None)
  qn.assert_bit_equal(got['t'].values, qn.quantile(host, q, 1, True), 'whole')
  # every other time, from the second one
  view = full[:, 1::2]
  assert not view.is_contiguous()
  ds = xl.Dataset({'t': xl.DataArray(view, dims)})
  got = quantiles.quantile(ds, q, 'time', skipna=True)
  assert all(copies)  # .contiguous() only ever met contiguous tensors
  ptr, table = calls[-1]
  assert ptr == view.data_ptr() != full.data_ptr()
  n_half = view.shape[1]
  assert np.array_equal(table, (np.arange(2)[:, None] * 23
                                + 2 * np.arange(n_half)[None, :]).ravel())
  qn.assert_bit_equal(got['t'].values,
                      qn.quantile(host[:, 1::2], q, 1, True), 'sliced view')
  # two adjacent reduced dims of a view: still a table
  got = quantiles.quantile(ds, q, ['member', 'time'], skipna=False)
  assert calls[-1][0] == view.data_ptr() and all(copies)
  qn.assert_bit_equal(got['t'].values,
                      qn.quantile(host[:, 1::2], q, (0, 1), False), 'two dims')
  # a gather: the slabs of a resident base picked in another order
  base = full.reshape(-1, sizes['latitude'], sizes['longitude'])
  rs = np.random.RandomState(2)
  index = np.stack([rs.permutation(23)[:19] + t * 23 for t in (1, 0, 1)])
  picked = host.reshape((-1,) + host.shape[2:])[index]
  materialized = []
  real_m = xl.SlabGather.materialize
  monkeypatch.setattr(xl.SlabGather, 'materialize',
                      lambda self, *a, **k: (materialized.append(1),
                                             real_m(self, *a, **k))[1])
  ds = xl.Dataset({'t': xl.DataArray(xl.SlabGather(base, index), dims)})
  got = quantiles.quantile(ds, q, 'time', skipna=True)
  assert not materialized and all(copies)
  ptr, table = calls[-1]
  assert ptr == base.data_ptr()
  assert np.array_equal(table, index.ravel())
  assert got['t'].data.is_cuda
  qn.assert_bit_equal(got['t'].values, qn.quantile(picked, q, 1, True),
                      'gather')
  # the input is unchanged (bytes: it holds NaNs)
  assert full.cpu().numpy().tobytes() == host.tobytes()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_permuted_samples_through_the_table_alone(dtype):
  """The order of the samples cannot matter: a random permutation of the
  sample axis, given through the table, returns the bytes of the identity.
  Both regimes."""
  import torch
  m = _geometry(dtype)['max_resident']
  rs = np.random.RandomState(3)
  for n_red in (50, m + 5):
    host = _series((3, n_red, 21), dtype, n_red)
    x = torch.from_numpy(host).cuda()
    identity = np.arange(3 * n_red).reshape(3, n_red)
    perm = np.stack([row[rs.permutation(n_red)] for row in identity])
    for skipna in (False, True):
      plain = _select(x, Q, skipna)
      assert _select(x, Q, skipna, identity).tobytes() == plain.tobytes()
      assert _select(x, Q, skipna, perm).tobytes() == plain.tobytes()
      qn.assert_bit_equal(plain, qn.quantile(host, Q, 1, skipna), 'plain')
    # outer indices swapped through the table: the outputs swap
    swapped = _select(x, Q, True, identity[::-1])
    assert swapped.tobytes() == _select(x, Q, True)[:, ::-1].tobytes()


# ---------------------------------------------------------------------------
# isolation between the points of a tile
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_nan_or_inf_stays_in_its_point(dtype):
  """A NaN (skipna off) or an inf in one point changes no other point of the
  tile or of the next tile, at tile edges too.  Both regimes."""
  import torch
  geo = _geometry(dtype)
  p, m = geo['tile_points'], geo['max_resident']
  n_inner = 2 * p + 3
  for n_red in (29, m + 1):
    rs = np.random.RandomState(n_red)
    host = (rs.standard_normal((2, n_red, n_inner)) * 5).astype(dtype)
    base = _select(torch.from_numpy(host).cuda(), Q, False)
    assert not np.isnan(base).any()
    for point in (0, p - 1, p, 2 * p - 1, 2 * p, n_inner - 1):
      others = np.arange(n_inner) != point
      for value in (np.nan, np.inf, -np.inf):
        poked = host.copy()
        poked[1, n_red // 2, point] = value
        got = _select(torch.from_numpy(poked).cuda(), Q, False)
        assert got[:, 0].tobytes() == base[:, 0].tobytes()
        assert got[:, 1][:, others].tobytes() == base[:, 1][:, others].tobytes()
        qn.assert_bit_equal(got, qn.quantile(poked, Q, 1, False),
                            f'{value} at {point}')
        if np.isnan(value):
          assert np.isnan(got[:, 1, point]).all()


# ---------------------------------------------------------------------------
# end to end: the climatology of thresholds.QuantileThreshold
# ---------------------------------------------------------------------------
def test_quantile_threshold_from_device_quantiles():
  from weatherbench2_amd import quantiles, thresholds
  climatology, truth, want = cpu.threshold_inputs(device=True)
  host_climatology, _, _ = cpu.threshold_inputs()
  q = [0.1, 0.5, 0.9]
  clim = quantiles.compute_quantiles(climatology, q, 'sample',
                                     name_suffix='_quantile')
  assert list(clim.data_vars) == ['temperature_quantile']
  assert clim['temperature_quantile'].data.is_cuda
  assert clim['temperature_quantile'].dims == (
      'quantile', 'dayofyear', 'latitude', 'longitude')
  host = quantiles.compute_quantiles(host_climatology, q, 'sample',
                                     name_suffix='_quantile')
  got = thresholds.QuantileThreshold(clim, 0.9).compute(truth)
  ref = thresholds.QuantileThreshold(host, 0.9).compute(truth)
  assert got['temperature'].dims == ref['temperature'].dims == (
      'time', 'latitude', 'longitude')
  qn.assert_bit_equal(got['temperature'].values, ref['temperature'].values)
  qn.assert_bit_equal(got['temperature'].values, want)
