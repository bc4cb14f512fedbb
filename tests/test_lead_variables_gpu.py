"""The lead-time derived variables on the GPU (csrc/derived_lead.hip): every
fixture case bit for bit against the NumPy restatement and within the
reordering bound of the reference's fixture, the kernel's window counts and
geometry, views and gathers read in place, NaN windows, the clamp, and
`evaluate_chunks` / `_evaluate_all_metrics` on chunks that hold the whole lead
axis.  Reference: weatherbench2/derived_variables.py:471-528, 685-720."""
import dataclasses
import os

import numpy as np
import pytest

from tests import helpers, official_chunks as oc
from tests import lead_cases as lc
from tests import lead_np
from tests.test_lead_variables_cpu import check_against_reference

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LEAD = lc.LEAD


@pytest.fixture(scope='module')
def golden():
  return lc.load_golden(GOLDEN_DIR)


def _dataset(variables, coords, device=True):
  import torch
  from weatherbench2_amd import xarray_lite as xl
  return xl.Dataset(
      {k: xl.DataArray(torch.from_numpy(np.ascontiguousarray(a)).cuda()
                       if device else a, d) for k, (d, a) in variables.items()},
      dict(coords))


def _make(label):
  from weatherbench2_amd import derived_variables as dv
  name, kwargs = lc.CLASSES[label]
  return getattr(dv, name)(**kwargs)


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


# ---------------------------------------------------------------------------
# every fixture case through `compute`
# ---------------------------------------------------------------------------
def test_the_classes_are_importable():
  from weatherbench2_amd.derived_variables import (  # noqa: F401
      AggregatePrecipitationAccumulation, LEAD_VARIABLE_DICT,
      PrecipitationAccumulation, REFERENCE_DERIVED_VARIABLES)


@pytest.mark.parametrize('device', [True, False], ids=['device', 'host'])
def test_known_answers_of_the_reference(golden, device):
  for label, known in lc.KNOWN_ANSWERS.items():
    res = _make(label).compute(_dataset(known['vars'], known['coords'],
                                        device))
    got = res.values
    assert res.dims == (LEAD,) and sorted(res.coords) == [LEAD]
    _bit_equal(got, golden[f'known/{label}/ref'], label)
    _bit_equal(got, known['expected'].astype(np.float64), label)


@pytest.mark.parametrize('device', [True, False], ids=['device', 'host'])
@pytest.mark.parametrize('cname', list(lc.cases()))
def test_classes_against_the_restatement_and_the_reference(golden, cname,
                                                          device):
  """Bit-equal to tests/lead_np.py; within 2 w u sum_window |term| of the
  reference's fixture (bit-equal where w = 1), NaN and infinities in the same
  places; dtype, dims order and coordinates as recorded; a device result for
  device inputs, a NumPy one for host inputs; the inputs unchanged."""
  import torch
  case = lc.cases()[cname]()
  ds = _dataset(case['vars'], case['coords'], device)
  before = {k: np.array(a, copy=True) for k, (_, a) in case['vars'].items()}
  for label in case['labels']:
    key = f'{cname}/{label}'
    name, fields = lc.fields_of(label)
    res = _make(label).compute(ds)
    if device:
      assert isinstance(res.data, torch.Tensor) and res.data.is_cuda, key
    else:
      assert isinstance(res.data, np.ndarray), key
    got = np.asarray(res.values)
    dims, want, mag, w = lead_np.compute(name, fields, case['vars'],
                                         case['coords'], with_abs=True)
    ref = golden[f'{key}/ref']
    assert list(res.dims) == list(dims) == list(golden[f'{key}/dims']), key
    assert sorted(res.coords) == list(golden[f'{key}/coords']), key
    assert got.dtype == ref.dtype, key
    _bit_equal(got, want, key)
    ratio = check_against_reference(got, ref, mag, w, key)
    print(f'RATIO {key}: w = {w}, max |hip - reference| / bound = {ratio:.3f}')
  for k, v in ds.data_vars.items():
    now = v.data.cpu().numpy() if device else v.data
    assert now.tobytes() == before[k].tobytes(), (cname, k)


# ---------------------------------------------------------------------------
# the kernel: window counts, point counts, alignment
# ---------------------------------------------------------------------------
def _series(shape, dtype, seed):
  """Cumulative series along axis 1 with negative steps mixed in."""
  rs = np.random.RandomState(seed)
  steps = rs.gamma(0.5, 4e-3, size=shape)
  steps = np.where(rs.random_sample(shape) < 0.4,
                   -1e-3 * rs.random_sample(shape), steps)
  return np.cumsum(steps, axis=1).astype(dtype)


def _launch(mode, x, w, clamp=False, slab=None, sizes=None):
  from weatherbench2_amd import engine
  n_outer, n_lead, n_point = sizes if sizes is not None else x.shape
  out = engine.derived_lead_window(mode, x, slab, n_outer, n_lead, n_point, w,
                                   clamp)
  assert tuple(out.shape) == (n_outer, n_lead, n_point)
  return out.cpu().numpy()


def _expect(mode, host, w, clamp=False):
  if mode == 'diff_sum':
    return lead_np.precipitation_accumulation(host, 1, w, clamp)
  return lead_np.rolling_sum(host, 1, w)


@pytest.mark.parametrize('mode', ['diff_sum', 'sum'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_window_counts(dtype, mode):
  """Every instantiated window count, three without an instantiation (3, 5,
  7), and w = n_lead - 1, n_lead and beyond it; the clamp on and off."""
  import torch
  from weatherbench2_amd import engine
  tile, ahead, windows = engine.lead_geometry(_torch_dtype(dtype), True)
  assert set(windows) >= {1, 2, 4, 6, 8, 24} and ahead >= 1
  assert not {3, 5, 7} & set(windows)
  n_lead = 30
  width = 4 if dtype == np.float32 else 2
  for n_point in (3 * width, 3 * width + 1):  # the 16-byte and the narrow path
    host = _series((2, n_lead, n_point), dtype, n_point)
    x = torch.from_numpy(host).cuda()
    for w in sorted(set(windows) | {3, 5, 7, n_lead - 1, n_lead, n_lead + 5}):
      for clamp in (True, False):
        got = _launch(mode, x, w, clamp)
        _bit_equal(got, _expect(mode, host, w, clamp), (mode, w, clamp))
      first = w if mode == 'diff_sum' else w - 1
      assert np.isnan(got[:, :first]).all()
      assert np.isfinite(got[:, first:]).all()
    assert np.array_equal(x.cpu().numpy(), host)
  if mode == 'diff_sum':  # the clamp has something to do
    free = _expect(mode, host, 1, False)
    assert (free[:, 1:] < 0).sum() > 10
    assert not (_launch(mode, x, 1, True)[:, 1:] < 0).any()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_point_counts_around_the_vector_and_the_tile(dtype):
  """n_point = 1, VEC - 1, VEC + 1, one below and above the workgroup tile of
  both paths, a row length that rules out 16-byte loads, lead counts around
  the in-flight depth; a ring window and one that re-reads."""
  import torch
  from weatherbench2_amd import engine
  width = 4 if dtype == np.float32 else 2
  tilew, ahead, _ = engine.lead_geometry(_torch_dtype(dtype), True)
  tile1, _, _ = engine.lead_geometry(_torch_dtype(dtype), False)
  assert (tile1, tilew) == (256, 256 * width)
  seed = 0
  for n_point in (1, width - 1, width, width + 1, tile1 - 1, tile1 + 1,
                  tilew - width, tilew, tilew + width, tilew - 1, tilew + 1,
                  2 * tilew + width + 1):
    if n_point < 1:
      continue
    for n_lead in (9, ahead - 1, ahead, ahead + 1):
      seed += 1
      host = _series((2, max(n_lead, 1), n_point), dtype, seed)
      x = torch.from_numpy(host).cuda()
      for mode, w in (('diff_sum', 4), ('sum', 2), ('diff_sum', 3),
                      ('sum', 24)):
        _bit_equal(_launch(mode, x, w, True), _expect(mode, host, w, True),
                   (n_point, n_lead, mode, w))


@pytest.mark.parametrize('dtype,n_point', [(np.float32, 3), (np.float32, 4),
                                           (np.float64, 3)])
def test_outer_indices_beyond_one_grid_row(dtype, n_point):
  """One outer index more than the 32768 of a grid row
  (csrc/launch_common.hpp; the lead geometry call does not report it): the last
  one lies in the second grid plane.  Two leads of 3 points (narrow, with a
  tail) or 4 float32 points (one 16-byte lane) through two ring windows, three
  leads through a window that re-reads; every outer index holds its own random
  series, so a plane that reads or writes the series of plane 0 is caught."""
  import torch
  n_outer = 32769
  for n_lead, launches in ((2, (('diff_sum', 1), ('sum', 2))),
                           (3, (('sum', 3), ('diff_sum', 2)))):
    host = _series((n_outer, n_lead, n_point), dtype, n_point + n_lead)
    x = torch.from_numpy(host).cuda()
    for mode, w in launches:
      got = _launch(mode, x, w, True)
      want = _expect(mode, host, w, True)
      assert np.isfinite(want[:, -1]).all()
      for o in (0, 32767, 32768, n_outer - 1):
        _bit_equal(got[o], want[o], (mode, w, o))
      _bit_equal(got, want, (mode, w))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_base_misaligned_by_slicing(dtype):
  """A field that starts one element into its buffer is 4- or 8-byte aligned
  only: the narrow path, whatever the row length."""
  import torch
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import xarray_lite as xl
  host = _series((3, 13, 16), dtype, 5)
  buf = torch.empty(host.size + 1, dtype=_torch_dtype(dtype), device='cuda')
  buf[1:] = torch.from_numpy(host).cuda().reshape(-1)
  view = buf[1:].view(host.shape)
  assert view.data_ptr() % 16 != 0 and view.is_contiguous()
  for mode, w in (('diff_sum', 4), ('sum', 4), ('sum', 5)):
    _bit_equal(_launch(mode, view, w, True), _expect(mode, host, w, True),
               (mode, w))
  lead = (np.arange(13) * np.timedelta64(6, 'h')).astype('timedelta64[ns]')
  ds = xl.Dataset({'total_precipitation': xl.DataArray(
      view, ('time', LEAD, 'cell'))}, {LEAD: lead})
  res = dv.LEAD_VARIABLE_DICT['total_precipitation_24hr'].compute(ds)
  _bit_equal(res.values, _expect('diff_sum', host, 4, True), 'compute')


def test_views_and_gathers_are_read_in_place(monkeypatch):
  """A lead-sliced view (tp[:, ::2]) and a gathered lead order reach the
  kernel as the view's own pointer with a slab table that is not the
  identity: no copy of the input is made."""
  import torch
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import engine
  from weatherbench2_amd import xarray_lite as xl
  dims = ('time', LEAD, 'latitude', 'longitude')
  sizes = {'time': 3, LEAD: 17, 'latitude': 9, 'longitude': 16}
  host = _series(tuple(sizes[d] for d in dims), np.float32, 9)
  full = torch.from_numpy(host).cuda()
  lead6 = (np.arange(17) * np.timedelta64(6, 'h')).astype('timedelta64[ns]')
  calls = []
  real = engine.derived_lead_window

  def spy(mode, x, slab, *a, **k):
    calls.append((x.data_ptr(), None if slab is None
                  else slab.cpu().numpy().copy()))
    return real(mode, x, slab, *a, **k)
  monkeypatch.setattr(engine, 'derived_lead_window', spy)
  copies = []
  real_c = torch.Tensor.contiguous
  monkeypatch.setattr(torch.Tensor, 'contiguous',
                      lambda self, *a, **k: (copies.append(self.is_contiguous()),
                                             real_c(self, *a, **k))[1])
  tp24 = dv.PrecipitationAccumulation('total_precipitation', 24)
  # every other lead: 12-hourly, a window of two
  view = full[:, ::2]
  assert not view.is_contiguous()
  ds = xl.Dataset({'total_precipitation': xl.DataArray(view, dims)},
                  {LEAD: lead6[::2]})
  got = tp24.compute_on_device(ds)
  assert all(copies)  # .contiguous() only ever met contiguous tensors
  ptr, table = calls[-1]
  assert ptr == view.data_ptr() == full.data_ptr()
  n_half = view.shape[1]
  assert table is not None and table.size == 3 * n_half
  assert not np.array_equal(table, np.arange(table.size))
  assert np.array_equal(table, (np.arange(3)[:, None] * 17
                                + 2 * np.arange(n_half)[None, :]).ravel())
  want = lead_np.precipitation_accumulation(host[:, ::2], 1, 2, True)
  _bit_equal(got.values, want, 'lead-sliced view')
  # a view that starts at the second lead and the second time
  view = full[1:, 1::3]
  ds = xl.Dataset({'total_precipitation': xl.DataArray(view, dims)},
                  {LEAD: lead6[1::3]})
  got = dv.PrecipitationAccumulation('total_precipitation', 36
                                     ).compute_on_device(ds)
  assert calls[-1][0] == view.data_ptr() != full.data_ptr()
  want = lead_np.precipitation_accumulation(host[1:, 1::3], 1, 2, True)
  _bit_equal(got.values, want, 'offset view')
  # a gather: the leads of a resident base picked in another order
  base = full.reshape(-1, sizes['latitude'], sizes['longitude'])
  rs = np.random.RandomState(2)
  index = np.stack([rs.permutation(17) + t * 17 for t in (2, 0)])
  picked = host.reshape((-1,) + host.shape[2:])[index]
  materialized = []
  real_m = xl.SlabGather.materialize
  monkeypatch.setattr(xl.SlabGather, 'materialize',
                      lambda self, *a, **k: (materialized.append(1),
                                             real_m(self, *a, **k))[1])
  ds = xl.Dataset({'total_precipitation_6hr': xl.DataArray(
      xl.SlabGather(base, index), dims)}, {LEAD: lead6})
  got = dv.AggregatePrecipitationAccumulation(24).compute_on_device(ds)
  assert not materialized and all(copies)
  ptr, table = calls[-1]
  assert ptr == base.data_ptr()
  assert np.array_equal(table, index.ravel())
  _bit_equal(got.values, lead_np.rolling_sum(picked, 1, 4), 'gather')
  assert np.array_equal(full.cpu().numpy(), host)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_nan_reaches_exactly_the_windows_that_see_it(dtype):
  """A NaN at lead k: NaN for the w outputs that see it (w + 1 for the
  difference mode, where leads k and k + 1 both form a NaN term), finite
  values before and after."""
  import torch
  n_lead, k = 40, 9
  host = _series((2, n_lead, 8), dtype, 3)
  host[:, k] = np.nan
  x = torch.from_numpy(host).cuda()
  for w in (1, 2, 4, 6, 8, 24, 3, 5):
    got = _launch('sum', x, w)
    nan = np.isnan(got).all(axis=(0, 2))
    assert np.array_equal(np.isnan(got).any(axis=(0, 2)), nan)
    want = np.zeros(n_lead, bool)
    want[:w - 1] = True
    want[k:k + w] = True
    assert np.array_equal(nan, want), ('sum', w)
    got = _launch('diff_sum', x, w, True)
    nan = np.isnan(got).all(axis=(0, 2))
    assert np.array_equal(np.isnan(got).any(axis=(0, 2)), nan)
    want = np.zeros(n_lead, bool)
    want[:w] = True
    want[k:k + w + 1] = True
    assert np.array_equal(nan, want), ('diff_sum', w)
    _bit_equal(got, _expect('diff_sum', host, w, True), w)


def test_clamp_keeps_nan_and_negative_zero():
  import torch
  host = np.array([[0.0, 1.0, 0.5, 0.5, np.nan, 2.0, 2.0, -0.0, -0.0]],
                  dtype=np.float32).reshape(1, 9, 1)
  host[0, 7:, 0] = -0.0
  x = torch.from_numpy(host).cuda()
  on = _launch('diff_sum', x, 1, True)[0, :, 0]
  off = _launch('diff_sum', x, 1, False)[0, :, 0]
  assert np.isnan(on[[0, 4, 5]]).all() and np.isnan(off[[0, 4, 5]]).all()
  assert on[2] == 0 and not np.signbit(on[2]) and off[2] == -0.5
  assert on[3] == 0 and off[3] == 0
  # 2.0 -> -0.0 is -2.0 (clamped); -0.0 - -0.0 is +0.0 in round-to-nearest
  assert on[7] == 0 and off[7] == -2.0
  _bit_equal(on.reshape(1, 9, 1), _expect('diff_sum', host, 1, True), 'on')
  _bit_equal(off.reshape(1, 9, 1), _expect('diff_sum', host, 1, False), 'off')


def test_xarray_lite_protocol_and_errors():
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import xarray_lite as xl
  case = lc.cases()['latlon_time']()
  ds = _dataset(case['vars'], case['coords'])
  res = dv.LEAD_VARIABLE_DICT['total_precipitation_24hr'].compute(ds)
  assert isinstance(res, xl.DataArray)
  assert res.dims == ('time', LEAD, 'latitude', 'longitude')
  assert sorted(res.coords) == ['latitude', 'longitude', LEAD, 'time']
  short = ds.isel(**{LEAD: slice(0, 1)})
  with pytest.raises(ValueError, match=LEAD):
    dv.LEAD_VARIABLE_DICT['total_precipitation_24hr'].compute(short)
  # the aggregate does not look at the lead coordinate: one lead is all NaN
  one = dv.LEAD_VARIABLE_DICT['total_precipitation_24hr_from_6hr'].compute(
      short)
  assert one.shape == (2, 1, 9, 16) and np.isnan(one.values).all()
  empty = ds.isel(time=slice(0, 0))
  res = dv.LEAD_VARIABLE_DICT['total_precipitation_6hr'].compute(empty)
  assert res.shape == (0, 13, 9, 16)


# ---------------------------------------------------------------------------
# the drivers on chunks that hold the whole lead axis
# ---------------------------------------------------------------------------
NAME = 'total_precipitation_24hr'


def _official(n_init=5, n_lead=9, n_lat=19, n_lon=36, seed=0):
  """(forecast, truth by time, truth at valid time) as oracle DS: cumulative
  precipitation and a temperature, by init time, 6-hourly leads."""
  from oracle import evaluation_np as oe
  from oracle.named import DS, NA
  rs = np.random.RandomState(seed)
  lat = np.linspace(-90, 90, n_lat)
  lon = np.linspace(0, 360, n_lon, endpoint=False)
  init = (np.datetime64('2020-01-01T00', 'ns') +
          np.arange(n_init) * np.timedelta64(12, 'h'))
  lead = (np.arange(n_lead) * np.timedelta64(6, 'h')).astype('timedelta64[ns]')
  n_time = 2 * n_init + n_lead
  time = (np.datetime64('2020-01-01T00', 'ns') +
          np.arange(n_time) * np.timedelta64(6, 'h'))

  def fields(outer):
    shape = outer + (n_lat, n_lon)
    steps = rs.gamma(0.5, 4e-3, size=shape)
    steps = np.where(rs.random_sample(shape) < 0.3,
                     -2e-5 * rs.random_sample(shape), steps)
    return {'total_precipitation':
                np.cumsum(steps, axis=len(outer) - 1).astype(np.float32),
            '2m_temperature':
                (280 + 5 * rs.standard_normal(shape)).astype(np.float32)}
  fcoords = {'init_time': init, 'lead_time': lead, 'latitude': lat,
             'longitude': lon,
             'valid_time': NA(init[:, None] + lead[None, :],
                              ('init_time', 'lead_time'))}
  d2 = ('init_time', 'lead_time', 'latitude', 'longitude')
  forecast = DS({k: NA(a, d2) for k, a in fields((n_init, n_lead)).items()},
                fcoords)
  tcoords = {'time': time, 'latitude': lat, 'longitude': lon}
  truth = DS({k: NA(a, ('time', 'latitude', 'longitude'))
              for k, a in fields((n_time,)).items()}, tcoords)
  return forecast, truth, oe.truth_at_valid_time(truth, forecast)


def _variable():
  from weatherbench2_amd import derived_variables as dv
  return dv.PrecipitationAccumulation(
      total_precipitation_name='total_precipitation', accumulation_hours=24,
      lead_time_name='lead_time')


def _eval_setup(**kw):
  from weatherbench2_amd import config, evaluation, metrics as gm
  forecast, truth_by_time, truth = _official(**kw)
  regions = {'global': helpers.to_gpu_region(oc.oreg.SliceRegion()),
             'tropics': helpers.to_gpu_region(
                 oc.oreg.SliceRegion(lat_slice=slice(-20, 20)))}
  gf, gt, gtime = (evaluation.make_resident(helpers.to_gpu_dataset(x))
                   for x in (forecast, truth, truth_by_time))
  cfg = config.Eval(metrics={'mse': gm.MSE(), 'mae': gm.MAE(),
                             'bias': gm.Bias()},
                    regions=regions, derived_variables={NAME: _variable()})
  return forecast, truth, gf, gt, gtime, cfg


def _whole_lead_chunks(forecast, truth):
  n = forecast.sizes['init_time']
  return [(forecast.isel(init_time=slice(i, i + 1)),
           truth.isel(init_time=slice(i, i + 1))) for i in range(n)]


def _named(da, drop=()):
  """{dims without `drop`: float64 values} with size-one `drop` dims removed."""
  values = np.asarray(da.values, dtype=np.float64)
  dims = list(da.dims)
  for d in drop:
    if d in dims:
      assert values.shape[dims.index(d)] == 1
      values = np.take(values, 0, axis=dims.index(d))
      dims.remove(d)
  return tuple(dims), values


def _to_order(dims, values, order):
  assert sorted(dims) == sorted(order), (dims, order)
  return np.transpose(values, [dims.index(d) for d in order])


def _loop_per_chunk(forecast, truth, cfg):
  """_metric_and_region_loop over the whole-lead chunks, each fed the field
  of tests/lead_np.py as an ordinary variable: [(dims, values)] per chunk and
  variable, without the chunk's init_time."""
  import torch
  from weatherbench2_amd import evaluation
  from weatherbench2_amd import xarray_lite as xl
  plain = dataclasses.replace(cfg, derived_variables={})
  out = []
  for f, t in _whole_lead_chunks(forecast, truth):
    pair = []
    for ds in (f, t):
      ds = ds.copy()
      tp = ds['total_precipitation']
      host = tp.data.cpu().numpy()
      field = lead_np.precipitation_accumulation(
          host, tp.dims.index('lead_time'), 4, True)
      ds[NAME] = xl.DataArray(torch.from_numpy(field).cuda(), tp.dims)
      pair.append(ds)
    res = xl.as_dataset(evaluation._metric_and_region_loop(
        pair[0], pair[1], plain, False, compute_chunk=True))
    out.append({k: _named(res[k], drop=('init_time',))
                for k in res.data_vars})
  return out


@pytest.mark.parametrize('batch', [1, 3, None])
def test_evaluate_chunks_on_whole_lead_chunks(batch):
  """`evaluate_chunks` with the accumulation in `derived_variables`, over
  several init times, windowed and chunk by chunk, equals
  `_metric_and_region_loop` over the same chunks fed the NumPy field (1e-9,
  NaN leads equal) -- as a time mean and as a series."""
  from weatherbench2_amd import evaluation
  _, _, gf, gt, _, cfg = _eval_setup()
  chunks = _whole_lead_chunks(gf, gt)
  kwargs = {} if batch is None else {'batch_chunks': batch}
  want = _loop_per_chunk(gf, gt, cfg)
  got = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0, **kwargs)
  assert NAME in got.data_vars and 'total_precipitation' in got.data_vars
  assert all(NAME not in f.data_vars for f, _ in chunks)
  for name in got.data_vars:
    dims, values = _named(got[name])
    wdims = want[0][name][0]
    mean = np.mean([w[name][1] for w in want], axis=0)
    helpers.assert_close(_to_order(dims, values, wdims), mean, rtol=1e-9,
                         atol=1e-12, err_msg=name)
  dims, values = _named(got[NAME])
  nan = np.isnan(values).all(axis=tuple(a for a, d in enumerate(dims)
                                        if d != 'lead_time'))
  assert list(nan) == [True] * 4 + [False] * 5
  series = dataclasses.replace(cfg, temporal_mean=False)
  got = evaluation.evaluate_chunks(chunks, series, False, prefetch=0, **kwargs)
  for name in got.data_vars:
    dims, values = _named(got[name])
    axis = dims.index('init_time')
    assert values.shape[axis] == len(chunks)
    rest = tuple(d for d in dims if d != 'init_time')
    for i, w in enumerate(want):
      helpers.assert_close(
          _to_order(rest, np.take(values, i, axis=axis), w[name][0]),
          w[name][1], rtol=1e-9, atol=1e-12, err_msg=f'{name}[{i}]')


def test_evaluate_all_metrics_in_memory():
  """The in-memory driver hands the whole dataset to `compute`: the time mean
  of the per-chunk values."""
  from weatherbench2_amd import config, evaluation
  _, _, gf, gt, gtime, cfg = _eval_setup()
  want = _loop_per_chunk(gf, gt, cfg)
  got = evaluation._evaluate_all_metrics(
      'e', cfg, config.Data(by_init=True), False, forecast=gf, truth=gtime)
  assert NAME in got.data_vars
  for name in got.data_vars:
    dims, values = _named(got[name])
    mean = np.mean([w[name][1] for w in want], axis=0)
    helpers.assert_close(_to_order(dims, values, want[0][name][0]), mean,
                         rtol=1e-9, atol=1e-12, err_msg=name)


def test_a_single_lead_chunk_raises():
  """`init_time=1,lead_time=1` chunks cannot form the variable: the
  ValueError of `compute` surfaces unmasked."""
  from weatherbench2_amd import evaluation
  _, _, gf, gt, _, cfg = _eval_setup(n_init=2, n_lead=5)
  with pytest.raises(ValueError, match='lead_time') as info:
    evaluation.evaluate_chunks(oc.chunk_pairs(gf, gt), cfg, False, prefetch=0)
  assert 'whole lead axis in one chunk' in str(info.value)
