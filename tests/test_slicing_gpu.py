"""Dataset slicing on the GPU (K17, csrc/box_gather.hip).  Everything is
compared as bit patterns against tests/slice_np.py (`np.take`).  Before every
direct launch the output is filled with a sentinel and lies between two guard
bands, so an element that is never written, and a store outside the output,
are seen.  The inputs are random BIT patterns: NaNs with payloads, -0.0,
infinities and denormals are all among them."""
import numpy as np
import pytest

from tests import slice_cases
from tests import slice_np
from tests.test_slicing_cpu import check_against_fixture

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from weatherbench2_amd import engine  # noqa: E402
from weatherbench2_amd import operands  # noqa: E402
from weatherbench2_amd import slicing  # noqa: E402
from weatherbench2_amd import xarray_lite as xl  # noqa: E402

GUARD = 64  # elements: a multiple of 16 bytes for every dtype
N_COL_IN = (1, 3, 4, 5, 8, 63, 64, 65, 257)
N_ROW_IN = (1, 2, 5)
UINT = {4: np.uint32, 8: np.uint64}


def random_bits(rs, shape, dtype) -> np.ndarray:
  dtype = np.dtype(dtype)
  bits = rs.randint(0, 2**32, size=tuple(shape) + (dtype.itemsize // 4,),
                    dtype=np.uint64).astype(np.uint32)
  out = np.ascontiguousarray(bits).view(UINT[dtype.itemsize]).reshape(shape)
  return out.view(dtype)


def _between_guards(n: int, dtype, shift: int, fill=None):
  """(whole buffer, the n elements `GUARD + shift` in) on the device, as
  integers of the dtype's size; the guards and the rest hold a sentinel."""
  word = UINT[np.dtype(dtype).itemsize]
  sentinel = np.array([0x5a5a5a5a5a5a5a5a], np.uint64).astype(word)[0]
  host = np.full(n + 2 * GUARD + shift, sentinel, dtype=word)
  if fill is not None:
    host[GUARD + shift:GUARD + shift + n] = np.ascontiguousarray(
        fill).reshape(-1).view(word)
  whole = torch.from_numpy(host.view(np.dtype(dtype))).cuda()
  return whole, whole[GUARD + shift:GUARD + shift + n], sentinel


def launch(x: np.ndarray, src_slab=None, rows=None, cols=None, shift: int = 0,
           form=None) -> np.ndarray:
  """One K17 launch on `x` [n_slab, n_row, n_col]; `shift` moves input and
  output off 16-byte alignment by that many elements.  Checks the guard bands
  and the result against NumPy, returns the result."""
  n_slab, n_row, n_col = x.shape
  _, dev, _ = _between_guards(x.size, x.dtype, shift, x)
  listed = cols if not isinstance(cols, tuple) else slice_np.run(*cols)
  want = slice_np.box_gather(x, src_slab, rows, listed)
  whole, out, sentinel = _between_guards(want.size, x.dtype, shift)
  if form is not None:
    assert engine.box_gather_form(dev, out, n_col, cols if cols is not None
                                  else (0, 1, n_col)) == form
  got = engine.box_gather(dev.view(n_slab, n_row, n_col), n_row, n_col,
                          src_slab=src_slab, rows=rows, cols=cols,
                          out=out.view(want.shape))
  torch.cuda.synchronize()
  host = whole.cpu().numpy().view(UINT[x.dtype.itemsize])
  assert (host[:GUARD + shift] == sentinel).all(), 'store before the output'
  assert (host[GUARD + shift + want.size:] == sentinel).all(), \
      'store behind the output'
  got = got.cpu().numpy()
  assert slice_np.same_bits(got, want), (x.shape, src_slab, rows, cols)
  return got


def column_forms(rs, n: int) -> dict:
  """Every column form that fits a row of `n` columns."""
  forms = {'full': None, 'single': (n // 2, 1, 1),
           'list': rs.randint(0, n, size=n + 3)}
  for c in (0, 1, 4):
    if c < n:
      forms[f'from_{c}'] = (c, 1, n - c)
      forms[f'from_{c}_short'] = (c, 1, max(1, (n - c) // 2))
  forms['step_2'] = (0, 2, (n + 1) // 2)
  forms['step_3'] = (min(1, n - 1), 3, (n - min(1, n - 1) + 2) // 3)
  forms['reversed'] = (n - 1, -1, n)
  forms['reversed_part'] = (max(n - 2, 0), -1, max(n - 2, 0) + 1)
  if n >= 4:
    forms['reversed_aligned_part'] = (n // 4 * 4 - 1, -1, n // 4 * 4)
  forms['step_-2'] = (n - 1, -2, (n + 1) // 2)
  return forms


def row_tables(rs, n: int) -> dict:
  return {'identity': None, 'flip': np.arange(n)[::-1],
          'step_2': np.arange(0, n, 2), 'list': rs.randint(0, n, size=n + 2)}


@pytest.mark.parametrize('n_col_in', N_COL_IN)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_box_gather_every_form(dtype, n_col_in):
  rs = np.random.RandomState(n_col_in)
  for n_row_in in N_ROW_IN:
    x = random_bits(rs, (3, n_row_in, n_col_in), dtype)
    for cols in column_forms(rs, n_col_in).values():
      for rows in row_tables(rs, n_row_in).values():
        launch(x, None, rows, cols)
    launch(x, [2, 0, 0, 1], None, None)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_box_gather_specials_survive(dtype):
  info = np.finfo(dtype)
  word = UINT[np.dtype(dtype).itemsize]
  payload = np.array([0x7fc00123 if word is np.uint32
                      else 0x7ff8000000000456], dtype=word).view(dtype)[0]
  signalling = np.array([0x7f800001 if word is np.uint32
                         else 0x7ff0000000000001], dtype=word).view(dtype)[0]
  row = np.array([payload, -0.0, signalling, np.inf, -np.inf, info.tiny / 4,
                  0.0, info.max], dtype=dtype)
  x = np.tile(row, (2, 3, 1))
  for cols in (None, (7, -1, 8), (0, 2, 4), [1, 0, 2, 2]):
    got = launch(x, None, [2, 0], cols).view(word)
    # (`launch` compares every bit; these are the ones a cast would lose)
    kept = row[np.arange(8) if cols is None else slice_np.run(*cols)
               if isinstance(cols, tuple) else cols]
    for special in (payload, signalling, dtype(-0.0)):
      bits = np.array([special], dtype=dtype).view(word)[0]
      assert (got == bits).any() == (kept.view(word) == bits).any()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_box_gather_takes_the_wide_forms_only_when_aligned(dtype):
  rs = np.random.RandomState(3)
  w = 16 // np.dtype(dtype).itemsize
  x = random_bits(rs, (2, 5, 64), dtype)
  cases = {'run': (w, 1, 64 - 2 * w), 'reversed': (63, -1, 64)}
  for form, cols in cases.items():
    aligned = launch(x, None, [4, 0, 1], cols, form=form)
    shifted = launch(x, None, [4, 0, 1], cols, shift=1, form='scalar')
    assert slice_np.same_bits(aligned, shifted)
  # a run that starts or ends off a lane, a row that is no whole lanes
  launch(x, None, None, (1, 1, 63), form='scalar')
  launch(x, None, None, (0, 1, 63), form='scalar')
  launch(x, None, None, (62, -1, 60), form='scalar')
  launch(random_bits(rs, (2, 5, 63), dtype), None, None, (0, 1, 60),
         form='scalar')
  launch(x, None, None, [5, 4, 3], form='list')


@pytest.mark.parametrize('form,n_col_out', [
    ('scalar', 63), ('scalar', 64), ('scalar', 65), ('scalar', 256),
    ('scalar', 257), ('run', 64), ('run', 68), ('run', 1024), ('run', 1028),
    ('reversed', 64), ('reversed', 1028), ('list', 65)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_box_gather_tile_edges(dtype, form, n_col_out):
  """An output slab of exactly one tile of rows, one more and one less, at
  column counts on, below and above a tile's width."""
  rs = np.random.RandomState(n_col_out)
  tdtype = operands.torch_dtype(dtype)
  geo = engine.box_gather_geometry(tdtype, form, n_col_out)
  n_col_in = n_col_out + (0 if form in ('run', 'reversed') else 3)
  cols = {'scalar': (1, 1, n_col_out), 'run': (0, 1, n_col_out),
          'reversed': (n_col_out - 1, -1, n_col_out),
          'list': rs.randint(0, n_col_in, size=n_col_out)}[form]
  for n_row_out in (geo['tile_rows'] - 1, geo['tile_rows'],
                    geo['tile_rows'] + 1):
    x = random_bits(rs, (2, 7, n_col_in), dtype)
    launch(x, [1, 0, 1], rs.randint(0, 7, size=n_row_out), cols, form=form)


def test_box_gather_crosses_the_grid_row_limit():
  n = engine.box_gather_geometry(torch.float32, 'scalar', 1)[
      'max_grid_outer'] + 1
  assert n == 32769
  rs = np.random.RandomState(5)
  x = random_bits(rs, (n, 1, 1), np.float32)
  launch(x, None, None, None)
  launch(x, np.arange(n)[::-1], None, None)
  x = random_bits(rs, (n, 2, 3), np.float64)
  launch(x, rs.permutation(n), [1, 0], (2, -1, 3))


@pytest.mark.parametrize('dtype', [np.int32, np.int64])
def test_box_gather_integers_ride_the_same_instances(dtype):
  rs = np.random.RandomState(6)
  info = np.iinfo(dtype)
  x = rs.randint(info.min, info.max, size=(3, 5, 64), dtype=dtype)
  launch(x, [2, 1], [4, 0, 0], (63, -1, 64), form='reversed')
  launch(x, None, None, (8, 1, 48), form='run')
  launch(x, None, [1], (0, 3, 22), form='scalar')
  launch(x, [0, 0], None, [63, 0, 63], form='list')


# ---------------------------------------------------------------------------
# slice_dataset on device-backed datasets
# ---------------------------------------------------------------------------
class Launches:
  """Counts the launches of a block, per kernel."""

  def __enter__(self):
    self.count = {}
    self.old = engine.set_launch_hook(self)
    return self

  def __call__(self, when, kernel):
    if when == 'begin':
      self.count[kernel] = self.count.get(kernel, 0) + 1

  def __exit__(self, *exc):
    engine.set_launch_hook(self.old)


def to_numpy(data) -> np.ndarray:
  if isinstance(data, xl.SlabGather):
    data = data.materialize()
  return data.cpu().numpy() if isinstance(data, torch.Tensor) else np.asarray(
      data)


def same_datasets(a: xl.Dataset, b: xl.Dataset):
  assert list(a.data_vars) == list(b.data_vars)
  for name in a.data_vars:
    assert a[name].dims == b[name].dims, name
    assert slice_np.same_bits(to_numpy(a[name].data), to_numpy(b[name].data)), \
        name
  assert set(a.coords) == set(b.coords)
  for k in a.coords:
    np.testing.assert_array_equal(xl.coord_values(a, k), xl.coord_values(b, k))


@pytest.mark.parametrize('name', sorted(slice_cases.CASES))
def test_slice_dataset_device_matches_host_and_reference(name):
  description = slice_cases.build(name)
  options = slice_cases.options(name)
  out = slicing.slice_dataset(slice_cases.to_lite(description, 'cuda'),
                              **options)
  for v in out.data_vars.values():
    assert isinstance(v.data, torch.Tensor) and v.data.is_cuda
  check_against_fixture(out, name, values=to_numpy)
  same_datasets(out, slicing.slice_dataset(slice_cases.to_lite(description),
                                           **options))


def test_reference_case_is_one_launch_per_variable():
  """The reference test's case: a reversed latitude made increasing, a time
  range with a step, longitude_step and isel on latitude."""
  ds = slice_cases.to_lite(slice_cases.build('known_simple'), 'cuda')
  options = slice_cases.options('known_simple')
  with Launches() as launches:
    out = slicing.slice_dataset(ds, **options)
  assert launches.count == {'box_gather': 2}
  check_against_fixture(out, 'known_simple', values=to_numpy)
  with Launches() as launches:
    again = slicing.slice_dataset(ds, **options)
  assert launches.count == {'box_gather': 2}
  same_datasets(out, again)  # two runs, the same bits


def _grid_variants():
  """The same dataset four ways: contiguous, a time-sliced view of a longer
  one, a permuted view (level before time in memory) and a gather over a
  base with other slabs in between."""
  description = slice_cases.grid()
  plain = slice_cases.to_lite(description, 'cuda')
  variants = {'contiguous': plain}
  view, permuted, gathered = (xl.Dataset(coords=plain.coords) for _ in range(3))
  rs = np.random.RandomState(9)
  for name, v in plain.data_vars.items():
    data = v.data
    long = torch.zeros((2 * data.shape[0] + 1,) + tuple(data.shape[1:]),
                       dtype=data.dtype, device='cuda')
    long[1::2] = data
    view.data_vars[name] = xl.DataArray(long[1::2], v.dims, view.coords, name)
    if data.dim() == 4:
      stored = data.permute(1, 0, 2, 3).contiguous()
      permuted.data_vars[name] = xl.DataArray(stored.permute(1, 0, 2, 3),
                                              v.dims, permuted.coords, name)
    else:
      permuted.data_vars[name] = v
    outer = tuple(data.shape[:-2])
    n = int(np.prod(outer))
    index = rs.permutation(2 * n)[:n]
    base = torch.zeros((2 * n,) + tuple(data.shape[-2:]), dtype=data.dtype,
                       device='cuda')
    base[torch.as_tensor(index, device='cuda')] = data.reshape(
        (n,) + tuple(data.shape[-2:]))
    gathered.data_vars[name] = xl.DataArray(
        xl.SlabGather(base, index.reshape(outer)), v.dims, gathered.coords,
        name)
  variants.update(view=view, permuted=permuted, gathered=gathered)
  return description, variants


def test_views_permutations_and_gathers_differ_in_the_table_alone():
  description, variants = _grid_variants()
  host = slice_cases.to_lite(description)
  for options in (
      dict(sel='latitude_start=-33.33,latitude_stop=33.33', isel='time_step=5'),
      dict(isel='longitude_step=4,level_list=2+0,time_list=7+7+1'),
      dict(make_dims_increasing='latitude', isel='latitude_list=6+5+4+3+2+1+0')):
    want = slicing.slice_dataset(host, **options)
    for kind, ds in variants.items():
      with Launches() as launches:
        got = slicing.slice_dataset(ds, **options)
      assert launches.count == {'box_gather': 4}, (kind, launches.count)
      same_datasets(got, want)
  # whole slabs: K16 for the floats, and the lazy form moves nothing
  options = dict(isel='time_start=3,time_step=4,level_list=1')
  want = slicing.slice_dataset(host, **options)
  for kind, ds in variants.items():
    with Launches() as launches:
      got = slicing.slice_dataset(ds, **options)
    assert launches.count == {'slab_scatter': 3}, (kind, launches.count)
    same_datasets(got, want)
    with Launches() as launches:
      lazy = slicing.slice_dataset(ds, materialize=False, **options)
    assert launches.count == {}
    same_datasets(lazy, want)


def _torch_selection(ds: xl.Dataset, names, options) -> xl.Dataset:
  """The same selection the way a torch user writes it: one index_select per
  dim."""
  pos = slicing.compose_positions(ds, **options)
  coords = {k: (np.asarray(c)[pos[k]] if k in pos else c)
            for k, c in ds.coords.items() if not isinstance(c, xl.DataArray)}
  out = xl.Dataset(coords=coords)
  for name in names:
    v = ds[name]
    data = v.data
    for ax, d in enumerate(v.dims):
      if d in pos:
        data = torch.index_select(data, ax, torch.as_tensor(pos[d],
                                                            device='cuda'))
    out.data_vars[name] = xl.DataArray(data.contiguous(), v.dims, out.coords,
                                       name)
  return out


def test_sliced_datasets_feed_the_metrics():
  from weatherbench2_amd import metrics as gm
  description = slice_cases.grid()
  forecast = slice_cases.to_lite(description, 'cuda')
  other = slice_cases.grid(seed=11)
  truth = slice_cases.to_lite(other, 'cuda')
  names = ['t', 'sp']
  for options, lazy in (
      (dict(sel='latitude_start=-60,latitude_stop=60,longitude_start=30',
            isel='time_step=3,longitude_step=2'), False),
      (dict(isel='time_start=1,time_step=5,level_list=2+0'), True)):
    kwargs = dict(options, keep_variables=names)
    f = slicing.slice_dataset(forecast, **kwargs)
    t = slicing.slice_dataset(truth, **kwargs)
    want = gm.MSE().compute_chunk(_torch_selection(forecast, names, options),
                                  _torch_selection(truth, names, options))
    got = gm.MSE().compute_chunk(f, t)
    assert set(got.data_vars) == set(want.data_vars) == set(names)
    for name in names:
      assert got[name].dims == want[name].dims
      assert slice_np.same_bits(np.asarray(got[name].values),
                                np.asarray(want[name].values)), name
    if lazy:
      f = slicing.slice_dataset(forecast, materialize=False, **kwargs)
      assert isinstance(f['t'].data, xl.SlabGather)
      assert f['t'].data.base.data_ptr() == forecast['t'].data.data_ptr()
      got = gm.MSE().compute_chunk(f, t)
      for name in names:
        assert slice_np.same_bits(np.asarray(got[name].values),
                                  np.asarray(want[name].values)), name


def test_compute_derived_variables_with_the_defaults():
  from tests import column_cases
  from weatherbench2_amd import derived_dataset
  from weatherbench2_amd import derived_variables as dvs
  case = column_cases.cases()['era5_levels']()
  rs = np.random.RandomState(12)
  coords = dict(case['coords'])
  leads = (np.arange(9) * np.timedelta64(6, 'h')).astype('timedelta64[ns]')
  coords['prediction_timedelta'] = leads
  ds = xl.Dataset(coords=coords)
  for name, (dims, values) in case['vars'].items():
    ds.data_vars[name] = xl.DataArray(
        torch.from_numpy(np.ascontiguousarray(values)).cuda(), dims, ds.coords,
        name)
  n_lat, n_lon = coords['latitude'].size, coords['longitude'].size
  rain = np.cumsum(rs.random_sample((1, 9, n_lat, n_lon)), axis=1).astype(
      np.float32)
  ds.data_vars['total_precipitation'] = xl.DataArray(
      torch.from_numpy(rain).cuda(),
      ('time', 'prediction_timedelta', 'latitude', 'longitude'), ds.coords,
      'total_precipitation')
  before = list(ds.data_vars)
  out = derived_dataset.compute_derived_variables(ds)
  names = list(derived_dataset.DEFAULT_DERIVED_VARIABLES)
  assert list(out.data_vars) == before + names
  for name in before:
    assert out[name].data is ds[name].data
  for name in names:
    want = dvs.REFERENCE_DERIVED_VARIABLES[name].compute(ds)
    assert out[name].dims == want.dims, name
    assert isinstance(out[name].data, torch.Tensor) and out[name].data.is_cuda
    assert slice_np.same_bits(to_numpy(out[name].data), to_numpy(want.data)), \
        name
