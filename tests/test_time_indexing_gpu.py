"""Time re-indexing on the GPU (K16, csrc/slab_scatter.hip).  Everything is
compared as bit patterns against tests/time_indexing_np.py.  Before every
launch the output is filled with a sentinel and lies between two guard bands,
so a slab that is never written, and a store outside the output, are seen.
A slab written twice with the same value is not: that the destinations are
disjoint is `engine.scatter_csr`'s check on the host
(tests/test_time_indexing_cpu.py), and every source here holds other values,
so a destination that received a second, wrong source shows."""
import numpy as np
import pytest

from tests import time_indexing_cases as tc
from tests import time_indexing_np as tn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from weatherbench2_amd import engine  # noqa: E402
from weatherbench2_amd import operands  # noqa: E402
from weatherbench2_amd import time_indexing as ti  # noqa: E402
from weatherbench2_amd import xarray_lite as xl  # noqa: E402

DELTA = 'prediction_timedelta'
GUARD = 64  # elements: a multiple of 16 bytes for both dtypes
SENTINEL = 12345.0
PAIRS = {'f32': (np.float32, np.float32), 'f64': (np.float64, np.float64),
         'f64_f32': (np.float64, np.float32)}
DESTS_PER_GROUP = (1, 4, 64)


@pytest.fixture(scope='module')
def golden():
  out = tc.load_golden()
  assert out
  return out


def _between_guards(n: int, dtype, shift: int, fill=None):
  """(whole buffer, the n elements `GUARD + shift` in) on the device."""
  whole = torch.full((n + 2 * GUARD + shift,), SENTINEL,
                     dtype=operands.torch_dtype(dtype), device='cuda')
  inner = whole[GUARD + shift:GUARD + shift + n]
  if fill is not None:
    inner.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))
  return whole, inner


def launch(flat: np.ndarray, src, dst_lists, n_out: int, out_dtype,
           dests_per_group: int, shift: int = 0) -> np.ndarray:
  """One K16 launch on `flat` [n_in_slab, n_point]; `shift` moves input and
  output off 16-byte alignment by that many elements.  Returns the output
  after checking the guard bands."""
  n_in, n_point = flat.shape
  _, x = _between_guards(flat.size, flat.dtype, shift, flat)
  whole, out = _between_guards(n_out * n_point, out_dtype, shift)
  assert (x.data_ptr() % 16 == 0) == (shift * flat.itemsize % 16 == 0)
  got = engine.slab_scatter(
      x.view(n_in, n_point), src, dst_lists, n_out, n_point=n_point,
      out_dtype=operands.torch_dtype(out_dtype),
      dests_per_group=dests_per_group, out=out.view(n_out, n_point))
  torch.cuda.synchronize()
  host = whole.cpu().numpy()
  assert (host[:GUARD + shift] == SENTINEL).all(), 'store before the output'
  assert (host[GUARD + shift + n_out * n_point:] == SENTINEL).all(), \
      'store behind the output'
  return got.cpu().numpy()


def table_of(src, dst_lists, n_out: int) -> np.ndarray:
  table = np.full(n_out, -2, dtype=np.int64)
  for s, dests in zip(src, dst_lists):
    table[np.asarray(dests, dtype=np.int64)] = s
  assert (table >= -1).all()
  return table


def scattered_problem(rs, counts, n_in_slab: int, with_hole: int = 2):
  """Sources with `counts` destinations each, drawn without repeats from
  `n_in_slab` input slabs, and a -1 source with `with_hole` destinations; the
  destinations are a random permutation of the output slabs."""
  n_out = int(sum(counts)) + with_hole
  dests = rs.permutation(n_out)
  src = rs.permutation(n_in_slab)[:len(counts)].tolist()
  lists, at = [], 0
  for c in counts:
    lists.append(np.sort(dests[at:at + c]))
    at += c
  if with_hole:
    where = len(counts) // 2  # (among the others, not at an end)
    src.insert(where, -1)
    lists.insert(where, np.sort(dests[at:]))
  return src, lists, n_out


def n_points(in_dtype, out_dtype) -> list:
  out = {1, 3, 4, 5}
  for wide in (False, True):
    tile = engine.slab_scatter_geometry(operands.torch_dtype(in_dtype),
                                        operands.torch_dtype(out_dtype),
                                        wide)['tile_points']
    out |= {tile - 1, tile, tile + 1, 2 * tile + 4}
  return sorted(out)


def field(rs, shape, dtype) -> np.ndarray:
  x = (rs.standard_normal(shape) * 1e3).astype(dtype)
  x.reshape(-1)[::97] = np.nan
  return x


# ---------------------------------------------------------------------------
# kernel edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shift', (0, 1), ids=('aligned', 'offset_by_one'))
@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_point_counts_destination_counts_and_groups(pair, shift):
  """n_point around the vector and the tile (wide where alignment and size
  allow, scalar otherwise and for a base offset by one element); sources with
  0, 1, d - 1, d, d + 1 destinations for d = 4 and d = 64, with 37 and with
  2 d = 128 (few sources and tiles: the blocks go over several lanes, so a
  block boundary and a whole number of blocks are met at every d); a -1 source
  among them; dests_per_group in {1, 4, 64} with equal bits."""
  in_dtype, out_dtype = PAIRS[pair]
  rs = np.random.RandomState(len(pair) + shift)
  src, lists, n_out = scattered_problem(
      rs, [0, 1, 3, 4, 5, 37, 63, 64, 65, 128], 11)
  table = table_of(src, lists, n_out)
  for n_point in n_points(in_dtype, out_dtype):
    flat = field(rs, (11, n_point), in_dtype)
    want = tn.scatter(flat, table, out_dtype)
    for d in DESTS_PER_GROUP:
      got = launch(flat, src, lists, n_out, out_dtype, d, shift)
      assert tn.same_bits(got, want), (n_point, d)


def test_geometry_matches_the_header():
  assert engine.slab_scatter_geometry(torch.float32, wide=True) == {
      'tile_points': 1024, 'max_grid_outer': 32768}
  assert engine.slab_scatter_geometry(torch.float64)['tile_points'] == 256


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_nan_source_alone(pair):
  in_dtype, out_dtype = PAIRS[pair]
  flat = field(np.random.RandomState(1), (2, 20), in_dtype)
  got = launch(flat, [-1], [np.arange(5)], 5, out_dtype, 4)
  want = np.full((5, 20), np.nan, dtype=out_dtype)
  assert tn.same_bits(got, want)  # the quiet NaN of NumPy, bit for bit
  # ... and with no input at all
  empty = torch.zeros((0, 20), dtype=operands.torch_dtype(in_dtype),
                      device='cuda')
  got = engine.slab_scatter(empty, [-1], [[1, 0]], 2, n_point=20,
                            out_dtype=operands.torch_dtype(out_dtype))
  assert tn.same_bits(got.cpu().numpy(), want[:2])


def test_one_source_with_many_destinations_fills_lanes():
  """Few (source, tile) pairs: the destination blocks go over several lanes
  of the grid."""
  rs = np.random.RandomState(2)
  flat = field(rs, (3, 2052), np.float32)
  src, lists, n_out = scattered_problem(rs, [301, 2, 256], 3, with_hole=130)
  want = tn.scatter(flat, table_of(src, lists, n_out))
  for d in DESTS_PER_GROUP:
    assert tn.same_bits(launch(flat, src, lists, n_out, np.float32, d), want)


def test_more_sources_than_one_grid_row():
  n = engine.slab_scatter_geometry(torch.float32)['max_grid_outer'] + 1
  rs = np.random.RandomState(3)
  flat = rs.standard_normal((n, 4)).astype(np.float32)
  dests = rs.permutation(n)
  got = launch(flat, np.arange(n), (np.arange(n + 1), dests), n, np.float32, 4)
  want = np.empty_like(flat)
  want[dests] = flat
  assert tn.same_bits(got, want)


def test_views_and_gather_bases_differ_in_the_table_alone():
  """A lead-sliced view that starts inside its storage, read where it lies."""
  rs = np.random.RandomState(4)
  base = torch.from_numpy(field(rs, (5, 6, 3, 8), np.float64)).cuda()
  view = base[:, 1::2]  # leads 1, 3, 5
  table = operands.stride_table(view, 2)
  assert table is not None and not view.is_contiguous()
  logical = rs.randint(-1, view.shape[0] * view.shape[1], size=40)
  physical = np.where(logical < 0, -1, table[np.maximum(logical, 0)])
  src, begin, dst = ti.plan_scatter(physical)
  got = engine.slab_scatter(view, src, (begin, dst), 40, n_point=24,
                            out_dtype=torch.float32)
  want = tn.scatter(view.cpu().numpy().reshape(-1, 24), logical, np.float32)
  assert tn.same_bits(got.cpu().numpy(), want)
  # a table that leaves the storage behind the view is refused on the host
  with pytest.raises(IndexError):
    engine.slab_scatter(view, [int(table.max()) + 5], [[0]], 1, n_point=24)


def test_refusals_on_the_host():
  x = torch.zeros((4, 8), dtype=torch.float32, device='cuda')
  with pytest.raises(TypeError, match='unsupported dtype pair'):
    engine.slab_scatter(x, [0], [[0]], 1, out_dtype=torch.float64)
  with pytest.raises(TypeError, match='unsupported dtype pair'):
    engine.slab_scatter(x.to(torch.int32), [0], [[0]], 1)
  with pytest.raises(ValueError, match='exactly once'):
    engine.slab_scatter(x, [0, 1], [[0], [0]], 2)
  with pytest.raises(ValueError, match='bad sizes'):
    engine.slab_scatter(x, [0], [[0]], 1, dests_per_group=0)
  with pytest.raises(ValueError, match='out must be'):
    engine.slab_scatter(x, [0], [[0]], 1, out=torch.zeros(
        (1, 8), dtype=torch.float64, device='cuda'))


# ---------------------------------------------------------------------------
# the f64 -> f32 cast
# ---------------------------------------------------------------------------
def test_cast_values():
  tiny = np.finfo(np.float32).tiny
  values = np.array([
      0.1, 1 / 3, 1 + 2.0**-24, 1 + 2.0**-24 + 2.0**-50, 1 + 3 * 2.0**-24,
      16777217.0, -16777219.0,                    # not representable: ties
      3.5e38, -3.5e38, 1e300, -1e300,             # beyond the range: inf
      float(np.finfo(np.float32).max), 3.4028235677973366e38,  # rounds to inf
      tiny / 2, -tiny / 3, 1e-45, 7e-46, 1e-46, 4.9e-324, 1e-310,  # subnormals
      0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float64)
  for n_point in (values.size, 4 * values.size):  # scalar and wide
    flat = np.resize(values, (3, n_point))
    flat[1] = -flat[1]
    table = np.array([2, 0, 1, 1, -1, 0])
    src, begin, dst = ti.plan_scatter(table)
    got = launch(flat, src, (begin, dst), 6, np.float32, 4)
    assert tn.same_bits(got, tn.scatter(flat, table, np.float32)), n_point
  assert np.isinf(got[1][7:11]).all() and got[1][20:22].tobytes() == \
      np.array([0.0, -0.0], np.float32).tobytes()


# ---------------------------------------------------------------------------
# the module on device inputs
# ---------------------------------------------------------------------------
def to_device(case, names=None, view=False):
  variables = {}
  for name, (dims, array) in case['vars'].items():
    if names is not None and name not in names:
      continue
    variables[name] = xl.DataArray(
        torch.from_numpy(np.ascontiguousarray(array)).cuda(), dims)
  return xl.Dataset(variables, dict(case['coords']))


def to_host(case, names=None):
  return xl.Dataset({k: xl.DataArray(a, d) for k, (d, a) in case['vars'].items()
                     if names is None or k in names}, dict(case['coords']))


class Launches:
  """Counts the K16 launches of a block."""

  def __enter__(self):
    self.count = 0
    self.old = engine.set_launch_hook(self)
    return self

  def __call__(self, when, kernel):
    self.count += when == 'begin' and kernel == 'slab_scatter'

  def __exit__(self, *exc):
    engine.set_launch_hook(self.old)


def check_device_dataset(ds, host, golden, prefix: str, kernel_vars: int):
  for name, want in host.data_vars.items():
    da = ds[name]
    assert da.dims == want.dims, name
    if name == ti.SOURCE_TIME:
      continue
    if kernel_vars is not None:
      assert isinstance(da.data, torch.Tensor) and da.data.is_cuda, name
    assert tn.same_bits(np.asarray(da.values), np.asarray(want.values)), name
    if prefix + name in golden:
      assert tn.same_bits(np.asarray(da.values), golden[prefix + name]), name


@pytest.mark.parametrize('name', sorted(tc.expand_cases()))
def test_expand_climatology_on_the_device(name, golden):
  case = tc.expand_cases()[name]()
  host = ti.expand_climatology(to_host(case), case['times'])
  with Launches() as launches:
    ds = ti.expand_climatology(to_device(case), case['times'])
  check_device_dataset(ds, host, golden, f'expand/{name}/', True)
  floats = sum(a.dtype.kind == 'f' and 'dayofyear' in d
               for d, a in case['vars'].values())
  assert launches.count == floats  # (integers without holes: torch gathers)


@pytest.mark.parametrize('name', sorted(tc.index_cases()))
def test_index_on_valid_time_on_the_device(name, golden):
  case = tc.index_cases()[name]()
  host = ti.index_on_valid_time(to_host(case), case['mode'])
  with Launches() as launches:
    ds = ti.index_on_valid_time(to_device(case), case['mode'])
  check_device_dataset(ds, host, golden, f'index/{name}/', True)
  assert launches.count == len(case['vars'])  # integers too: float32 first
  for da in ds.data_vars.values():
    assert da.data.dtype == torch.float32


@pytest.mark.parametrize('name', ['ens_grid', 'known_ens_default',
                                  'known_ens_custom_time_name',
                                  'known_ens_delta_less_than_init',
                                  'known_ens_subday_delta_less'])
def test_probabilistic_forecasts_on_the_device(name, golden):
  case = tc.ensemble_cases()[name]()
  host = ti.probabilistic_climatological_forecasts(to_host(case),
                                                   **case['kwargs'])
  with Launches() as launches:
    ds = ti.probabilistic_climatological_forecasts(to_device(case),
                                                   **case['kwargs'])
  check_device_dataset(ds, host, golden, f'ensemble/{name}/', True)
  assert launches.count == len(case['vars'])


def test_module_reads_views_and_gathers_where_they_lie(monkeypatch):
  """A lead-sliced view and a SlabGather over a resident base reach the
  kernel as the resident tensor and a table: nothing is copied first."""
  case = tc.index_cases()['index_grid_delta']()
  dims, x = case['vars']['geopotential']
  want = ti.index_on_valid_time(to_host(case, ['geopotential']))
  big = np.zeros((x.shape[0], 2 * x.shape[1]) + x.shape[2:], dtype=x.dtype)
  big[:, 1::2] = x
  resident = torch.from_numpy(big).cuda()
  perm = np.random.RandomState(6).permutation(x.shape[0] * x.shape[1] * 2)
  shuffled = torch.from_numpy(x.reshape((-1,) + x.shape[-2:])[perm]).cuda()
  inverse = np.argsort(perm).reshape(x.shape[:3])
  monkeypatch.setattr(xl.SlabGather, 'materialize',
                      lambda self, *a, **k: pytest.fail('materialised'))
  real_scatter = engine.slab_scatter
  read = []

  def spy(x, *args, **kwargs):
    read.append(x.untyped_storage().data_ptr())
    return real_scatter(x, *args, **kwargs)

  monkeypatch.setattr(engine, 'slab_scatter', spy)
  for data, storage in ((resident[:, 1::2], resident),
                        (xl.SlabGather(shuffled, inverse), shuffled)):
    ds = xl.Dataset({'geopotential': xl.DataArray(data, dims)}, case['coords'])
    with Launches() as launches:
      got = ti.index_on_valid_time(ds)
    assert launches.count == 1
    assert read.pop() == storage.untyped_storage().data_ptr()  # (no copy)
    assert tn.same_bits(got['geopotential'].values,
                        want['geopotential'].values)


def test_variables_that_share_a_table_are_planned_once(monkeypatch):
  case = tc.ensemble_cases()['ens_grid']()
  dims, x = case['vars']['geopotential']
  twin = dict(case, vars={'a': (dims, x), 'b': (dims, x[::-1].copy()),
                          'c': (dims, x.astype(np.float64))})
  real, calls = ti.plan_scatter, []
  monkeypatch.setattr(ti, 'plan_scatter',
                      lambda *a, **k: calls.append(1) or real(*a, **k))
  with Launches() as launches:
    ds = ti.probabilistic_climatological_forecasts(to_device(twin),
                                                   **case['kwargs'])
  assert launches.count == 3 and len(calls) == 1
  host = ti.probabilistic_climatological_forecasts(to_host(twin),
                                                   **case['kwargs'])
  check_device_dataset(ds, host, {}, 'none/', True)


# ---------------------------------------------------------------------------
# the zero-copy path: existing kernels, new tables
# ---------------------------------------------------------------------------
def _same_results(a, b):
  assert set(a.data_vars) == set(b.data_vars)
  for name in a.data_vars:
    assert a[name].dims == b[name].dims
    assert tn.same_bits(np.asarray(a[name].values), np.asarray(b[name].values))


def test_crps_reads_the_lazy_ensemble_in_place():
  from weatherbench2_amd import metrics as gm
  case = tc.ensemble_cases()['ens_grid']()
  truth = to_device(case, ['geopotential'])
  lazy = ti.probabilistic_climatological_forecasts(
      truth, materialize=False, **case['kwargs'])
  done = ti.probabilistic_climatological_forecasts(truth, **case['kwargs'])
  gather = lazy['geopotential'].data
  assert isinstance(gather, xl.SlabGather)
  assert gather.base.data_ptr() == truth['geopotential'].data.data_ptr()
  dims = done['geopotential'].dims[1:]
  shape = done['geopotential'].shape[1:]
  rs = np.random.RandomState(7)
  target = xl.Dataset({'geopotential': xl.DataArray(
      torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).cuda(),
      dims)}, {k: v for k, v in done.coords.items() if k != 'realization'})
  for name in (ti.SOURCE_TIME,):
    lazy.data_vars.pop(name, None)
    done.data_vars.pop(name, None)
  for metric in (gm.CRPS(), gm.EnsembleMeanMSE()):
    _same_results(metric.compute_chunk(lazy, target),
                  metric.compute_chunk(done, target))


def test_mse_reads_the_lazy_valid_time_forecast_in_place():
  from weatherbench2_amd import metrics as gm
  case = tc.index_cases()['index_lead_first_delta']()
  forecast = to_device(case)
  lazy = ti.index_on_valid_time(forecast, materialize=False)
  done = ti.index_on_valid_time(forecast)
  assert lazy['wind'].data.has_missing
  rs = np.random.RandomState(8)
  target = xl.Dataset({'wind': xl.DataArray(
      torch.from_numpy(rs.standard_normal(done['wind'].shape
                                          ).astype(np.float32)).cuda(),
      done['wind'].dims)}, done.coords)
  for skipna in (False, True):
    _same_results(gm.MSE().compute_chunk(lazy, target, skipna=skipna),
                  gm.MSE().compute_chunk(done, target, skipna=skipna))
