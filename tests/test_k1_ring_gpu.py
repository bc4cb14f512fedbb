"""K1's ring form against its batch form (-m gpu).

stream_partials_kernel<..., RING> feeds a wave's rows through RING stages of
LDS filled by LDS-DMA; the batch form loads U rows into registers.  Same loads
per lane, same arithmetic, same order of the float64 additions: the partials,
the folded sums and the metrics must have the SAME BITS.  Every case runs
engine.stream_reduce with WB2HIP_K1_RING = 0 (batch), 3 and 4 (ring forced)
and compares bit patterns; the batch result is also held against a NumPy
float64 reference at the tolerance of tests/test_det_gpu.py.

Shapes are the smallest at which the ring can go wrong: chunks of 1, 2,
RING - 1, RING, RING + 1 and 2 RING + 1 rows for both depths (asserted on the
plan), a one-row band between two latitude slices that share an endpoint, the
empty chunks that pad the plan to a multiple of 8, a slab of two rows; one
full column tile, a second tile with one active lane, four tiles, and 1440
columns (last tile 160 columns wide).
"""
import contextlib
import os
import re

import numpy as np
import pytest

from oracle import regions_np as oreg
from oracle.named import NA
from tests import geometry_reference as gr
from tests import helpers
from tests import stream_geometry_cases as sg

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12  # tests/test_det_gpu.py
DEPTHS = (3, 4)
SWITCH = 'WB2HIP_K1_RING'
SENTINEL = -12345.0
# rows of the bands (= chunks, at 9 rows per chunk) of band_regions(), top down
BAND_ROWS = (1, 2, 3, 4, 5, 7, 9, 2, 1, 3)
WANTED_ROWS = {1, 2} | {d + k for d in DEPTHS for k in (-1, 0, 1)} | {
    2 * d + 1 for d in DEPTHS}
N_ROW = sum(BAND_ROWS)
TABLES = {'identity': None, 'perm': (2, 0, 1), 'twice': (1, 1, 0)}


@pytest.fixture(scope='module')
def dev():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  return torch.device('cuda')


@contextlib.contextmanager
def ring_switch(value):
  """WB2HIP_K1_RING = value (None: unset) for the launches inside."""
  old = os.environ.pop(SWITCH, None)
  if value is not None:
    os.environ[SWITCH] = str(value)
  try:
    yield
  finally:
    os.environ.pop(SWITCH, None)
    if old is not None:
      os.environ[SWITCH] = old


def band_regions(lat, lon, n_col):
  """Latitude slices whose bands have BAND_ROWS rows (the 8th and 10th region
  share the row between them: a one-row band), and a longitude box that cuts
  the columns into three segs across the first tile edge."""
  out = {'global': oreg.SliceRegion()}
  r = 0
  spans = []
  for n in BAND_ROWS:
    spans.append((r, r + n - 1))
    r += n
  for i, (a, b) in enumerate(spans):
    if i == 8:                      # the shared endpoint belongs to both
      continue
    if i == 7:
      b = spans[8][1]
    if i == 9:
      a = spans[8][0]
    out[f'rows{i}'] = oreg.SliceRegion(
        lat_slice=slice(float(lat[a]), float(lat[b])))
  c0, c1 = max(n_col // 2 - 70, 1), min(n_col // 2 + 140, n_col - 2)
  out['box'] = oreg.SliceRegion(      # whole bands: rows 3 .. 30
      lat_slice=slice(float(lat[3]), float(lat[30])),
      lon_slice=slice(float(lon[c0]), float(lon[c1])))
  return out


def make_plan(lat, lon, regions, dev, rows_per_chunk=9):
  from weatherbench2_amd import plan as plan_lib
  return plan_lib.build_plan(
      lat, lon, plan_lib.LATLON,
      {k: helpers.to_gpu_region(v) for k, v in regions.items()}, dev,
      rows_per_chunk=rows_per_chunk)


def mode_code(mode):
  from weatherbench2_amd import _lib
  return {'det': _lib.MODE_DET, 'det_acc': _lib.MODE_DET_ACC,
          'wind': _lib.MODE_WIND}[mode]


def make_inputs(mode, shape, seed, dtype=np.float32):
  rs = np.random.RandomState(seed)

  def err():
    return np.where(rs.rand(*shape) < 0.3, -1.0, 1.0) * rs.uniform(0.25, 1.5,
                                                                    shape)
  if mode == 'det':
    t = rs.uniform(-3, 3, shape)
    ins = [t + err(), t]
  elif mode == 'det_acc':
    c = rs.uniform(-3, 3, shape)
    t = c + err()
    ins = [t + err(), t, c]
  else:
    tu, tv = rs.uniform(-3, 3, shape), rs.uniform(-3, 3, shape)
    ins = [tu + err(), tu, tv + err(), tv]
  return [x.astype(dtype) for x in ins]


def k1_partials(pl, mode, t_ins, tabs, n_outer, skipna):
  """K1 alone through the C ABI (wb2_stream_partials_ex) into a buffer of the
  test's own, pre-filled with a sentinel: [n_outer, n_chunk, nwf, n_ts, K]."""
  import torch
  from weatherbench2_amd import _lib
  from weatherbench2_amd import engine
  lib = _lib.load()
  code = {torch.float32: _lib.WB2_F32, torch.float64: _lib.WB2_F64}[
      t_ins[0].dtype]
  m = mode_code(mode)
  aligned = all(x.data_ptr() % 16 == 0 for x in t_ins) and (
      pl.wfield is None or pl.wfield.data_ptr() % 16 == 0)
  tile = lib.wb2_tile_cols_ex(m, code, int(skipna), int(pl.wfield is not None),
                              pl.n_col, int(aligned))
  seg_eoff, n_ts = pl.seg_entries(tile)
  k = lib.wb2_num_slots(m, int(skipna))
  out = torch.full((n_outer, pl.n_chunk, pl.nwf, n_ts, k), SENTINEL,
                   dtype=torch.float64, device=pl.device)
  _lib.check(lib.wb2_stream_partials_ex(
      m, code, int(skipna), _lib.ptr_array(t_ins), _lib.ptr_array(tabs),
      n_outer, pl.n_row, pl.n_col, _lib.ptr(pl.w_row), _lib.ptr(pl.w_col),
      _lib.ptr(pl.wfield), _lib.WB2_F64, None, 0.0, _lib.ptr(pl.chunk_row0),
      _lib.ptr(pl.chunk_nrow), pl.n_chunk, -(-pl.n_col // tile),
      _lib.ptr(pl.seg_col0), _lib.ptr(seg_eoff), pl.n_seg, n_ts,
      _lib.ptr(out), engine.current_stream_ptr(pl.device)),
             'wb2_stream_partials_ex')
  return out


def launch(pl, mode, t_ins, tabs, n_outer, switch, skipna=False):
  """(K1's partials, sums, metrics) as NumPy arrays: the partials from K1
  alone into the test's own buffer, sums and metrics from
  engine.stream_reduce (K1 + K2)."""
  import torch
  from weatherbench2_amd import engine
  with ring_switch(switch):
    part = k1_partials(pl, mode, t_ins, tabs, n_outer, skipna)
    m, s = engine.stream_reduce(pl, mode_code(mode), t_ins, tabs, n_outer,
                                skipna, want_sums=True)
    torch.cuda.synchronize()
  part = part.cpu().numpy()
  full = pl.chunk_nrow.cpu().numpy() > 0
  assert not (part[:, full] == SENTINEL).any()   # every entry written
  assert (part[:, ~full] == SENTINEL).all()      # empty chunks write nothing
  return part, s.cpu().numpy(), m.cpu().numpy()


def assert_same_bits(got, want, tag):
  for name, g, w in zip(('partials', 'sums', 'metrics'), got, want):
    assert g.shape == w.shape and g.dtype == w.dtype == np.float64, (tag, name)
    same = g.view(np.uint64) == w.view(np.uint64)
    if not same.all():
      at = tuple(np.argwhere(~same)[0])
      raise AssertionError(f'{tag}: {name}{at}: ring {g[at]!r} ({g.view(np.uint64)[at]:#x}) '
                           f'batch {w[at]!r} ({w.view(np.uint64)[at]:#x}); '
                           f'{(~same).sum()} of {same.size} differ')


def reference_metrics(mode, ins, outer, weights):
  """[MSE, RMSE, MAE, Bias, ACC][n_region][n_outer] in float64 from per-point
  quantities computed in the input dtype: sum(w x) / sum(w) over the points
  with w > 0 (weights = latitude weights x what Region.apply leaves)."""
  x = [a[np.asarray(outer)] for a in ins]
  with np.errstate(all='ignore'):
    if mode == 'wind':
      du, dv = x[0] - x[1], x[2] - x[3]
      q = {'mse': du * du + dv * dv}
    else:
      d = x[0] - x[1]
      q = {'bias': d, 'mae': np.abs(d), 'mse': d * d}
      if mode == 'det_acc':
        fa, ta = x[0] - x[2], x[1] - x[2]
        q.update(ft=fa * ta, ff=fa * fa, tt=ta * ta)
    out = np.full((5, len(weights), len(outer)), np.nan)
    for r, w in enumerate(weights):
      inside = w > 0
      mean = {k: (np.where(inside, v.astype(np.float64), 0.0) * w).sum(
          axis=(1, 2)) / w.sum() for k, v in q.items()}
      out[0, r] = mean['mse']
      out[1, r] = np.sqrt(mean['mse'])
      if mode != 'wind':
        out[2, r], out[3, r] = mean['mae'], mean['bias']
      if mode == 'det_acc':
        out[4, r] = mean['ft'] / np.sqrt(mean['ff'] * mean['tt'])
  return out


def assert_reference(metrics, mode, ins, outer, regions, lat, lon, tag):
  weights = [gr.region_weights(r, lat, lon, 'latlon')
             for r in regions.values()]
  want = reference_metrics(mode, ins, outer, weights)
  np.testing.assert_allclose(metrics, want, rtol=RTOL, atol=ATOL,
                             equal_nan=True, err_msg=tag)


def to_device(ins, table, dev):
  import torch
  t_ins = [torch.as_tensor(x, device=dev) for x in ins]
  if table is None:
    return t_ins, [None] * len(ins)
  tab = torch.as_tensor(np.array(table), dtype=torch.int64, device=dev)
  return t_ins, [tab] * len(ins)


def compare_forms(pl, mode, ins, table, dev, tag, depths=DEPTHS, skipna=False):
  """Batch and ring-forced launches of the same inputs; returns the batch
  result after asserting the same bits."""
  t_ins, tabs = to_device(ins, table, dev)
  n_outer = len(table) if table is not None else ins[0].shape[0]
  batch = launch(pl, mode, t_ins, tabs, n_outer, 0, skipna)
  for depth in depths:
    ring = launch(pl, mode, t_ins, tabs, n_outer, depth, skipna)
    assert_same_bits(ring, batch, f'{tag} ring {depth}')
  return batch


# (mode, n_col, slabs in the pool, slab table)
CASES = [
    ('det_acc', 1440, 3, 'perm'),
    ('det_acc', 256, 1, 'identity'),
    ('det_acc', 1024, 3, 'twice'),
    ('det', 260, 3, 'twice'),
    ('det', 1024, 3, 'identity'),
    ('det', 1440, 3, 'perm'),
    ('wind', 1440, 1, 'identity'),
    ('wind', 260, 3, 'perm'),
    ('wind', 256, 3, 'twice'),
]


@pytest.mark.parametrize('mode,n_col,n_pool,table', CASES,
                         ids=['-'.join(map(str, c)) for c in CASES])
def test_ring_gives_the_batch_bits(dev, mode, n_col, n_pool, table):
  lat, lon = sg.coords(N_ROW, n_col, 'latlon')
  regions = band_regions(lat, lon, n_col)
  pl = make_plan(lat, lon, regions, dev)
  nrow = pl.chunk_nrow.cpu().numpy()
  assert WANTED_ROWS <= set(nrow.tolist()), nrow     # rows around both depths
  assert (nrow == 0).any(), nrow                       # a padded empty chunk
  assert pl.n_seg >= 3
  ins = make_inputs(mode, (n_pool, N_ROW, n_col), seed=n_col + n_pool)
  tab = TABLES[table]
  outer = tab if tab is not None else tuple(range(n_pool))
  tag = f'{mode} n_col={n_col} {table}'
  _, _, metrics = compare_forms(pl, mode, ins, tab, dev, tag)
  assert_reference(metrics, mode, ins, outer, regions, lat, lon, tag)


@pytest.mark.parametrize('mode', ['det', 'det_acc', 'wind'])
def test_slab_with_fewer_rows_than_the_ring(dev, mode):
  """Two rows in all: the ring is never full, every request is up front."""
  n_col = 260
  lat, lon = sg.coords(2, n_col, 'latlon')
  regions = {'global': oreg.SliceRegion(),
             'top': oreg.SliceRegion(lat_slice=slice(float(lat[1]), None))}
  pl = make_plan(lat, lon, regions, dev)
  assert pl.chunk_nrow.cpu().numpy().sum() == 2
  ins = make_inputs(mode, (3, 2, n_col), seed=5)
  _, _, metrics = compare_forms(pl, mode, ins, None, dev, f'{mode} two rows')
  assert_reference(metrics, mode, ins, (0, 1, 2), regions, lat, lon,
                   f'{mode} two rows')


@pytest.mark.parametrize('mode', ['det', 'det_acc', 'wind'])
def test_non_finite_values_propagate_alike(dev, mode):
  """NaN, +Inf and -Inf inside and outside every region: the same bits from
  both forms, NaN patterns included, and the reference's values."""
  n_col = 1440
  lat, lon = sg.coords(N_ROW, n_col, 'latlon')
  regions = {
      'north': oreg.SliceRegion(lat_slice=slice(float(lat[22]), None)),
      'south': oreg.SliceRegion(lat_slice=slice(None, float(lat[14]))),
      'box': oreg.SliceRegion(lat_slice=slice(float(lat[3]), float(lat[30])),
                              lon_slice=slice(float(lon[200]),
                                              float(lon[300]))),
      'clean': oreg.SliceRegion(lat_slice=slice(float(lat[5]), float(lat[12])),
                                lon_slice=slice(float(lon[900]),
                                                float(lon[1300])))}
  pl = make_plan(lat, lon, regions, dev)
  ins = make_inputs(mode, (3, N_ROW, n_col), seed=11)
  f, t = ins[0], ins[1]
  f[0, 25, 10] = np.nan        # north only
  f[0, 2, 1439] = np.inf       # south only
  t[0, 10, 250] = -np.inf      # south and box
  t[1, 18, 250] = np.nan       # box only
  f[1, 18, 700] = np.inf       # outside every region (rows 15 .. 21, no box)
  t[1, 17, 5] = np.nan         # outside every region
  ins[-1][2, 30, 256] = np.inf  # north and box, first lane of tile 1
  f[2, 36, 1280] = -np.inf     # north, first lane of the partial last tile
  tag = f'{mode} non-finite'
  _, _, metrics = compare_forms(pl, mode, ins, (2, 0, 1), dev, tag)
  assert_reference(metrics, mode, ins, (2, 0, 1), regions, lat, lon, tag)
  clean = list(regions).index('clean')
  rows = (0, 1) if mode == 'wind' else (0, 1, 2, 3)
  assert np.isfinite(metrics[rows, clean]).all()
  assert not np.isfinite(metrics[0]).all()


def test_forced_ring_falls_back_to_the_batch_form(dev):
  """No ring instantiation for skipna, float64, a weight field, a base that is
  not 16-byte aligned or rows of 721 columns: the forced switch must leave the
  batch form's result."""
  import torch
  lat, lon = sg.coords(N_ROW, 1440, 'latlon')
  regions = band_regions(lat, lon, 1440)
  pl = make_plan(lat, lon, regions, dev)
  shape = (3, N_ROW, 1440)
  outer = (0, 1, 2)

  ins = make_inputs('det_acc', shape, seed=21)
  ins[0][1, 7, 300] = np.nan
  compare_forms(pl, 'det_acc', ins, None, dev, 'skipna', skipna=True)

  ins = make_inputs('det', shape, seed=22, dtype=np.float64)
  _, _, metrics = compare_forms(pl, 'det', ins, None, dev, 'float64')
  assert_reference(metrics, 'det', ins, outer, regions, lat, lon, 'float64')

  # base pointers 4 bytes past a 16-byte boundary
  ins = make_inputs('det_acc', shape, seed=23)
  n_el = int(np.prod(shape))
  t_ins = []
  for x in ins:
    buf = torch.zeros((n_el + 4,), dtype=torch.float32, device=dev)
    buf[1:n_el + 1] = torch.as_tensor(x.ravel(), device=dev)
    view = buf[1:n_el + 1].view(shape)
    assert view.data_ptr() % 16 == 4
    t_ins.append(view)
  batch = launch(pl, 'det_acc', t_ins, [None] * 3, 3, 0)
  for depth in DEPTHS:
    assert_same_bits(launch(pl, 'det_acc', t_ins, [None] * 3, 3, depth), batch,
                     f'offset base ring {depth}')
  assert_reference(batch[2], 'det_acc', ins, outer, regions, lat, lon,
                   'offset base')

  # a 2-D weight field (land mask)
  mask = NA(sg.land_mask('f32', lat, lon), ('latitude', 'longitude'))
  land = dict(regions, land=oreg.LandRegion(mask, lat, lon))
  pl_land = make_plan(lat, lon, land, dev)
  assert pl_land.wfield is not None
  ins = make_inputs('det_acc', shape, seed=24)
  _, _, metrics = compare_forms(pl_land, 'det_acc', ins, None, dev, 'field')
  assert_reference(metrics, 'det_acc', ins, outer, land, lat, lon, 'field')

  # rows of 721 columns: no 16-byte aligned rows
  lat7, lon7 = sg.coords(N_ROW, 721, 'latlon')
  regions7 = band_regions(lat7, lon7, 721)
  pl7 = make_plan(lat7, lon7, regions7, dev)
  ins = make_inputs('det', (3, N_ROW, 721), seed=25)
  _, _, metrics = compare_forms(pl7, 'det', ins, None, dev, '721 columns')
  assert_reference(metrics, 'det', ins, outer, regions7, lat7, lon7,
                   '721 columns')


def test_small_launch_keeps_the_batch_form_by_default(dev):
  """The rule (switch unset): a one-slab launch is far below four rounds of
  resident workgroups and takes the batch form.  Neither the launch hook nor
  a counter tells the forms apart, so this asserts the result only."""
  lat, lon = sg.coords(N_ROW, 1440, 'latlon')
  regions = band_regions(lat, lon, 1440)
  pl = make_plan(lat, lon, regions, dev)
  ins = make_inputs('det_acc', (1, N_ROW, 1440), seed=31)
  t_ins, tabs = to_device(ins, None, dev)
  batch = launch(pl, 'det_acc', t_ins, tabs, 1, 0)
  assert_same_bits(launch(pl, 'det_acc', t_ins, tabs, 1, None), batch,
                   'switch unset')
  assert_reference(batch[2], 'det_acc', ins, (0,), regions, lat, lon,
                   'switch unset')


# ---- which kernel ran ---------------------------------------------------------
def k1_kernel_names(fn):
  """Names of the stream_partials_kernel launches inside fn(), from torch's
  profiler (it records every kernel of the process, ours included)."""
  import torch
  from torch.profiler import ProfilerActivity, profile
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize()
  return [e.name for e in prof.events()
          if 'stream_partials_kernel' in e.name]


def ring_depth_of(name):
  """The trailing RING template argument of a kernel name, 0 without one."""
  m = re.search(r'double, (\d+)>', name)
  return int(m.group(1)) if m else 0


def test_the_switch_and_the_rule_select_the_kernel(dev):
  """The forced switch launches the ring instantiation of that depth, `0` and
  a small launch with the switch unset the batch form, a large launch with the
  switch unset the ring (at least four rounds of resident workgroups: 256
  columns are one wave per workgroup, 12 KiB of LDS at depth 4, 13 workgroups
  per CU; 16 chunks x 1024 slabs = 16 384 workgroups against 4 x 256 CUs x 13
  = 13 312)."""
  import torch
  from weatherbench2_amd import engine
  lat, lon = sg.coords(N_ROW, 256, 'latlon')
  pl = make_plan(lat, lon, band_regions(lat, lon, 256), dev)
  ins = make_inputs('det_acc', (2, N_ROW, 256), seed=41)
  t_ins = [torch.as_tensor(x, device=dev) for x in ins]

  def run(switch, n_outer):
    tab = torch.arange(n_outer, dtype=torch.int64, device=dev) % 2
    out = []

    def go():
      with ring_switch(switch):
        out.append(engine.stream_reduce(pl, mode_code('det_acc'), t_ins,
                                        [tab] * 3, n_outer, False))
    names = k1_kernel_names(go)
    assert len(names) == 1, names
    return ring_depth_of(names[0]), out[0][0]

  assert run(0, 2)[0] == 0
  assert run(3, 2)[0] == 3
  assert run(4, 2)[0] == 4
  assert run(None, 2)[0] == 0
  depth, big = run(None, 1024)
  assert depth in DEPTHS, depth
  _, big_batch = run(0, 1024)
  assert torch.equal(big.view(torch.int64), big_batch.view(torch.int64))
