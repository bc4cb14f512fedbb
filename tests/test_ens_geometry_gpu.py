"""The ensemble reductions across tile, row-end, 64-row-block, segment and grid
edges (-m gpu).

K3 (ens_partials_kernel + wb2_ens_combine), K3t (ens_threshold_kernel +
wb2_det_combine) and K3e (energy_partials_kernel) over the sweep of
tests/ens_geometry_cases.py (its coverage is asserted on the CPU by
test_ens_geometry_cpu.py), in two parts:

1. Per-point values.  K3's maps (written into a view of a larger buffer with
   sentinel guard bands) and K3t's maps (wb2_ens_threshold_maps, the same point
   function) against the oracle's pointwise fields at the tolerances of
   test_ens_exact_gpu.py / test_thresholds_gpu.py; every point must be written
   and the guard bands left alone.
2. The fold.  The raw region sums against math.fsum of the oracle's region
   weights times the kernel's own per-point values, to 1e-12 * sum|w x|
   (tests/geometry_reference.py); the metric rows against the combine's
   formulas on those sums.  K3e's float32 / float64 squares are reproducible
   in NumPy (-ffp-contract=off), so its (score, spread, skill) are compared
   with fsum-based means, square roots and member means.

Each case proves on the reference alone that dropping column 64 or counting
column n_col - 1 twice breaks the sum tolerance.
"""
import numpy as np
import pytest

from oracle import metrics_np as om
from oracle.named import DS, NA
from tests import ens_geometry_cases as eg
from tests import geometry_reference as gr
from tests import helpers

pytestmark = pytest.mark.gpu

N_POOL = 3
TABLE = (2, 0, 2, 1)  # permutes and repeats the pool's slabs
SENTINEL = -7.25e300  # what the maps and their guard bands start as
GUARD = 64
METRIC_RTOL = 1e-10


@pytest.fixture(scope='module')
def dev():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  return torch.device('cuda')


def _seed(case):
  return sum(map(ord, case.id)) % 100003


def _make_plan(res, dev):
  from weatherbench2_amd import plan as plan_lib
  return plan_lib.build_plan(
      res.lat, res.lon,
      plan_lib.LATLON if res.case.layout == 'latlon' else plan_lib.LONLAT,
      {k: helpers.to_gpu_region(v) for k, v in res.regions.items()}, dev,
      rows_per_chunk=res.case.rows_per_chunk)


def _weights(res):
  return [gr.region_weights(r, res.lat, res.lon, res.case.layout)
          for r in res.regions.values()]


def _ds(x, members):
  dims = (('realization',) if members else ()) + ('y', 'x')
  return DS({'z': NA(x, dims)}, {'y': np.arange(x.shape[-2]),
                                 'x': np.arange(x.shape[-1])})


def _assert_rows(got, want, names, tag):
  """Metric rows [n_metric, n_region, n_outer]: NaN where `want` is NaN, else
  METRIC_RTOL (quotients of positive sums good to SUM_RTOL)."""
  got = np.asarray(got, dtype=np.float64)
  assert got.shape == want.shape, (got.shape, want.shape, tag)
  with np.errstate(invalid='ignore'):
    ok = (np.isnan(got) == np.isnan(want)) & (
        np.isnan(want) | (np.abs(got - want) <= METRIC_RTOL * np.abs(want)))
  if not ok.all():
    m, r, o = np.argwhere(~ok)[0]
    raise AssertionError(f'{tag}: metric {m} region {names[r]} outer {o}: '
                         f'got {got[m, r, o]!r} want {want[m, r, o]!r}')


def _nan_patterns(res, pl, ens, truth, weights):
  """Strict: one NaN member at column n_col - 1 of pool slab 1.  Skipna:
  NaN members in the last column and on the first column of tiles, a NaN
  truth row, truth NaN over all of region 'one_col' (pool slab 2); with chunks
  of more than 64 rows instead: NaNs only past row 64 of those chunks (slab 0,
  one wave of the row) and in both 64-row blocks (slab 1)."""
  case = res.case
  n, rows = res.n_col, np.arange(res.n_row)
  m_last = ens.shape[0] - 1
  if not case.skipna:
    ens[0, 1, 0, n - 1] = np.nan
    return
  long = [(int(r0), int(k)) for r0, k in zip(pl.chunk_row0_host,
                                             pl.chunk_nrow_host) if k > 64]
  if long:
    for r0, k in long:
      ens[0, 0, r0 + 64:r0 + k:3, min(5, n - 1)] = np.nan
      ens[m_last, 0, r0 + 66:r0 + k:7, n - 1] = np.nan
      ens[0, 1, r0 + 3, min(7, n - 1)] = np.nan
      ens[0, 1, r0 + 70, min(7, n - 1)] = np.nan
    return
  ens[0, 0, rows % 3 == 2, n - 1] = np.nan
  for c in range(eg.T, n, eg.T):
    ens[m_last, 0, rows % 2 == 1, c] = np.nan
  truth[1, res.n_row // 2, :] = np.nan
  if 'one_col' in res.regions:
    truth[2][weights[list(res.regions).index('one_col')] != 0] = np.nan


# ---- K3 -----------------------------------------------------------------------


def k3_slots(maps, skipna):
  """The K3 partial slots of every point from the kernel's maps [6, o, p]."""
  if not skipna:
    return [maps[k] for k in range(6)]
  ok = [~np.isnan(maps[k]) for k in range(6)]
  return ([np.nan_to_num(maps[k], nan=0.0) for k in range(6)] +
          [ok[j].astype(np.float64) for j in (0, 1, 3, 5)])


def k3_metrics(sums, wsum, skipna):
  """wb2_ens_combine's eight metrics [8, n_region, n_outer]."""
  s = np.moveaxis(sums, 0, -1)  # [n_region, K, n_outer]
  with np.errstate(all='ignore'):
    den = lambda j: (np.where(s[:, j] != 0, s[:, j], np.nan) if skipna
                     else np.where(wsum != 0, wsum, np.nan)[:, None])
    skill, spread = s[:, 0] / den(6), s[:, 1] / den(7)
    emse, var = s[:, 2] / den(6), s[:, 3] / den(8)
    return np.stack([skill - 0.5 * spread, spread, skill, emse, np.sqrt(emse),
                     var, np.sqrt(s[:, 4] / den(8)), s[:, 5] / den(9)])


def _k3_ensemble(res, rs, pl, weights):
  case = res.case
  shape = (case.n_member, N_POOL, res.n_row, res.n_col)
  ens = rs.uniform(-1, 1, shape).astype(case.dtype)
  sign = np.where(rs.rand(*shape[1:]) < 0.5, -1.0, 1.0)
  truth = (sign * rs.uniform(2.5, 3.5, shape[1:])).astype(case.dtype)
  _nan_patterns(res, pl, ens, truth, weights)
  return ens, truth


def _gather_index(case):
  """[n_outer, M] flat slab indices (member * N_POOL + pool slab) of the
  gathered members: rotated per outer index, member 1 repeats member 0."""
  m = case.n_member
  out = np.zeros((len(TABLE), m), dtype=np.int64)
  for o, s in enumerate(TABLE):
    mem = np.roll(np.arange(m)[::-1], o)
    if m >= 3:
      mem[1] = mem[0]
    out[o] = mem * N_POOL + s
  return out


def run_k3(res, pl, ens, truth, dev):
  """(maps [6, n_outer, P], sums, metrics, members [n_outer][M, R, C],
  truth [n_outer, R, C]) of the case's slab form."""
  import torch
  from weatherbench2_amd import engine
  case = res.case
  tdt = getattr(torch, case.dtype)
  p = res.n_row * res.n_col
  M = case.n_member
  table = np.array(TABLE)
  n_outer = N_POOL if case.slabs == 'contiguous' else len(table)
  outer = np.arange(N_POOL) if case.slabs == 'contiguous' else table
  d_truth = torch.as_tensor(truth, device=dev)
  d_tab = torch.as_tensor(table, dtype=torch.int64, device=dev)
  slab_tab = None if case.slabs == 'contiguous' else d_tab
  n_maps = 6 * n_outer * p
  buf = torch.full((n_maps + 2 * GUARD,), SENTINEL, dtype=torch.float64,
                   device=dev)
  maps = buf[GUARD:GUARD + n_maps]
  kw = dict(want_sums=True, maps=maps)
  if case.slabs == 'gather':
    d_ens = torch.as_tensor(ens, device=dev)
    index = _gather_index(case)
    kw['member_ptrs'] = torch.as_tensor(
        engine.gather_pointers(d_ens, index, p), device=dev)
    members = [ens.reshape(M * N_POOL, res.n_row, res.n_col)[ix]
               for ix in index]
    stride = N_POOL * p
  elif case.slabs == 'stride':
    # members far apart, NaNs between them
    stride = N_POOL * p + 7
    flat = np.full(M * stride, np.nan, dtype=case.dtype)
    for m in range(M):
      flat[m * stride:m * stride + N_POOL * p] = ens[m].ravel()
    d_ens = torch.as_tensor(flat, device=dev)
    members = [ens[:, s] for s in outer]
  else:
    d_ens = torch.as_tensor(ens, device=dev)
    stride = N_POOL * p
    members = [ens[:, s] for s in outer]
  metrics, sums = engine.ensemble_reduce(
      pl, d_ens, stride, M, slab_tab, d_truth, slab_tab, n_outer, case.skipna,
      **kw)
  host = buf.cpu().numpy()
  assert (host[:GUARD] == SENTINEL).all() and (
      host[GUARD + n_maps:] == SENTINEL).all(), 'K3 wrote into a guard band'
  got_maps = host[GUARD:GUARD + n_maps].reshape(6, n_outer, p)
  unwritten = got_maps == SENTINEL
  assert not unwritten.any(), (
      f'{int(unwritten.sum())} map entries never written, first at '
      f'{np.argwhere(unwritten)[0]} (slot, outer, point)')
  if case.slabs in ('addr', 'addr_offset'):
    # member 0's slab and the truth slab by byte address; members follow
    # member_stride elements behind (one element past an aligned base)
    elem = np.dtype(case.dtype).itemsize
    lead = int(case.slabs == 'addr_offset')
    keep = []
    addr = np.zeros((2, n_outer), dtype=np.int64)
    for i, x in enumerate((ens, truth)):
      b = torch.zeros((x.size + lead,), dtype=tdt, device=dev)
      b[lead:] = torch.as_tensor(x.ravel(), device=dev)
      keep.append(b)
      addr[i] = b.data_ptr() + lead * elem + table * p * elem
    d_addr = torch.as_tensor(addr, device=dev)
    m_a, s_a = engine.ensemble_reduce(
        pl, keep[0], stride, M, None, keep[1], None, n_outer, case.skipna,
        want_sums=True, addresses=d_addr)
    torch.cuda.synchronize()
    assert np.array_equal(s_a.cpu().numpy(), sums.cpu().numpy(),
                          equal_nan=True), 'address form != slab-table form'
    assert np.array_equal(m_a.cpu().numpy(), metrics.cpu().numpy(),
                          equal_nan=True)
  return (got_maps, sums.cpu().numpy(), metrics.cpu().numpy(), members,
          truth[outer])


def check_k3_maps(case, maps, members, truths):
  tol = (dict(rtol=2e-6, atol=1e-7) if case.dtype == 'float32' else
         dict(rtol=1e-9, atol=1e-12))
  shape = truths.shape[1:]
  for o in range(len(members)):
    with np.errstate(all='ignore'):
      import warnings
      with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fields = om_fields(_ds(members[o], True), _ds(truths[o], False),
                           case.skipna)
    for k, f in enumerate(fields):
      helpers.assert_close(maps[k, o].reshape(shape),
                           np.asarray(f['z'].data, dtype=np.float64),
                           err_msg=f'{case.id} map {k} outer {o}', **tol)


def om_fields(f, t, skipna):
  from tests.test_ens_exact_gpu import _oracle_fields
  return _oracle_fields(f, t, skipna)


K3_CASES = [c for c in eg.CASES if c.kernel == 'k3' and c.slabs != 'zgrid']


@pytest.mark.parametrize('case', K3_CASES, ids=lambda c: c.id)
def test_k3_geometry(dev, case):
  res = eg.resolve(case)
  rs = np.random.RandomState(_seed(case))
  weights = _weights(res)
  pl = _make_plan(res, dev)
  ens, truth = _k3_ensemble(res, rs, pl, weights)
  maps, sums, metrics, members, truths = run_k3(res, pl, ens, truth, dev)
  check_k3_maps(case, maps, members, truths)
  shape = (maps.shape[1], res.n_row, res.n_col)
  slots = [x.reshape(shape) for x in k3_slots(maps, case.skipna)]
  want, mags, wsum = gr.ref_sums(weights, slots)
  outer = (np.arange(N_POOL) if case.slabs == 'contiguous'
           else np.array(TABLE))
  gr.prove_tolerance(weights, slots, want, mags, int(np.argmax(outer == 0)),
                     eg.T, [0, 2])
  tag = f'{case.id}'
  gr.assert_sums(sums, want, mags, tag)
  names = list(res.regions)
  _assert_rows(metrics, k3_metrics(want, wsum, case.skipna), names, tag)
  if not case.skipna and 'to_n2' in res.regions and res.n_col - 2 >= (
      res.n_col - 1) // eg.T * eg.T:
    # the NaN at column n_col - 1 of pool slab 1 stays out of the region that
    # stops one column before it, in the same tile
    r = names.index('to_n2')
    assert np.isfinite(sums[outer == 1][:, r, [0, 2]]).all(), tag
  if not case.skipna and not case.gather:
    assert np.isnan(sums[outer == 1, names.index('global'), 0]).all(), tag
  if case.skipna and 'one_col' in res.regions and res.n_row < eg.LONG_ROWS:
    r = names.index('one_col')
    assert (sums[outer == 2, r, 6] == 0).all() and np.isnan(
        metrics[0, r, outer == 2]).all(), tag


# ---- K3t ----------------------------------------------------------------------
def _k3t_data(res, rs, pl, weights):
  """Members in [-1, 1]; every threshold halfway between two of the point's
  non-NaN members (one on either side: finite ignorance, no zero Brier or
  RPS)."""
  case = res.case
  m = case.n_member
  shape = (m, N_POOL, res.n_row, res.n_col)
  ens = rs.uniform(-1, 1, shape).astype(case.dtype)
  truth = rs.uniform(-1.5, 1.5, shape[1:]).astype(case.dtype)
  _nan_patterns(res, pl, ens, truth, weights)
  srt = np.sort(ens, axis=0)  # NaNs last
  nn = (~np.isnan(ens)).sum(0)
  k = 1 + (rs.rand(*shape[1:]) * (nn - 1)).astype(np.int64)
  lo = np.take_along_axis(srt, k[None] - 1, 0)[0]
  hi = np.take_along_axis(srt, k[None], 0)[0]
  thr = ((lo.astype(np.float64) + hi) / 2).astype(case.dtype)
  truth[truth == thr] += np.asarray(0.125, dtype=case.dtype)
  return ens, truth, thr


def k3t_oracle(case, ens, truth, thr, skipna):
  f, t, h = _ds(ens, True), _ds(truth, False), _ds(thr, False)
  with np.errstate(all='ignore'):
    return [om.compute_brier_score(f, t, h, 'realization', False, skipna),
            om.compute_brier_score(f, t, h, 'realization', True, skipna),
            om.compute_ignorance_score(f, t, h, 'realization', skipna),
            om.compute_rps_part(f, t, h, 'realization', skipna)]


def k3t_slots(maps, skipna):
  if not skipna:
    return [maps[k] for k in range(4)]
  return ([np.nan_to_num(maps[k], nan=0.0) for k in range(4)] +
          [(~np.isnan(maps[k])).astype(np.float64) for k in range(4)])


def generic_metrics(sums, wsum, skipna, kq):
  s = np.moveaxis(sums, 0, -1)
  with np.errstate(all='ignore'):
    return np.stack([
        s[:, i] / (np.where(s[:, kq + i] != 0, s[:, kq + i], np.nan) if skipna
                   else np.where(wsum != 0, wsum, np.nan)[:, None])
        for i in range(kq)])


K3T_CASES = [c for c in eg.CASES if c.kernel == 'k3t' and c.slabs != 'zgrid']


@pytest.mark.parametrize('case', K3T_CASES, ids=lambda c: c.id)
def test_k3t_geometry(dev, case):
  import torch
  from weatherbench2_amd import engine
  res = eg.resolve(case)
  rs = np.random.RandomState(_seed(case))
  weights = _weights(res)
  pl = _make_plan(res, dev)
  ens, truth, thr = _k3t_data(res, rs, pl, weights)
  p = res.n_row * res.n_col
  table = np.array(TABLE)
  contiguous = case.slabs == 'contiguous'
  outer = np.arange(N_POOL) if contiguous else table
  tab = (None if contiguous else
         torch.as_tensor(table, dtype=torch.int64, device=dev))
  d = [torch.as_tensor(x, device=dev) for x in (ens, truth, thr)]
  args = (d[0], N_POOL * p, case.n_member, tab, d[1], tab, d[2], tab,
          len(outer))
  metrics, sums = engine.ensemble_threshold_reduce(
      pl, *args, case.skipna, want_sums=True)
  maps = engine.ensemble_threshold_maps(*args, p, case.skipna).cpu().numpy()
  metrics, sums = metrics.cpu().numpy(), sums.cpu().numpy()
  for o, s in enumerate(outer):
    want = k3t_oracle(case, ens[:, s], truth[s], thr[s], case.skipna)
    for k, w in enumerate(want):
      helpers.assert_close(maps[k, o].reshape(res.n_row, res.n_col),
                           np.asarray(w['z'].data, dtype=np.float64),
                           rtol=1e-12, atol=1e-14,
                           err_msg=f'{case.id} map {k} outer {o}')
  shape = (len(outer), res.n_row, res.n_col)
  slots = [x.reshape(shape) for x in k3t_slots(maps, case.skipna)]
  want, mags, wsum = gr.ref_sums(weights, slots)
  gr.prove_tolerance(weights, slots, want, mags, int(np.argmax(outer == 0)),
                     eg.T, [0, 2, 3])
  gr.assert_sums(sums, want, mags, case.id)
  _assert_rows(metrics, generic_metrics(want, wsum, case.skipna, 4),
               list(res.regions), case.id)


# ---- K3e ----------------------------------------------------------------------
def energy_reference(case, ens, truth, weights, outer):
  """(score, spread, skill) [3, n_region, n_outer] and the proof material:
  squares in the input dtype, fsum region means, square roots, member
  means."""
  m = case.n_member
  sk = [np.stack([((ens[j, s] - truth[s]) ** 2).astype(np.float64)
                  for s in outer]) for j in range(m)]
  sp = [np.stack([((ens[j, s] - ens[j + 1, s]) ** 2).astype(np.float64)
                  for s in outer]) for j in range(m - 1)]

  def means(q):
    if case.skipna:
      slots = [np.nan_to_num(x, nan=0.0) for x in q] + [
          (~np.isnan(x)).astype(np.float64) for x in q]
    else:
      slots = list(q)
    s, mags, wsum = gr.ref_sums(weights, slots)
    with np.errstate(all='ignore'):
      if case.skipna:
        n = s[..., len(q):]
        return s[..., :len(q)] / np.where(n != 0, n, np.nan), slots, s, mags
      return s / np.where(wsum != 0, wsum, np.nan)[None, :, None], slots, s, \
          mags

  def member_mean(roots):  # [n_outer, n_region, members]
    import warnings
    with warnings.catch_warnings(), np.errstate(all='ignore'):
      warnings.simplefilter('ignore')
      return (np.nanmean(roots, -1) if case.skipna else roots.mean(-1))
  mk, slots, s, mags = means(sk)
  skill = member_mean(np.sqrt(mk))
  if m == 1:
    spread = np.zeros_like(skill)
  else:
    spread = member_mean(np.sqrt(means(sp)[0]))
  out = np.stack([skill - 0.5 * spread, spread, skill])  # [3, o, r]
  return np.moveaxis(out, 1, 2), slots, s, mags


K3E_CASES = [c for c in eg.CASES if c.kernel == 'k3e' and c.slabs != 'zgrid']


@pytest.mark.parametrize('case', K3E_CASES, ids=lambda c: c.id)
def test_k3e_geometry(dev, case):
  import torch
  from weatherbench2_amd import engine
  res = eg.resolve(case)
  rs = np.random.RandomState(_seed(case))
  weights = _weights(res)
  pl = _make_plan(res, dev)
  ens, truth = _k3_ensemble(res, rs, pl, weights)
  p = res.n_row * res.n_col
  table = np.array(TABLE)
  contiguous = case.slabs == 'contiguous'
  outer = np.arange(N_POOL) if contiguous else table
  tab = (None if contiguous else
         torch.as_tensor(table, dtype=torch.int64, device=dev))
  got = engine.energy_score(
      pl, torch.as_tensor(ens, device=dev), N_POOL * p, case.n_member, tab,
      torch.as_tensor(truth, device=dev), tab, len(outer),
      case.skipna).cpu().numpy()
  want, slots, s, mags = energy_reference(case, ens, truth, weights, outer)
  o0 = int(np.argmax(outer == 0))
  gr.prove_tolerance(weights, slots, s, mags, o0, eg.T, [0])
  # ... and the same for the metric: a doubled last column moves the skill
  # (a mean over a single column is the same under any weight)
  w2 = [w.copy() for w in weights]
  w2[0][:, -1] *= 2
  moved = energy_reference(case, ens, truth, w2, outer[o0:o0 + 1])[0]
  assert res.n_col == 1 or abs(moved[2, 0, 0] - want[2, 0, o0]) > 10 * METRIC_RTOL * abs(
      want[2, 0, o0])
  _assert_rows(got, want, list(res.regions), case.id)


# ---- n_outer past the grid's y dimension ----------------------------------------
def _zgrid_setup(case, dev):
  res = eg.resolve(case)
  pl = _make_plan(res, dev)
  weights = np.stack([w.ravel() for w in _weights(res)])  # [n_region, P]
  return res, pl, weights


def _zgrid_data(case, rs, n_outer, p):
  """Every slab different: the slabs at o >= 32768 are not copies of the
  slabs below."""
  m = case.n_member
  ens = rs.uniform(-1, 1, (m, n_outer, p)) + 0.25 * np.sin(
      np.arange(n_outer))[None, :, None]
  sign = np.where(rs.rand(n_outer, p) < 0.5, -1.0, 1.0)
  truth = sign * rs.uniform(2.5, 3.5, (n_outer, p))
  return ens.astype(case.dtype), truth.astype(case.dtype)


def _zgrid_sums(weights, slots):
  """Vectorised fold: [n_outer, n_region, K] sums and sums of |w x| (float64
  dot products of 65 points: far inside SUM_RTOL)."""
  s = np.stack([x @ weights.T for x in slots], -1)
  mags = np.stack([np.abs(x) @ np.abs(weights).T for x in slots], -1)
  return s, mags


ZGRID = {c.kernel: c for c in eg.CASES if c.slabs == 'zgrid'}
SPOT = (0, 1, 32767, 32768, 32769, eg.ZGRID_OUTER - 1)


def test_k3_grid_z(dev):
  import torch
  from weatherbench2_amd import _lib, engine
  case = ZGRID['k3']
  lib = _lib.load()
  res, pl, weights = _zgrid_setup(case, dev)
  n_outer, p, m = case.n_outer, res.n_row * res.n_col, case.n_member
  ens, truth = _zgrid_data(case, np.random.RandomState(5), n_outer, p)
  d_ens = torch.as_tensor(ens, device=dev)
  d_truth = torch.as_tensor(truth, device=dev)
  k = lib.wb2_ens_num_slots(int(case.skipna))
  seg_eoff, n_ts = pl.seg_entries(eg.T)
  partials = torch.full((n_outer, pl.n_chunk, pl.nwf, n_ts, k), float('nan'),
                        dtype=torch.float64, device=dev)
  maps = torch.full((6, n_outer, p), SENTINEL, dtype=torch.float64,
                    device=dev)
  stream = engine.current_stream_ptr(dev)
  _lib.check(lib.wb2_ens_partials_maps(
      _lib.WB2_F32, int(case.skipna), _lib.ptr(d_ens), None, _lib.ptr(d_truth),
      None, m, n_outer * p, n_outer, pl.n_row, pl.n_col, _lib.ptr(pl.w_row),
      _lib.ptr(pl.w_col), _lib.ptr(pl.wfield), _lib.ptr(pl.chunk_row0),
      _lib.ptr(pl.chunk_nrow), pl.n_chunk, -(-pl.n_col // eg.T),
      _lib.ptr(pl.seg_col0), _lib.ptr(seg_eoff), pl.n_seg, n_ts,
      _lib.ptr(partials), _lib.ptr(maps), stream), 'wb2_ens_partials_maps')
  sums = torch.full((n_outer, pl.n_region, k), float('nan'),
                    dtype=torch.float64, device=dev)
  metrics = torch.empty((_lib.NMETRIC_ENS, pl.n_region, n_outer),
                        dtype=torch.float64, device=dev)
  _lib.check(lib.wb2_ens_combine(
      int(case.skipna), _lib.ptr(partials), n_outer, pl.n_chunk, pl.nwf,
      pl.n_seg, _lib.ptr(seg_eoff), n_ts, _lib.ptr(pl.band_chunk0), pl.n_band,
      _lib.ptr(pl.coef_band), _lib.ptr(pl.coef_seg), _lib.ptr(pl.region_wf),
      _lib.ptr(pl.region_wsum), pl.n_region, _lib.ptr(sums),
      _lib.ptr(metrics), stream), 'wb2_ens_combine')
  maps = maps.cpu().numpy()
  assert not (maps == SENTINEL).any(), np.argwhere(maps == SENTINEL)[0]
  shape = (1, res.n_row, res.n_col)
  check_k3_maps(case, maps[:, list(SPOT)],
                [ens[:, o].reshape((m,) + shape[1:]) for o in SPOT],
                truth[list(SPOT)].reshape((-1,) + shape[1:]))
  want, mags = _zgrid_sums(weights, k3_slots(maps, case.skipna))
  gr.assert_sums(sums.cpu().numpy(), want, mags, case.id)
  _assert_rows(metrics.cpu().numpy(),
               k3_metrics(want, weights.sum(1), case.skipna),
               list(res.regions), case.id)


def test_k3t_grid_z(dev):
  import torch
  from weatherbench2_amd import _lib, engine
  case = ZGRID['k3t']
  lib = _lib.load()
  res, pl, weights = _zgrid_setup(case, dev)
  n_outer, p, m = case.n_outer, res.n_row * res.n_col, case.n_member
  rs = np.random.RandomState(6)
  ens, _ = _zgrid_data(case, rs, n_outer, p)
  srt = np.sort(ens, axis=0)
  thr = ((srt[0].astype(np.float64) + srt[1]) / 2).astype(case.dtype)
  truth = rs.uniform(-1.5, 1.5, (n_outer, p)).astype(case.dtype)
  ens[0, n_outer - 1, 3] = np.nan
  d = [torch.as_tensor(x, device=dev) for x in (ens, truth, thr)]
  kq = 4
  k = lib.wb2_num_slots(_lib.MODE_ENS_THR, int(case.skipna))
  seg_eoff, n_ts = pl.seg_entries(eg.T)
  partials = torch.full((n_outer, pl.n_chunk, pl.nwf, n_ts, k), float('nan'),
                        dtype=torch.float64, device=dev)
  stream = engine.current_stream_ptr(dev)
  _lib.check(lib.wb2_ens_threshold_partials(
      _lib.WB2_F32, int(case.skipna), _lib.ptr(d[0]), None, _lib.ptr(d[1]),
      None, _lib.ptr(d[2]), None, m, n_outer * p, n_outer, pl.n_row, pl.n_col,
      _lib.ptr(pl.w_row), _lib.ptr(pl.w_col), _lib.ptr(pl.wfield),
      _lib.ptr(pl.chunk_row0), _lib.ptr(pl.chunk_nrow), pl.n_chunk,
      -(-pl.n_col // eg.T), _lib.ptr(pl.seg_col0), _lib.ptr(seg_eoff),
      pl.n_seg, n_ts, _lib.ptr(partials), stream),
      'wb2_ens_threshold_partials')
  sums = torch.full((n_outer, pl.n_region, k), float('nan'),
                    dtype=torch.float64, device=dev)
  metrics = torch.empty((kq, pl.n_region, n_outer), dtype=torch.float64,
                        device=dev)
  _lib.check(lib.wb2_det_combine(
      _lib.MODE_ENS_THR, int(case.skipna), _lib.ptr(partials), n_outer,
      pl.n_chunk, pl.nwf, pl.n_seg, _lib.ptr(seg_eoff), n_ts,
      _lib.ptr(pl.band_chunk0), pl.n_band, _lib.ptr(pl.coef_band),
      _lib.ptr(pl.coef_seg), _lib.ptr(pl.region_wf), _lib.ptr(pl.region_wsum),
      pl.n_region, _lib.ptr(sums), _lib.ptr(metrics), stream),
      'wb2_det_combine')
  maps = engine.ensemble_threshold_maps(
      d[0], n_outer * p, m, None, d[1], None, d[2], None, n_outer, p,
      case.skipna).cpu().numpy()
  for o in SPOT:
    want = k3t_oracle(case, ens[:, o].reshape(m, 1, p), truth[o].reshape(1, p),
                      thr[o].reshape(1, p), case.skipna)
    for j, w in enumerate(want):
      helpers.assert_close(maps[j, o], np.asarray(w['z'].data).ravel(),
                           rtol=1e-12, atol=1e-14, err_msg=f'map {j} {o}')
  want, mags = _zgrid_sums(weights, k3t_slots(maps, case.skipna))
  gr.assert_sums(sums.cpu().numpy(), want, mags, case.id)
  _assert_rows(metrics.cpu().numpy(),
               generic_metrics(want, weights.sum(1), case.skipna, kq),
               list(res.regions), case.id)


def test_k3e_grid_z(dev):
  import ctypes
  import torch
  from weatherbench2_amd import _lib, engine
  case = ZGRID['k3e']
  lib = _lib.load()
  res, pl, weights = _zgrid_setup(case, dev)
  n_outer, p, m = case.n_outer, res.n_row * res.n_col, case.n_member
  ens, truth = _zgrid_data(case, np.random.RandomState(7), n_outer, p)
  block, n_block, k = (ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32())
  _lib.check(lib.wb2_energy_layout(
      m, int(case.skipna), 0, ctypes.byref(block), ctypes.byref(n_block),
      ctypes.byref(k)), 'wb2_energy_layout')
  tables, keep = engine.plan_tables(pl, eg.T, pl.wfield)
  n_virtual = n_outer * n_block.value
  nan = float('nan')
  partials = torch.full((n_virtual, pl.n_chunk, pl.nwf, keep[3], k.value),
                        nan, dtype=torch.float64, device=dev)
  means = torch.full((2 * block.value, pl.n_region, n_virtual), nan,
                     dtype=torch.float64, device=dev)
  out = torch.full((3, pl.n_region, n_outer), nan, dtype=torch.float64,
                   device=dev)
  d_ens = torch.as_tensor(ens, device=dev)
  d_truth = torch.as_tensor(truth, device=dev)
  _lib.check(lib.wb2_energy_score(
      _lib.WB2_F64, int(case.skipna), _lib.ptr(d_ens), None, _lib.ptr(d_truth),
      None, m, n_outer * p, n_outer, ctypes.byref(tables), _lib.ptr(partials),
      _lib.ptr(means), _lib.ptr(out), engine.current_stream_ptr(dev)),
      'wb2_energy_score')
  got = out.cpu().numpy()
  del keep
  wsum = weights.sum(1)
  sk = np.sqrt(np.einsum('mop,rp->mor', (ens - truth[None]) ** 2, weights) /
               wsum)
  sp = np.sqrt(np.einsum('mop,rp->mor', (ens[:-1] - ens[1:]) ** 2, weights) /
               wsum)
  skill, spread = sk.mean(0), sp.mean(0)  # [n_outer, n_region]
  want = np.moveaxis(np.stack([skill - 0.5 * spread, spread, skill]), 1, 2)
  _assert_rows(got, want, list(res.regions), case.id)

