"""The map kernels and running means across vector, tail and grid edges (-m gpu).

spatial_maps_kernel, spatial_accumulate_kernel, spatial_accumulate_addr_kernel
(K5), seeps_map_kernel, time_accumulate_kernel and gather_accumulate_kernel,
called through the C ABI over the sweep of tests/map_geometry_cases.py (its
reach is asserted on the CPU by test_map_geometry_cpu.py), against the
bit-exact references of tests/geometry_reference.py:

  * maps: NumPy in the input dtype, bit for bit (NaN in the same places);
  * sums: a float64 loop in time order from the accumulator's value, a skipped
    value adding 0.0, bit for bit, counts included;
  * SEEPS: the per-point restatement of oracle/metrics_np.SpatialSEEPS in the
    input dtype (tied to the oracle by test_map_geometry_cpu.py), bit for bit.

Every buffer a kernel reads or writes sits inside a larger allocation with at
least 8 slabs or 64 elements of sentinel on each side; whole allocations are
compared, so a write outside what a call addresses fails like a wrong value.
Accumulators start from random non-zero values, and every accumulating case
runs three ways -- all steps in one call, one step per call, 3 + (T - 3) steps
-- which must all give the reference's bits.  The data spread over 1e-6 ... 1e6,
so each case shows on the reference that a U group summed pairwise or
reversed, or a dropped or doubled last step, would change a bit.
"""
import ctypes
import zlib

import numpy as np
import pytest

from tests import geometry_reference as gr
from tests import map_geometry_cases as mc

pytestmark = pytest.mark.gpu

GUARD_MIN = 64
GUARD_SLABS = 8
SENTINEL = -12345.6875  # exact in float32 and float64
DRY = 0.25 / 1000.0     # SpatialSEEPS' default dry threshold, in metres
CODE = {'float32': 0, 'float64': 1}
FINITE_KINDS = ('f nan', 't nan', 'both nan', 'inf - inf')
# a SEEPS thread stores only the slabs of its group below n_outer: the guard
# after the map holds a whole group's padding
assert GUARD_SLABS >= mc.SEEPS_SLABS - 1


@pytest.fixture(scope='module')
def dev():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  return torch.device('cuda')


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import _lib
  return _lib.load()


def _stream(dev):
  import torch
  return torch.cuda.current_stream(dev).cuda_stream


def _sync():
  import torch
  torch.cuda.synchronize()


class Buf:
  """`data` (flattened) on the device inside a larger allocation: `guard`
  elements of `sentinel` on each side and `shift` more before the data (one
  element: the data start 4 or 8 bytes off 16)."""

  def __init__(self, dev, data, guard=GUARD_MIN, shift=0, sentinel=SENTINEL):
    import torch
    data = np.ascontiguousarray(data).ravel()
    self.n = data.size
    self.lo = max(guard, GUARD_MIN) + shift
    full = np.full(self.lo + self.n + max(guard, GUARD_MIN), sentinel,
                   dtype=data.dtype)
    full[self.lo:self.lo + self.n] = data
    self.init = full
    self.t = torch.from_numpy(full).to(dev)
    self.esize = data.itemsize

  @property
  def ptr(self):
    return self.t.data_ptr() + self.lo * self.esize

  def addr(self, i):
    return self.ptr + int(i) * self.esize

  def reset(self):
    import torch
    self.t.copy_(torch.from_numpy(self.init))

  def host(self):
    return self.t.cpu().numpy()

  def expect(self, data=None, at=None):
    """The whole allocation as it must be: the initial contents with `data`
    in place of the data (or at the flat positions `at`)."""
    full = self.init.copy()
    if data is not None:
      if at is None:
        full[self.lo:self.lo + self.n] = np.asarray(data).ravel()
      else:
        full[self.lo + np.asarray(at).ravel()] = np.asarray(data).ravel()
    return full


def _rs(case, salt=''):
  return np.random.RandomState(zlib.crc32((case.id + salt).encode()))


def spread(rs, shape, dtype, lo=-6.0, hi=6.0):
  """Random signs, magnitudes log-uniform over 10**lo ... 10**hi."""
  shape = tuple(np.atleast_1d(shape))
  sign = np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)
  return (sign * 10.0 ** rs.uniform(lo, hi, shape)).astype(dtype)


def inject(pool, which):
  """NaN / +inf at every fourth point (p % 4 == 1), by kind (slab + p // 4) %
  5 + 1: 1 forecast NaN, 2 truth NaN, 3 both, 4 both +inf (inf - inf = NaN),
  5 forecast +inf.  Slabs of the same index in the forecast and truth pools
  meet every kind (point 1 of 4 slabs, or points 1, 5, 9, 13 of one); the
  other points stay finite, so without skipna most sums are not NaN."""
  n_slab, n_point = pool.shape
  p = np.arange(n_point)[None, :]
  k = np.where(p % 4 == 1, (np.arange(n_slab)[:, None] + p // 4) % 5 + 1, 0)
  nan = (k == 3) | (k == (1 if which == 'f' else 2))
  inf = (k == 4) | ((k == 5) & (which == 'f'))
  out = pool.copy()
  out[nan] = np.nan
  out[inf] = np.inf
  return out


def meets_every_kind(n_slab, n_point):
  """Whether inject() gives identity-table steps every kind of NaN."""
  return n_point >= 2 and (n_slab >= 4 or n_point >= 14)


def start_sums(rs, shape):
  """Non-zero accumulators: random signs, magnitudes 1e-3 ... 1e3."""
  return spread(rs, shape, np.float64, -3.0, 3.0)


def start_counts(rs, shape):
  return rs.randint(1, 1000, size=shape).astype(np.float64)


def show_order(case, start, steps, u):
  """gr.prove_order on the case's data; returns the start used.  Spread data
  show the time order on most elements, but a case of one or two elements may
  need other start values: the starts of the elements without NaN steps are
  redrawn (seeded by the case) until every variant shows."""
  rs = _rs(case, 'order')
  start = np.array(start, copy=True)
  ok = np.ones(start.shape, bool)
  if not case.skipna:
    for x in steps:
      ok &= ~np.isnan(x)
  for _ in range(100):
    try:
      gr.prove_order(start, steps, case.skipna, u, case.id)
      return start
    except AssertionError:
      if not ok.any():
        raise
      start[ok] = spread(rs, int(ok.sum()), np.float64)
  gr.prove_order(start, steps, case.skipna, u, case.id)
  return start


def splits(n_time):
  """All steps in one call, one step per call, 3 + (T - 3)."""
  out = [((0, n_time),)]
  if n_time > 1:
    out.append(tuple((i, i + 1) for i in range(n_time)))
  if n_time > 3:
    out.append(((0, 3), (3, n_time)))
  return out


def pick_vec(dtype, n_point, ptrs):
  """pick_vec of spatial_maps.hip on real addresses (null outputs pass)."""
  w = mc.W[dtype]
  ok = n_point % w == 0 and all(p % 16 == 0 for p in ptrs)
  return w if ok else 1


def _vp(x):
  return None if x is None else ctypes.c_void_p(x)


# ---- K5: maps ----------------------------------------------------------------
def slab_tables(case, rs, n_slab, n_rest):
  """(f table, f pool size, t table, t pool size); a table is None for the
  identity.  'perm': forecast slabs permuted and repeated; 'bcast': truth
  slab j of every time step (one truth slab per rest index)."""
  if case.tables == 'perm':
    n_pool = max(1, (n_slab + 1) // 2)
    return rs.permutation(n_slab) % n_pool, n_pool, None, n_slab
  if case.tables == 'bcast':
    return None, n_slab, np.arange(n_slab) % n_rest, n_rest
  return None, n_slab, None, n_slab


def table_buf(dev, tab):
  # guards of 0: a stray read there still names a slab inside the pool
  return None if tab is None else Buf(dev, tab.astype(np.int64), sentinel=0)


def pools(case, rs, n_f, n_t):
  dt = np.dtype(case.dtype)
  fp = spread(rs, (n_f, case.n_point), dt)
  tp = spread(rs, (n_t, case.n_point), dt)
  if case.nan:
    fp, tp = inject(fp, 'f'), inject(tp, 't')
  return fp, tp


def guard_of(case):
  return max(GUARD_MIN, GUARD_SLABS * case.n_point)


def run_maps(case, dev, lib):
  rs = _rs(case)
  n, n_outer = case.n_point, case.n_outer
  rest = 2 if n_outer % 2 == 0 else 1
  ftab, n_f, ttab, n_t = slab_tables(case, rs, n_outer, rest)
  fp, tp = pools(case, rs, n_f, n_t)
  g = guard_of(case)
  fb = Buf(dev, fp, g, shift=int(case.misalign == 'f'))
  tb = Buf(dev, tp, g, shift=int(case.misalign == 't'))
  fk, tk = table_buf(dev, ftab), table_buf(dev, ttab)
  outs = {}
  for key, name in zip('bms', mc.OUTS):
    if key in case.outs:
      # the whole map starts as the sentinel: an element left unwritten fails
      outs[name] = Buf(dev, np.full(n_outer * n, SENTINEL, fp.dtype), g,
                       shift=int(case.misalign == name), sentinel=SENTINEL)
  ptrs = [outs[k].ptr if k in outs else None for k in mc.OUTS]
  assert pick_vec(case.dtype, n, [fb.ptr, tb.ptr] +
                  [p for p in ptrs if p is not None]) == case.vec
  rc = lib.wb2_spatial_maps(CODE[case.dtype], fb.ptr, fk and fk.ptr, tb.ptr,
                            tk and tk.ptr, n_outer, n, *[_vp(p) for p in ptrs],
                            _stream(dev))
  assert rc == 0, lib.wb2_last_error()
  _sync()
  f = fp[ftab] if ftab is not None else fp
  t = tp[ttab] if ttab is not None else tp
  want = dict(zip(mc.OUTS, gr.spatial_maps(f, t)))
  for name, b in outs.items():
    gr.assert_bits(b.host(), b.expect(want[name]), f'{case.id} {name}')
  for b in (fb, tb) + tuple(x for x in (fk, tk) if x is not None):
    gr.assert_bits(b.host(), b.init, f'{case.id} input changed')


# ---- K5: accumulate ------------------------------------------------------------
def acc_steps(f, t, skipna):
  """Per time step the three float64 terms (d, d^2, |d|), NaN where d is."""
  d, d2, ad = gr.spatial_maps(f, t)
  return [np.stack([x[i] for x in (d, d2, ad)]).astype(np.float64)
          for i in range(f.shape[0])]


def kinds_met(f, t):
  """Which of FINITE_KINDS the steps meet (d = f - t NaN for each reason)."""
  with np.errstate(all='ignore'):
    seen = set()
    if (np.isnan(f) & ~np.isnan(t)).any():
      seen.add('f nan')
    if (~np.isnan(f) & np.isnan(t)).any():
      seen.add('t nan')
    if (np.isnan(f) & np.isnan(t)).any():
      seen.add('both nan')
    if (np.isinf(f) & np.isinf(t) & (np.sign(f) == np.sign(t))).any():
      seen.add('inf - inf')
  return seen


def check_sums(case, steps, start, count0, got_sum, got_count, tag):
  want, wc = gr.running_sum(start, steps, case.skipna,
                            None if count0 is None else count0)
  gr.assert_bits(got_sum, want, f'{tag} sums')
  if count0 is not None:
    gr.assert_bits(got_count, wc, f'{tag} counts')
  return want, wc


def run_acc(case, dev, lib):
  rs = _rs(case)
  n, n_rest, n_time = case.n_point, case.n_outer, case.n_time
  n_slab = n_time * n_rest
  ftab, n_f, ttab, n_t = slab_tables(case, rs, n_slab, n_rest)
  fp, tp = pools(case, rs, n_f, n_t)
  g = guard_of(case)
  fb = Buf(dev, fp, g, shift=int(case.misalign == 'f'))
  tb = Buf(dev, tp, g, shift=int(case.misalign == 't'))
  fk, tk = table_buf(dev, ftab), table_buf(dev, ttab)
  assert pick_vec(case.dtype, n, [fb.ptr, tb.ptr]) == case.vec
  f = (fp[ftab] if ftab is not None else fp).reshape(n_time, n_rest, n)
  t = (tp[ttab] if ttab is not None else tp).reshape(n_time, n_rest, n)
  if case.skipna and case.nan and case.tables == '' and meets_every_kind(
      n_slab, n):
    assert kinds_met(f, t) == set(FINITE_KINDS), case.id
  steps = acc_steps(f, t, case.skipna)  # [3, n_rest, n] per step
  start = start_sums(rs, (3, n_rest, n))
  count0 = start_counts(rs, (3, n_rest, n)) if case.skipna else None
  start = show_order(case, start, steps, mc.U)
  sb = Buf(dev, start, g)
  cb = Buf(dev, count0, g) if case.skipna else None
  for parts in splits(n_time):
    sb.reset()
    if cb is not None:
      cb.reset()
    for a, b in parts:
      fa = fk.addr(a * n_rest) if fk else None
      ta = tk.addr(a * n_rest) if tk else None
      fptr = fb.ptr if fk else fb.addr(a * n_rest * n)
      tptr = tb.ptr if tk else tb.addr(a * n_rest * n)
      rc = lib.wb2_spatial_accumulate(
          CODE[case.dtype], int(case.skipna), fptr, fa, tptr, ta, b - a,
          n_rest, n, sb.ptr, cb and cb.ptr, _stream(dev))
      assert rc == 0, lib.wb2_last_error()
    _sync()
    want, wc = gr.running_sum(start, steps, case.skipna, count0)
    tag = f'{case.id} split {len(parts)}'
    gr.assert_bits(sb.host(), sb.expect(want), f'{tag} sums')
    if cb is not None:
      gr.assert_bits(cb.host(), cb.expect(wc), f'{tag} counts')
      inc = cb.host()[cb.lo:cb.lo + cb.n].reshape(3, -1) - count0.reshape(3, -1)
      assert (inc == inc[0]).all(), f'{tag}: count planes differ'
  for b in (fb, tb) + tuple(x for x in (fk, tk) if x is not None):
    gr.assert_bits(b.host(), b.init, f'{case.id} input changed')


# ---- K5: accumulate by address -----------------------------------------------
N_ALLOC = 3


def run_addr(case, dev, lib):
  rs = _rs(case)
  n, n_dst, n_time = case.n_point, case.n_outer, case.n_time
  dt = np.dtype(case.dtype)
  n_slab = n_time * n_dst
  g = guard_of(case)
  shift = int(case.aligned16 == 'off')
  fp, tp = pools(case, rs, n_slab, n_slab)
  # slab s = i * n_dst + j of each pool lives in allocation s % N_ALLOC at
  # position s // N_ALLOC
  s = np.arange(n_slab)
  fbufs = [Buf(dev, fp[s % N_ALLOC == k], g, shift) for k in range(N_ALLOC)]
  tbufs = [Buf(dev, tp[s % N_ALLOC == k], g, shift) for k in range(N_ALLOC)]

  def slab_addr(bufs, slab):
    base = np.array([b.ptr for b in bufs], dtype=np.int64)
    return base[slab % N_ALLOC] + (slab // N_ALLOC) * n * dt.itemsize
  fslab = s.reshape(n_time, n_dst).copy()
  tslab = s.reshape(n_time, n_dst).copy()
  if n_dst >= 2:  # addresses repeated across destinations
    fslab[:, -1] = fslab[:, 0]
    tslab[:, 1::2] = tslab[:, 0:-1:2][:, :tslab[:, 1::2].shape[1]]
  fa = Buf(dev, slab_addr(fbufs, fslab), sentinel=fbufs[0].ptr)
  ta = Buf(dev, slab_addr(tbufs, tslab), sentinel=tbufs[0].ptr)
  f = fp[fslab].reshape(n_time, n_dst, n)
  t = tp[tslab].reshape(n_time, n_dst, n)
  steps = acc_steps(f, t, case.skipna)
  if case.skipna and n_dst == 1 and meets_every_kind(n_slab, n):
    assert kinds_met(f, t) == set(FINITE_KINDS), case.id
  start = start_sums(rs, (3, n_dst, n))
  count0 = start_counts(rs, (3, n_dst, n))
  start = show_order(case, start, steps, mc.U)
  # per wanted kind one sum (and count) allocation of n_dst + 1 slabs, the
  # destinations permuted, one slab never addressed; sums 8 bytes off 16
  wanted = [m for m, key in enumerate('bms') if key in case.outs]
  perm = rs.permutation(n_dst + 1)[:n_dst]
  sums, counts = {}, {}
  sum_tab = np.zeros((3, n_dst), np.int64)
  count_tab = np.zeros((3, n_dst), np.int64)
  pos = (perm[:, None] * n + np.arange(n)[None, :])  # [n_dst, n]
  for m in wanted:
    filler = start_sums(rs, (n_dst + 1, n))
    filler.reshape(-1)[pos.ravel()] = start[m].ravel()
    sums[m] = Buf(dev, filler, g, shift=int(case.sum_off))
    sum_tab[m] = sums[m].ptr + perm * n * 8
    if case.skipna:
      cf = start_counts(rs, (n_dst + 1, n))
      cf.reshape(-1)[pos.ravel()] = count0[m].ravel()
      counts[m] = Buf(dev, cf, g)
      count_tab[m] = counts[m].ptr + perm * n * 8
  if case.sum_off:
    assert all(sums[m].ptr % 16 == 8 for m in wanted)
  sa = Buf(dev, sum_tab, sentinel=0)
  ca = Buf(dev, count_tab, sentinel=0) if case.skipna else None
  flag = int(case.aligned16 in ('yes', 'ragged'))
  if case.aligned16 == 'yes':
    assert (fa.init[fa.lo:fa.lo + fa.n] % 16 == 0).all()
    assert (ta.init[ta.lo:ta.lo + ta.n] % 16 == 0).all()
  elif case.aligned16 == 'off':
    assert (fa.init[fa.lo:fa.lo + fa.n] % 16 != 0).all()
  want, wc = gr.running_sum(start, steps, case.skipna, count0)
  for parts in splits(n_time):
    for b in list(sums.values()) + list(counts.values()):
      b.reset()
    for a, b in parts:
      rc = lib.wb2_spatial_accumulate_addr(
          CODE[case.dtype], int(case.skipna), flag, fa.addr(a * n_dst),
          ta.addr(a * n_dst), b - a, n_dst, n, sa.ptr, ca and ca.ptr,
          _stream(dev))
      assert rc == 0, lib.wb2_last_error()
    _sync()
    tag = f'{case.id} split {len(parts)}'
    for m in wanted:
      gr.assert_bits(sums[m].host(), sums[m].expect(want[m], pos), f'{tag} sums')
      if case.skipna:
        gr.assert_bits(counts[m].host(), counts[m].expect(wc[m], pos),
                       f'{tag} counts')
  for b in fbufs + tbufs + [fa, ta, sa] + ([ca] if ca else []):
    gr.assert_bits(b.host(), b.init, f'{case.id} input changed')
  if case.outs == 'bms':
    # the same data through wb2_spatial_accumulate: the same bits
    fb = Buf(dev, f, g)
    tb = Buf(dev, t, g)
    sb = Buf(dev, start, g)
    cb = Buf(dev, count0, g) if case.skipna else None
    rc = lib.wb2_spatial_accumulate(
        CODE[case.dtype], int(case.skipna), fb.ptr, None, tb.ptr, None, n_time,
        n_dst, n, sb.ptr, cb and cb.ptr, _stream(dev))
    assert rc == 0, lib.wb2_last_error()
    _sync()
    got = sb.host()[sb.lo:sb.lo + sb.n].reshape(3, n_dst, n)
    for m in wanted:
      addr_got = sums[m].host()[sums[m].lo:][pos.ravel()].reshape(n_dst, n)
      gr.assert_bits(got[m], addr_got, f'{case.id}: wb2_spatial_accumulate')


# ---- SEEPS map ---------------------------------------------------------------
def seeps_inputs(case, rs):
  """(forecast, truth, wet pool, wet table, p1): values below the dry
  threshold, exactly on it, between it and the wet threshold, exactly on the
  wet threshold and above it; NaN forecasts and truths; p1 in (0.1, 0.85) or
  NaN (masked)."""
  dt = np.dtype(case.dtype)
  n, n_outer = case.n_point, case.n_outer
  n_valid = 3 if case.tables == 'wet' else n_outer
  wet_pool = rs.uniform(0.002, 0.02, (n_valid, n)).astype(dt)
  wtab = (np.arange(n_outer) // 2) % n_valid if case.tables == 'wet' else None
  wet = wet_pool[wtab] if wtab is not None else wet_pool

  def values():
    c = rs.randint(0, 6 if case.nan else 5, size=(n_outer, n))
    v = np.empty((n_outer, n), dt)
    dry = dt.type(DRY)
    v[c == 0] = rs.uniform(0.0, DRY * 0.9, (c == 0).sum()).astype(dt)
    v[c == 1] = dry
    mid = rs.uniform(0.0, 1.0, (n_outer, n))
    between = (dry * 1.1 + mid * (wet - dry * 1.1) * 0.9).astype(dt)
    v[c == 2] = between[c == 2]
    v[c == 3] = wet[c == 3]
    v[c == 4] = (wet * 1.5).astype(dt)[c == 4]
    v[c == 5] = np.nan
    return v
  f, y = values(), values()
  p1 = rs.uniform(0.1, 0.85, n)
  p1[(p1 <= 0.1) | (p1 >= 0.85)] = 0.5
  if case.nan:
    p1[np.arange(n) % 5 == 2] = np.nan
  return f, y, wet_pool, wtab, p1


def run_seeps(case, dev, lib):
  rs = _rs(case)
  n, n_outer = case.n_point, case.n_outer
  dt = np.dtype(case.dtype)
  f, y, wet_pool, wtab, p1 = seeps_inputs(case, rs)
  g = guard_of(case)
  aux = Buf(dev, p1)
  # sentinel, not 0: many scores are exactly 0, an unwritten one must fail
  out = Buf(dev, np.full(n_outer * n, SENTINEL), g)
  keep = [aux]
  if case.entry == 'in':
    fb, yb, wb = Buf(dev, f, g), Buf(dev, y, g), Buf(dev, wet_pool, g)
    wk = table_buf(dev, wtab)
    keep += [fb, yb, wb] + ([wk] if wk else [])
    ins = (ctypes.c_void_p * 3)(fb.ptr, yb.ptr, wb.ptr)
    tabs = (ctypes.c_void_p * 3)(None, None, wk.ptr if wk else None)
    rc = lib.wb2_seeps_map(CODE[case.dtype], ins, tabs, n_outer, n, aux.ptr,
                           DRY, out.ptr, _stream(dev))
  else:
    # slabs in different allocations: forecast slab o in allocation o % 2,
    # truth slab o in allocation (o + 1) % 2, wet thresholds by table
    o = np.arange(n_outer)
    fbs = [Buf(dev, f[o % 2 == k], g) for k in range(2)]
    ybs = [Buf(dev, y[(o + 1) % 2 == k], g) for k in range(2)]
    wb = Buf(dev, wet_pool, g)
    slab = n * dt.itemsize
    fad = np.where(o % 2 == 0, fbs[0].ptr, fbs[1].ptr) + (o // 2) * slab
    yad = (np.where((o + 1) % 2 == 0, ybs[0].ptr, ybs[1].ptr) +
           (o // 2) * slab)
    wad = wb.ptr + (wtab if wtab is not None else o) * slab
    tabs_b = [Buf(dev, x.astype(np.int64), sentinel=int(x[0]))
              for x in (fad, yad, wad)]
    keep += fbs + ybs + [wb] + tabs_b
    tabs = (ctypes.c_void_p * 3)(*[b.ptr for b in tabs_b])
    rc = lib.wb2_seeps_map_addr(CODE[case.dtype], tabs, n_outer, n, aux.ptr,
                                DRY, out.ptr, _stream(dev))
  assert rc == 0, lib.wb2_last_error()
  _sync()
  wet = wet_pool[wtab] if wtab is not None else wet_pool
  want = gr.seeps_map(f, y, wet, p1, DRY, dt)
  if n_outer * n >= 64:  # NaNs, scores of 0 and above
    assert np.isnan(want).any() and (want == 0).any() and (want > 0).any()
  gr.assert_bits(out.host(), out.expect(want), case.id)
  for b in keep:
    gr.assert_bits(b.host(), b.init, f'{case.id} input changed')


# ---- time_accumulate ---------------------------------------------------------
def run_time(case, dev, lib):
  rs = _rs(case)
  n_lead, n_time, n_tail = case.n_outer, case.n_time, case.n_tail
  dt = np.dtype(case.dtype)
  nel = n_lead * n_tail
  v = spread(rs, (n_lead, n_time, n_tail), dt)
  if case.nan:
    # every fourth element, at every third step
    e = np.arange(nel).reshape(n_lead, 1, n_tail)
    t = np.arange(n_time).reshape(1, n_time, 1)
    v[(e % 4 == 1) & ((e // 4 + t) % 3 == 0)] = np.nan
  # the accumulator: larger than the result; dst sends runs of `run` result
  # elements to a permutation of its runs (identity for 'plain')
  run = case.run
  n_acc = nel + 3 * run
  if case.entry == 'plain':
    dst_el = np.arange(nel)
    dst = None
  else:
    slots = rs.permutation(n_acc // run)[:nel // run]
    dst = slots * run
    dst_el = (dst[:, None] + np.arange(run)[None, :]).ravel()
  g = max(GUARD_MIN, 8 * run)
  start = start_sums(rs, n_acc)
  count0 = start_counts(rs, n_acc)
  with_count = case.skipna or case.entry == 'plain'
  steps = [v[:, i, :].ravel() for i in range(n_time)]
  start[dst_el] = show_order(case, start[dst_el], steps, mc.U_TIME)
  sb = Buf(dev, start, g)
  cb = Buf(dev, count0, g) if with_count else None
  db = None if dst is None else Buf(dev, dst.astype(np.int64), sentinel=0)
  ws, wc = gr.running_sum(start[dst_el], steps, case.skipna, count0[dst_el])
  for parts in splits(n_time):
    sb.reset()
    if cb is not None:
      cb.reset()
    for a, b in parts:
      vb = Buf(dev, np.ascontiguousarray(v[:, a:b, :]))
      if case.entry == 'plain':
        rc = lib.wb2_time_accumulate(vb.ptr, n_lead, b - a, n_tail,
                                     int(case.skipna), sb.ptr, cb and cb.ptr,
                                     _stream(dev))
      elif case.entry == 'scatter':
        rc = lib.wb2_time_accumulate_scatter(
            CODE[case.dtype], vb.ptr, n_lead, b - a, n_tail, int(case.skipna),
            db.ptr, sb.ptr, cb and cb.ptr, _stream(dev))
      else:
        rc = lib.wb2_time_accumulate_runs(
            CODE[case.dtype], vb.ptr, n_lead, b - a, n_tail, int(case.skipna),
            db.ptr, run, sb.ptr, cb and cb.ptr, _stream(dev))
      assert rc == 0, lib.wb2_last_error()
      _sync()
      gr.assert_bits(vb.host(), vb.init, f'{case.id} values changed')
    tag = f'{case.id} split {len(parts)}'
    gr.assert_bits(sb.host(), sb.expect(ws, dst_el), f'{tag} sums')
    if cb is not None:
      gr.assert_bits(cb.host(), cb.expect(wc, dst_el), f'{tag} counts')


# ---- gather_accumulate -------------------------------------------------------
N_ROWS = 3


def gather_arena(rs, n):
  """float64 values whose float32 rounding differs: random magnitudes, and
  exact ties between two float32 neighbours (round half to even)."""
  a = spread(rs, n, np.float64)
  f = spread(rs, n, np.float32).astype(np.float64)
  up = np.nextafter(f.astype(np.float32), np.float32(np.inf)).astype(np.float64)
  tie = (f + up) / 2.0  # exact in float64
  a[::3] = tie[::3]
  return a


def run_gather(case, dev, lib):
  rs = _rs(case)
  n_out, n_time = case.n_outer, case.n_time
  n_arena = 4 * n_out * n_time + 5
  arena = gather_arena(rs, n_arena)
  src = rs.randint(0, n_arena, size=(n_out, n_time)).astype(np.int32)
  if case.nan:
    e, t = np.arange(n_out)[:, None], np.arange(n_time)[None, :]
    src[(e % 4 == 1) & ((e // 4 + t) % 3 == 0)] = -1
  r32 = (rs.rand(n_out) < 0.5).astype(np.uint8)
  r32[0] = 1
  vals = arena[np.maximum(src, 0)]
  vals[src < 0] = np.nan
  vals = np.where(r32[:, None] == 1, vals.astype(np.float32).astype(np.float64),
                  vals)
  # the rounding itself changes values (not only the NaN fills)
  rounded = (r32[:, None] == 1) & (src >= 0)
  assert (vals != arena[np.maximum(src, 0)])[rounded].any()
  # accumulators: elements spread over N_ALLOC sum and N_ALLOC count
  # allocations of row_len[k] * N_ROWS doubles, at distinct permuted positions
  alloc = np.arange(n_out) % N_ALLOC
  row_len = [int((alloc == k).sum()) + 2 for k in range(N_ALLOC)]
  place = np.empty(n_out, np.int64)
  for k in range(N_ALLOC):
    idx = np.where(alloc == k)[0]
    place[idx] = rs.permutation(row_len[k])[:idx.size]
  n_rows = N_ROWS if case.entry == 'rows' else 1
  rows = rs.permutation(n_rows + 2)[:n_rows].astype(np.int64)
  sel = rs.randint(0, n_rows, size=n_out).astype(np.int32)
  shift_el = rows[sel] * np.array(row_len)[alloc] if case.entry == 'rows' else 0
  el = place + shift_el  # element index inside its allocation
  stores = []  # the per-call src tables live until the sync
  fill_s = [start_sums(rs, row_len[k] * (n_rows + 2)) for k in range(N_ALLOC)]
  fill_c = [start_counts(rs, row_len[k] * (n_rows + 2)) for k in range(N_ALLOC)]
  start_s = np.array([fill_s[a][e] for a, e in zip(alloc, el)])
  start_c = np.array([fill_c[a][e] for a, e in zip(alloc, el)])
  steps = [vals[:, i] for i in range(n_time)]
  start_s = show_order(case, start_s, steps, mc.U_TIME)
  for a, e, v0 in zip(alloc, el, start_s):
    fill_s[a][e] = v0
  sum_b = [Buf(dev, x) for x in fill_s]
  cnt_b = [Buf(dev, x) for x in fill_c]
  base_s = np.array([b.ptr for b in sum_b], np.int64)
  base_c = np.array([b.ptr for b in cnt_b], np.int64)
  sa = Buf(dev, base_s[alloc] + 8 * place, sentinel=int(base_s[0]))
  ca = Buf(dev, base_c[alloc] + 8 * place, sentinel=int(base_c[0]))
  ab = Buf(dev, arena)
  sb = Buf(dev, src, sentinel=0)
  rb = Buf(dev, r32, sentinel=0)
  extra = []
  if case.entry == 'rows':
    extra = [Buf(dev, rows, sentinel=0), Buf(dev, sel, sentinel=0),
             Buf(dev, (8 * np.array(row_len, np.int64))[alloc], sentinel=0)]
    assert len(set(rows[sel].tolist())) == min(n_rows, n_out) or n_out < 8
  ws, wc = gr.running_sum(start_s, steps, case.skipna, start_c)
  for parts in splits(n_time):
    for b in sum_b + cnt_b:
      b.reset()
    for a, b in parts:
      sub = Buf(dev, np.ascontiguousarray(src[:, a:b]), sentinel=0)
      stores.append(sub)
      if case.entry == 'plain':
        rc = lib.wb2_gather_accumulate(ab.ptr, sub.ptr, rb.ptr, n_out, b - a,
                                       int(case.skipna), sa.ptr, ca.ptr,
                                       _stream(dev))
      else:
        rc = lib.wb2_gather_accumulate_rows(
            ab.ptr, sub.ptr, rb.ptr, n_out, b - a, int(case.skipna), sa.ptr,
            ca.ptr, extra[0].ptr, extra[1].ptr, extra[2].ptr, _stream(dev))
      assert rc == 0, lib.wb2_last_error()
    _sync()
    tag = f'{case.id} split {len(parts)}'
    for k in range(N_ALLOC):
      m = alloc == k
      gr.assert_bits(sum_b[k].host(), sum_b[k].expect(ws[m], el[m]),
                     f'{tag} sums {k}')
      gr.assert_bits(cnt_b[k].host(), cnt_b[k].expect(wc[m], el[m]),
                     f'{tag} counts {k}')
  for b in [sa, ca, ab, sb, rb] + extra:
    gr.assert_bits(b.host(), b.init, f'{case.id} input changed')


RUNNERS = {'maps': run_maps, 'acc': run_acc, 'addr': run_addr,
           'seeps': run_seeps, 'time': run_time, 'gather': run_gather}


@pytest.mark.parametrize('case', mc.CASES, ids=[c.id for c in mc.CASES])
def test_map_geometry(case, dev, lib):
  RUNNERS[case.kind](case, dev, lib)
