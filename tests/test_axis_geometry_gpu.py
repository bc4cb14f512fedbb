"""K7 (axis_reduce.hip) across run, slice, split and grid edges (-m gpu).

wb2_axis_moments, through engine.axis_moments with an explicit n_split, on a
[n_lead, n_red, n_tail] view: the contiguous kernel (n_tail == 1: a workgroup
per (lead, slice), its waves taking weight runs in turn, 16-byte or scalar
loads) and the strided one (n_tail > 1: a thread per tail element walking its
slice, 8 rows in flight), with slices of the reduced axis combined in order by
axis_combine_kernel.  Splits are counted in units: a weight run (w_repeat
elements) when weighted, else 4096 elements (contiguous) or one row (strided);
a slice is ceil(units / n_split) units, so n_split > units leaves empty
trailing splits.

The reference is math.fsum of w[r // w_repeat] * float64(x) (squares: x * x
in the input dtype, as take() computes them).  Sums must lie within 1e-12 *
fsum |w x| of it and counts must be exact.  x is bounded away from zero, so
every case can prove on the reference that dropping the last element of a
slice, or counting a split twice, breaks the tolerance.
"""
import dataclasses
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-12
CONTIG_UNIT = 4096   # elements per unweighted unit of the contiguous kernel
SPLITS = (1, 2, 5, 'auto', 'units', 'units+3')
ZGRID_LEAD = 32769   # past the grid's y dimension (32768): blockIdx.z > 0


@dataclasses.dataclass(frozen=True)
class Case:
  dtype: str
  n_lead: int
  n_red: int
  n_tail: int
  w_repeat: int      # 0: unweighted
  split: object      # a SPLITS entry
  skipna: bool
  want_sq: bool
  offset: int = 0    # elements past an aligned start

  @property
  def unit(self):
    if self.w_repeat:
      return self.w_repeat
    return 1 if self.n_tail > 1 else CONTIG_UNIT

  @property
  def units(self):
    return -(-self.n_red // self.unit)

  @property
  def id(self):
    w = f'w{self.w_repeat}' if self.w_repeat else 'unw'
    return (f'{self.dtype}-l{self.n_lead}-r{self.n_red}-t{self.n_tail}-{w}-'
            f'sp{self.split}-{"skipna" if self.skipna else "strict"}-'
            f'{"sq" if self.want_sq else "nosq"}-off{self.offset}')


def _cases():
  out = []
  i = 0
  dts = ('float32', 'float64')

  def add(dtype, n_lead, n_red, n_tail, w_repeat, offset=0):
    nonlocal i
    out.append(Case(dtype, n_lead, n_red, n_tail, w_repeat,
                    SPLITS[i % len(SPLITS)], bool(i // 2 % 2), i % 3 != 2,
                    offset))
    i += 1

  # contiguous kernel, unweighted: both sides of one and two 4096-element
  # units, 16-byte and scalar loads (odd lengths, a one-element offset)
  for n_red in (4095, 4096, 4097, 8193):
    for dtype in dts:
      for offset in (0, 1):
        add(dtype, 3, n_red, 1, 0, offset)
  # contiguous, weighted: odd runs on the scalar path, 1440 (16-byte), runs
  # fewer than the workgroup's 4 waves
  for w_repeat in (3, 1440, 1441):
    for runs in (7, 2):
      for dtype in dts:
        add(dtype, 2, w_repeat * runs, 1, w_repeat)
  add('float32', 2, 1440 * 3, 1, 1440, 1)
  # strided kernel: tails of one to four lanes' width and both sides of
  # 1024, reduced lengths on both sides of the 8-row unroll; weight runs
  weights = {1: 1, 7: 7, 8: 2, 9: 3, 65: 5, 200: 8}
  j = 0
  for n_tail in (2, 3, 4, 1023, 1024, 1025):
    for n_red in (1, 7, 8, 9, 65, 200):
      add(dts[j % 2], 2, n_red, n_tail, weights[n_red] if j % 3 else 0,
          1 if j % 5 == 4 else 0)
      j += 1
  # every split kind on both kernels in both dtypes, whatever the cycle gave
  for dtype in dts:
    for split in SPLITS:
      out.append(Case(dtype, 2, 4 * 1441, 1, 1441, split, True, True))
      out.append(Case(dtype, 2, 200, 1024, 8, split, True, True))
      out.append(Case(dtype, 3, 3 * CONTIG_UNIT + 5, 1, 0, split, False, True))
      out.append(Case(dtype, 2, 65, 3, 0, split, False, False))
  # leads past the grid's y dimension
  for dtype in dts:
    out.append(Case(dtype, ZGRID_LEAD, 3, 1, 0, 2, True, True))
    out.append(Case(dtype, ZGRID_LEAD, 2, 2, 0, 2, True, True))
  return out


CASES = _cases()


def n_split_of(case):
  if case.split == 'auto':
    from weatherbench2_amd import _lib
    return _lib.load().wb2_axis_moments_splits(
        case.n_lead, case.n_red, case.n_tail, case.w_repeat or 1)
  if case.split == 'units':
    return case.units
  if case.split == 'units+3':
    return case.units + 3
  return case.split


def slice_len(case, n_split):
  return -(-case.units // n_split) * case.unit


def test_the_sweep_reaches_its_edges():
  """(Also run with -m gpu: the split heuristic needs the library.)"""
  contig = [c for c in CASES if c.n_tail == 1]
  strided = [c for c in CASES if c.n_tail > 1]
  assert {4095, 4096, 4097, 8193} <= {c.n_red for c in contig
                                      if not c.w_repeat}
  assert {3, 1440, 1441} <= {c.w_repeat for c in contig}
  assert any(c.n_red == 2 * c.w_repeat for c in contig if c.w_repeat)
  vec = lambda c: (c.offset == 0 and c.n_red % (16 // _size(c)) == 0 and
                   c.unit % (16 // _size(c)) == 0)
  assert {vec(c) for c in contig} == {True, False}
  assert any(c.offset for c in contig) and any(c.offset for c in strided)
  assert {2, 3, 4, 1023, 1024, 1025} <= {c.n_tail for c in strided}
  assert {1, 7, 8, 9, 65, 200} <= {c.n_red for c in strided}
  assert any(c.w_repeat > 1 for c in strided)
  for group in (contig, strided):
    for dtype in ('float32', 'float64'):
      assert {c.split for c in group if c.dtype == dtype} >= set(SPLITS)
    assert {(c.skipna, c.want_sq) for c in group} == {
        (a, b) for a in (False, True) for b in (False, True)}
    assert any(c.n_lead == ZGRID_LEAD for c in group)


def _size(case):
  return 4 if case.dtype == 'float32' else 8


# ---- inputs and reference -----------------------------------------------------
def make_inputs(case, n_split, rs):
  """x [n_lead, n_red, n_tail] bounded away from zero, weights, and the NaN
  patterns: skipna puts NaN at the first and last element of a run (output
  1), over a whole slice (output 2) and over all of output n_out - 1 (count
  0); strict one NaN in output n_out - 1.  Output 0 stays finite."""
  shape = (case.n_lead, case.n_red, case.n_tail)
  sign = np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)
  x = (sign * rs.uniform(0.5, 1.5, shape)).astype(case.dtype)
  w = (rs.uniform(0.5, 1.5, case.n_red // case.w_repeat)
       if case.w_repeat else None)
  n_out = case.n_lead * case.n_tail
  flat = x.transpose(0, 2, 1).reshape(n_out, case.n_red)  # a copy
  if case.skipna:
    run = case.w_repeat or min(slice_len(case, n_split),
                               CONTIG_UNIT if case.n_tail == 1 else case.n_red)
    r0 = run if case.n_red >= 2 * run else 0
    if n_out >= 2:
      flat[1, r0] = flat[1, min(r0 + run, case.n_red) - 1] = np.nan
    if n_out >= 3:
      sl = slice_len(case, n_split)
      s0 = sl if sl < case.n_red else 0
      flat[2, s0:s0 + sl] = np.nan
    if n_out >= 4:
      flat[n_out - 1] = np.nan
  elif n_out >= 2:
    flat[n_out - 1, case.n_red // 2] = np.nan
  x = np.ascontiguousarray(
      flat.reshape(case.n_lead, case.n_tail, case.n_red).transpose(0, 2, 1))
  return x, w, flat


def reference(case, flat, w):
  """(sum, sum |w x|, sumsq, sum |w x^2|, count) per output, math.fsum."""
  wr = (np.repeat(w, case.w_repeat) if w is not None
        else np.ones(case.n_red))
  x64 = flat.astype(np.float64)
  sq64 = (flat * flat).astype(np.float64)   # squared in the input dtype
  ok = ~np.isnan(x64)
  if case.skipna:
    x64, sq64 = np.where(ok, x64, 0.0), np.where(ok, sq64, 0.0)
  def fs(a):
    return np.array([math.fsum(r) for r in a.tolist()])
  p, q = wr * x64, wr * sq64
  count = ok.sum(1).astype(np.float64) if case.skipna else np.full(
      len(flat), float(case.n_red))
  with np.errstate(invalid='ignore'):
    return fs(p), fs(np.abs(p)), fs(q), fs(np.abs(q)), count


def violations(got, want, mag):
  with np.errstate(invalid='ignore'):
    off = np.abs(got - want) > SUM_RTOL * mag
  return (np.isnan(got) != np.isnan(want)) | (off & ~np.isnan(want))


def prove_tolerance(case, flat, w, n_split, want, mag):
  """On output 0 (finite): the last element of slice 0 dropped, and slice 0
  counted twice, each move the sum outside the tolerance."""
  wr = np.repeat(w, case.w_repeat) if w is not None else np.ones(case.n_red)
  p = wr * flat[0].astype(np.float64)
  end = min(slice_len(case, n_split), case.n_red)
  dropped = want[0] - p[end - 1]
  twice = want[0] + math.fsum(p[:end].tolist())
  for what, mut in (('slice end dropped', dropped), ('split twice', twice)):
    assert abs(mut - want[0]) > SUM_RTOL * mag[0], (what, case.id)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_axis_geometry(case):
  import torch
  from weatherbench2_amd import engine
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  dev = torch.device('cuda')
  n_split = n_split_of(case)
  assert 1 <= n_split <= 65535
  rs = np.random.RandomState(sum(map(ord, case.id)) % 100003)
  x, w, flat = make_inputs(case, n_split, rs)
  buf = torch.empty(x.size + case.offset, dtype=getattr(torch, case.dtype),
                    device=dev)
  buf[case.offset:] = torch.as_tensor(x.ravel(), device=dev)
  xd = buf[case.offset:]
  assert (xd.data_ptr() % 16 == 0) == (case.offset == 0)
  wd = None if w is None else torch.as_tensor(w, device=dev)
  total, sq, count = engine.axis_moments(
      xd, case.n_lead, case.n_red, case.n_tail, wd, case.skipna, case.want_sq,
      case.w_repeat or 1, n_split=n_split)
  want, mag, want_sq, mag_sq, want_count = reference(case, flat, w)
  # outputs are [n_lead, n_tail] in memory, the reference [n_lead * n_tail]
  got = total.cpu().numpy()
  bad = violations(got, want, mag)
  assert not bad.any(), (case.id, 'sum', int(np.argmax(bad)),
                         got[bad][:3], want[bad][:3])
  if case.want_sq:
    got_sq = sq.cpu().numpy()
    bad = violations(got_sq, want_sq, mag_sq)
    assert not bad.any(), (case.id, 'sumsq', int(np.argmax(bad)))
  else:
    assert sq is None
  np.testing.assert_array_equal(count.cpu().numpy(), want_count)
  prove_tolerance(case, flat, w, n_split, want, mag)
