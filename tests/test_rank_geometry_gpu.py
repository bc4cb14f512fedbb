"""The rank histogram across member, bin, wave, grid and stream edges (-m gpu).

rank_histogram_kernel (one-hot and atomic counts) and
rank_histogram_mean_kernel (means and sums) over the sweep of
tests/rank_geometry_cases.py (its reach is asserted on the CPU by
test_rank_geometry_cpu.py), against the plain NumPy references of
tests/rank_np.py.  Every output is 0/1, an integer count or a count divided by
n_time, so every comparison is exact:

  * no ties, ties broken for the truth (break_ties = 0), a NaN truth: the
    one-hot of the counted rank;
  * hash ties: exact where no member equals the truth, inside [lo, lo + eq]
    where some do, the same bytes from a second run and from permuted tables;
  * seeded ties: the reference's own rank (NumPy's PCG64 stream, the
    perturbation sized in the data dtype) on every sample whose order the
    reference does not leave open, inside its bounds on the others;
  * counts, means and sums: float64 sums of the reference's one-hots (a true
    division for the mean), never another kernel form.

Outputs are poisoned before a kernel fills them, rows of the counts that no
acc_row names must stay zero, and the inputs are compared by bytes afterwards.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import rank_geometry_cases as rc
from tests import rank_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  return torch.device('cuda', 0)


def _pcg(seed):
  state = np.random.PCG64(seed).state['state']
  return int(state['state']), int(state['inc'])


def _sums_through_the_c_abi(case, dev, t, numpy_stream):
  """wb2_rank_histogram_mean with mean = 0 (the sums), which
  engine.rank_histogram never asks for: the same call, made here."""
  import torch
  from weatherbench2_amd import _lib
  from weatherbench2_amd import engine
  lib = _lib.load()
  n_lead, n_time, n_tail = case.shape
  out = torch.full((n_lead * n_tail, case.n_point, case.n_bins), float('nan'),
                   dtype=torch.float64, device=dev)
  pcg = st = ref_off = None
  n_col = 1
  if numpy_stream is not None:
    state, inc, ref_off, strides, n_col = numpy_stream
    mask = (1 << 64) - 1
    pcg = (ctypes.c_uint64 * 4)(state >> 64, state & mask, inc >> 64,
                                inc & mask)
    st = (ctypes.c_int64 * 3)(*[int(v) for v in strides])
  _lib.check(lib.wb2_rank_histogram_mean(
      _lib.WB2_F32 if case.dtype == 'float32' else _lib.WB2_F64,
      _lib.ptr(t['ens']), _lib.ptr(t['ens_slab']), _lib.ptr(t['truth']),
      _lib.ptr(t['truth_slab']), case.n_member, t['member_stride'], n_lead,
      n_time, n_tail, case.n_point, int(n_col), case.n_bins,
      int(case.ties != 'first'), case.seed, pcg, _lib.ptr(ref_off), st, 0,
      _lib.ptr(out), engine.current_stream_ptr(dev)),
             'wb2_rank_histogram_mean')
  return out


def run(case, dev, expect, bufs=None):
  """One case through the library: the result as a NumPy array."""
  import torch
  from weatherbench2_amd import engine
  bufs = rc.make_buffers(case, expect.data) if bufs is None else bufs
  up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
  host = {'ens': bufs.ens, 'truth': bufs.truth, 'ens_slab': bufs.ens_slab,
          'truth_slab': bufs.truth_slab}
  t = {k: up(v) for k, v in host.items()}
  t['member_stride'] = bufs.member_stride
  numpy_stream = None
  if case.ties == 'numpy':
    s = expect.stream
    host['ref_off'] = s.off
    t['ref_off'] = up(s.off)
    numpy_stream = _pcg(case.seed) + (t['ref_off'], s.strides, s.n_col)
  rows = None
  if case.form == 'counts':
    host['rows'] = rc.acc_rows(case)
    rows = t['rows'] = up(host['rows'])
  shape = (case.n_acc, case.n_point, case.n_bins)
  if case.form == 'sum':
    out = _sums_through_the_c_abi(case, dev, t, numpy_stream)
  else:
    # what the allocator hands out next holds NaNs, not an earlier result
    poison = torch.full(shape, float('nan'), dtype=torch.float64, device=dev)
    del poison
    out = engine.rank_histogram(
        t['ens'], bufs.member_stride, case.n_member, t['ens_slab'], t['truth'],
        t['truth_slab'], case.n_outer, case.n_point, case.n_bins,
        case.ties != 'first', case.seed, rows, case.n_acc if rows is not None
        else 0, numpy_stream=numpy_stream,
        mean_over=case.shape if case.form == 'mean' else None)
  torch.cuda.synchronize()
  assert tuple(out.shape) == shape and out.dtype == torch.float64
  got = out.cpu().numpy()
  for name, before in host.items():
    if before is not None:
      assert t[name].cpu().numpy().tobytes() == before.tobytes(), (
          case.id, name, 'input changed')
  return got


def rank_bounds(case, e):
  """The ranks the references allow per sample, lo <= rank <= hi: equal
  wherever the result is determined."""
  if case.ties in ('none', 'first'):
    return e.first, e.first
  if case.ties == 'hash':
    return e.first, e.first + e.eq
  lo = np.where(e.open, e.less, e.rank)
  hi = np.where(e.open, e.less + e.equal, e.rank)
  nan_truth = np.isnan(e.data.truth)
  return np.where(nan_truth, e.nn, lo), np.where(nan_truth, e.nn, hi)


def check(case, got, e):
  m, nb = case.n_member, case.n_bins
  lo, hi = rank_bounds(case, e)
  if case.ties == 'none':
    assert (e.eq == 0).all()
  sure = lo == hi
  want = rank_np.one_hot(rank_np.bin_of(lo, m, nb), nb)
  if case.form == 'onehot':
    np.testing.assert_array_equal(got[sure], want[sure], err_msg=case.id)
    # the others: a one-hot all the same, its bin inside the bounds
    rest = got[~sure]
    assert ((rest == 0) | (rest == 1)).all() and (rest.sum(-1) == 1).all(), (
        case.id)
    at = rest.argmax(-1)
    assert (rank_np.bin_of(lo[~sure], m, nb) <= at).all() and (
        at <= rank_np.bin_of(hi[~sure], m, nb)).all(), case.id
    if case.ties == 'hash' and case.recipe != 'plain':
      assert (~sure).any(), case.id
    return
  assert sure.all(), case.id
  if case.form == 'counts':
    total = np.zeros((case.n_acc, case.n_point, nb))
    np.add.at(total, rc.acc_rows(case), want)
    assert not total[-1].any() and total[:-1].any()
  else:
    n_lead, n_time, n_tail = case.shape
    by_axis = want.reshape(n_lead, n_time, n_tail, case.n_point, nb)
    total = (rank_np.mean_over(by_axis, 1) if case.form == 'mean'
             else rank_np.sum_over(by_axis, 1))
    total = total.reshape(n_lead * n_tail, case.n_point, nb)
  np.testing.assert_array_equal(got, total, err_msg=case.id)


def _parts():
  """One test per part of the sweep: a group's cases of one dtype; the mean
  kernel's by the shape of its outer index."""
  parts = {}
  for c in rc.CASES:
    if c.group == 'uniform':
      continue
    key = (c.group, 'x'.join(map(str, c.shape)) if c.group == 'mean'
           else c.dtype)
    parts.setdefault(key, []).append(c)
  return parts


_PARTS = _parts()


@pytest.mark.parametrize('part', list(_PARTS), ids=lambda k: f'{k[0]}-{k[1]}')
def test_sweep(part, dev):
  for case in _PARTS[part]:
    e = rc.expected(case)
    check(case, run(case, dev, e), e)


def test_hash_draw_is_reproducible_and_ignores_the_tables(dev):
  """One seed, one (o, pt): the same bytes from a second run, and from tables
  that keep the slabs somewhere else."""
  cases = [c for c in rc.CASES if c.group == 'slabs' and c.ties == 'hash']
  assert len(cases) == 4
  for dtype in rc.DTYPES:
    plain, = [c for c in cases if c.dtype == dtype and c.slab == 'identity']
    moved, = [c for c in cases if c.dtype == dtype and c.slab == 'permuted']
    e = rc.expected(plain)
    first = run(plain, dev, e)
    check(plain, first, e)
    assert run(plain, dev, e).tobytes() == first.tobytes()
    assert run(moved, dev, rc.expected(moved)).tobytes() == first.tobytes()
    # and the draw does depend on the seed
    other = run(dataclasses.replace(plain, seed=plain.seed + 1), dev, e)
    assert other.tobytes() != first.tobytes()


@pytest.mark.parametrize('case', [c for c in rc.CASES if c.group == 'uniform'],
                         ids=lambda c: c.id)
def test_hash_draw_reaches_every_rank(case, dev):
  e = rc.expected(case)
  got = run(case, dev, e)
  check(case, got, e)
  assert case.n_sample >= 20000 and case.n_bins == case.n_member + 1 <= 6
  assert (got.reshape(-1, case.n_bins).sum(0) > 0).all()


def test_mean_kernel_refuses_257_bins(dev):
  from weatherbench2_amd import _lib
  case = rc.Case('limit', 'mean', 'first', 'float32', 2 * (rc.MAX_BINS + 1) - 1,
                 rc.MAX_BINS + 1, shape=(1, 2, 1), n_point=3,
                 recipe='quantised')
  e = rc.expected(case)
  with pytest.raises(_lib.Wb2HipError, match=f'more than {rc.MAX_BINS} bins'):
    run(case, dev, e)


@pytest.mark.parametrize('dtype', rc.DTYPES)
def test_counts_beyond_the_mean_kernels_bins(dtype, dev):
  case = rc.Case('limit', 'counts', 'first', dtype, 2 * rc.MAX_BINS - 1,
                 2 * rc.MAX_BINS, n_outer=4, n_point=65, recipe='quantised')
  e = rc.expected(case)
  check(case, run(case, dev, e), e)


def test_metric_falls_back_to_counts_beyond_256_bins(dev):
  """RankHistogram(num_bins=512).compute on 2 x 3 points: the atomic counts,
  divided by n_time, equal the mean of the reference's one-hots."""
  from oracle.named import DS, NA
  from tests import helpers
  from weatherbench2_amd import metrics as gm
  rs = np.random.RandomState(6)
  n_t, n_m, nb = 3, 2 * rc.MAX_BINS - 1, 2 * rc.MAX_BINS
  f = (np.round(rs.standard_normal((n_t, 2, 3, n_m)) * 40) / 4).astype(
      np.float32)
  t = (np.round(rs.standard_normal((n_t, 2, 3)) * 40) / 4).astype(np.float32)
  f[1, 0, 1, 5] = np.nan
  t[2, 1, 2] = np.nan
  coords = {'time': np.arange(n_t), 'realization': np.arange(n_m),
            'latitude': np.array([-30.0, 30.0]),
            'longitude': np.array([0.0, 120.0, 240.0])}
  forecast = DS({'z': NA(f, ('time', 'latitude', 'longitude', 'realization'))},
                coords)
  truth = DS({'z': NA(t, ('time', 'latitude', 'longitude'))},
             {k: v for k, v in coords.items() if k != 'realization'})
  g = helpers.to_gpu_dataset
  got = gm.RankHistogram(num_bins=nb, break_ties_randomly=False).compute(
      g(forecast), g(truth))['z']
  assert got.dims == ('latitude', 'longitude', 'bins')
  rank = rank_np.first_rank(f, t)
  assert (rank_np.counts(f, t)[1] > 0).mean() > 0.2
  want = rank_np.mean_over(rank_np.one_hot(rank_np.bin_of(rank, n_m, nb), nb),
                           0)
  values = got.data
  values = (values.cpu().numpy() if hasattr(values, 'cpu')
            else np.asarray(values))
  np.testing.assert_array_equal(values, want)
