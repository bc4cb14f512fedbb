"""The class-sums layer on the device (-m gpu): K20 (csrc/crps_bins.hip), K21
(csrc/twcrps.hip) and K24 (csrc/conditional_sums.hip) request the points of a
tile in the same way (csrc/class_sums.hpp's class_tile(), of which K20 keeps a
copy), so on the same operands their valid counts per (outer index, row, column
class) are the same integers, and those of a count taken in NumPy from the
inputs.  Every table handed to a kernel here is valid."""
import numpy as np
import pytest
import torch

from weatherbench2_amd import engine

pytestmark = pytest.mark.gpu

_ID = lambda v: getattr(v, '__name__', None) or str(v)
DTYPES = (np.float32, np.float64)
# below, at and above one wave = the column tile: one, two and three tiles of
# a row, with and without a partial last one
COLS = (1, 63, 64, 65, 129)
# the padded register counts 2, 4, 32 and 64
MEMBERS = (1, 3, 17, 50)
N_OUTER, N_ROW, N_CLASS = 2, 2, 3
EDGES = (-0.5, 0.5)  # three bins of the truth


def _classes(n_col):
  """Class 0, a border to class 1 inside the first tile, class 0 again (left
  and met again), class 2 from column 70 on: no column of a row of up to 70
  columns has it."""
  j = np.arange(n_col)
  return np.where(j < 5, 0, np.where(j < 40, 1, np.where(j < 70, 0, 2))
                  ).astype(np.int32)


def _inputs(n_member, n_col, dtype, seed):
  rs = np.random.RandomState(seed)
  ens = rs.standard_normal((n_member, N_OUTER, N_ROW, n_col)).astype(dtype)
  truth = rs.standard_normal((N_OUTER, N_ROW, n_col)).astype(dtype)
  truth[0, 0, 0] = np.nan                          # in the truth
  ens[n_member // 2, 1, 1, min(2, n_col - 1)] = np.nan  # in one member
  ens[0, 1, 0, n_col - 1] = np.nan                 # in a last-tile column
  return ens, truth


def _counts(ens, stride, n_member, truth, n_col, cls):
  """The valid counts [outer, row, class] of K20, of K21 under a NaN-free
  threshold and of K24 summed over its bins."""
  front = (ens, stride, n_member, None, truth, None)
  back = (N_OUTER, N_ROW, n_col, cls, N_CLASS)
  thr = torch.zeros((N_OUTER, N_ROW, n_col), dtype=truth.dtype, device='cuda')
  k20 = engine.crps_bin_sums(*front, *back)[1][..., 2]
  k21 = engine.twcrps_sums(*front, [thr], None, *back)[1][0, ..., 0]
  k24 = engine.conditional_sums(*front, *back, 'truth', EDGES)[1].sum(dim=-1)
  return tuple(x.cpu().numpy().astype(np.int64) for x in (k20, k21, k24))


def _want(ens, truth, cls):
  valid = ~(np.isnan(truth) | np.isnan(ens).any(axis=0))
  return np.stack([valid[..., cls == c].sum(axis=-1) for c in range(N_CLASS)],
                  axis=-1).astype(np.int64)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID)
@pytest.mark.parametrize('n_member', MEMBERS)
def test_the_three_kernels_count_the_same_valid_points(n_member, dtype):
  for n_col in COLS:
    cls = _classes(n_col)
    ens, truth = _inputs(n_member, n_col, dtype, 100 * n_member + n_col)
    want = _want(ens, truth, cls)
    assert want.sum() == N_OUTER * N_ROW * n_col - 3  # (the three NaN points)
    got = _counts(torch.from_numpy(ens).cuda(), N_OUTER * N_ROW * n_col,
                  n_member, torch.from_numpy(truth).cuda(), n_col, cls)
    for name, have in zip(('K20', 'K21', 'K24'), got):
      np.testing.assert_array_equal(have, want, err_msg=f'{name} {n_col}')


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID)
def test_members_off_their_storage_start_with_an_odd_stride(dtype):
  """The members start one element into their storage, member m
  `member_stride` = one member + 3 elements further: no multiple of 4."""
  n_member, n_col = 3, 65
  cls = _classes(n_col)
  ens, truth = _inputs(n_member, n_col, dtype, 7)
  one = N_OUTER * N_ROW * n_col
  stride = one + 3
  assert stride % 4
  store = np.full(1 + n_member * stride, np.nan, dtype=dtype)
  for m in range(n_member):
    store[1 + m * stride:1 + m * stride + one] = ens[m].reshape(-1)
  view = torch.from_numpy(store).cuda()[1:]
  got = _counts(view, stride, n_member, torch.from_numpy(truth).cuda(), n_col,
                cls)
  for name, have in zip(('K20', 'K21', 'K24'), got):
    np.testing.assert_array_equal(have, _want(ens, truth, cls), err_msg=name)
