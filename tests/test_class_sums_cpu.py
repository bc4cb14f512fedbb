"""The class-sums layer without a device: what csrc/class_sums.hpp checks for
K20, K21 and K24 alike before anything is enqueued, and the host fold of
weatherbench2_amd/class_tables.py against the three modules' callers."""
import ctypes

import numpy as np
import pytest

from weatherbench2_amd import class_tables


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_every_sums_entry_point_refuses_a_row_too_long_for_its_lanes(lib):
  """A lane's byte offset into its row is an int: n_col * 8 must stay below
  2^31.  The pointers are dummies; nothing is read before the check."""
  h = lib.load()
  buf = np.zeros(64, dtype=np.int64)
  b = buf.ctypes.data
  thr = (ctypes.c_void_p * 1)(b)
  long_row = 1 << 28

  def crps(n_col):
    return h.wb2_crps_bin_sums(lib.WB2_F32, b, None, b, None, 5, 8, 2, 2,
                               n_col, b, 2, b, b, None)

  def twcrps(n_col):
    return h.wb2_twcrps_sums(lib.WB2_F32, b, None, b, None, thr, None, 1, 5, 8,
                             2, 2, n_col, b, 2, 0, b, b, None)

  def conditional(n_col):
    return h.wb2_conditional_sums(lib.WB2_F32, b, None, b, None, 5, 8, 2, 2,
                                  n_col, b, 2, 0, b, 3, b, b, None)
  for sums in (crps, twcrps, conditional):
    assert sums(long_row) < 0, sums.__name__
    assert b'the row is too long' in h.wb2_last_error(), sums.__name__
    # (the other checks still come first, and an empty call is still a no-op)
    assert sums(-1) < 0 and b'negative' in h.wb2_last_error()
    assert sums(0) == 0


def test_host_fold_is_the_ordered_fold_over_any_trailing_axes():
  rs = np.random.RandomState(0)
  n_row, n_class, n_region = 5, 3, 4
  wrow = rs.standard_normal((n_region, n_row))
  mult = rs.randint(0, 3, (n_region, n_class)).astype(np.int32)
  for lead, trail in (((2,), (2, 6)), ((3, 2), (2,)), ((2,), ())):
    sums = rs.standard_normal(lead + (n_row, n_class) + trail)
    got = class_tables.host_fold(sums, wrow, mult, n_lead=len(lead))
    assert got.shape == lead + (n_region,) + trail
    for cell in np.ndindex(*lead):
      for r in range(n_region):
        acc = np.zeros(trail)
        for i in range(n_row):
          s = np.zeros(trail)
          for c in range(n_class):
            s = s + float(mult[r, c]) * sums[cell + (i, c)]
          acc = acc + wrow[r, i] * s
        np.testing.assert_array_equal(
            np.asarray(got[cell + (r,)]).view(np.uint64),
            np.asarray(acc).view(np.uint64))
