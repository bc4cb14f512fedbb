"""Shared cases of tests/test_joint_cpu.py and tests/test_joint_gpu.py: seeded,
all small, built on the generators of tests/crps_decomposition_cases.py (values
on a 0.25 grid, so a truth or a member on an edge occurs by itself)."""
import itertools

import numpy as np

from tests import crps_decomposition_cases as base
from tests import events_cases

NAME = base.NAME
DTYPES = base.DTYPES
NANS = base.NANS            # none, truth, member, both
SIDES = ('right', 'left')
EDGES = (0, 1, 8, 31)       # no edge, one, a few, every edge the kernel takes
TRUTH_BIN, FORECAST_BIN = 'truth_bin', 'forecast_bin'

grid = base.grid
arrays = base.arrays
datasets = base.datasets
oracle_regions = base.oracle_regions
product_regions = base.product_regions
assert_same_dataset = events_cases.assert_same_dataset
rotated = events_cases.classes   # class = column mod n_class, rotated


def edges(n_edge):
  """`n_edge` edges on the 0.25 grid of the values, centred on 0 (31 of them
  span -3.75 .. 3.75: the outer categories are thinly filled)."""
  return tuple(0.25 * (k - n_edge // 2) for k in range(n_edge))


def planted(n_member, n_outer, n_row, n_col, dtype, given, nan=True, seed=0):
  """(ens [M, O, R, C], truth [O, R, C]) of `dtype`: `arrays` with, at columns
  0..5 and the last four of every row (around the 16-byte lane borders),
  cycling over rows and outer indices: NaN in the truth, NaN in one member
  (both only with `nan`), a member and the truth exactly on an edge, +-inf in
  a member and in the truth."""
  ens, truth = arrays(n_member, n_outer, n_row, n_col, dtype, seed=seed)
  cols = sorted({c for c in list(range(6)) + list(range(n_col - 4, n_col))
                 if 0 <= c < n_col})
  inf, nan_ = dtype(np.inf), dtype(np.nan)
  given = [dtype(e) for e in given] or [dtype(0.0)]
  for n, (o, r, c) in enumerate(itertools.product(
      range(n_outer), range(n_row), cols)):
    kind, m, e = n % 8, n % n_member, given[n % len(given)]
    if kind == 0 and nan:
      truth[o, r, c] = nan_
    elif kind == 1 and nan:
      ens[m, o, r, c] = nan_
    elif kind == 2:
      ens[m, o, r, c] = e
    elif kind == 3:
      truth[o, r, c] = e
    elif kind == 4:
      ens[m, o, r, c] = inf
    elif kind == 5:
      truth[o, r, c] = -inf
    elif kind == 6:
      ens[m, o, r, c] = -inf
    elif kind == 7:
      truth[o, r, c] = inf
  return ens, truth
