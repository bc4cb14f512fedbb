"""Shared cases of tests/test_variogram_cpu.py and tests/test_variogram_gpu.py:
seeded, all small, built on the generators of
tests/crps_decomposition_cases.py (values on a 0.25 grid, so equal neighbours
-- a zero increment -- occur by themselves)."""
import itertools

import numpy as np

from tests import crps_decomposition_cases as base
from tests import events_cases

NAME = base.NAME
DTYPES = base.DTYPES
ORDERS = (0.5, 1, 2)
GRIDS = ((2, 7), (5, 30), (9, 68), (19, 72))
TERM, LAG = 'term', 'lag'
TERMS = ('truth_variogram', 'forecast_variogram', 'score')
# column neighbours both ways, a row neighbour, both offsets at once; on two
# rows (2, 5) is a lag that no row reaches; |b| < 7
LAGS = ((0, 1), (0, -1), (1, 0), (1, -3), (2, 5))

grid = base.grid
arrays = base.arrays
datasets = base.datasets
oracle_regions = base.oracle_regions
product_regions = base.product_regions
assert_same_dataset = events_cases.assert_same_dataset
rotated = events_cases.classes   # class = column mod n_class, rotated


def planted(n_member, n_outer, n_row, n_col, dtype, nan=True, seed=0):
  """(ens [M, O, R, C], truth [O, R, C]) of `dtype`: `arrays` without NaN and,
  with `nan`, one NaN in three rows of four, cycling over rows and outer
  indices: in the truth at column 1 (an anchor, and the partner of its
  neighbours), in member 0 at the middle column (a partner), in the LAST member
  at the last column and in the truth at column 0 (the two seam columns)."""
  ens, truth = arrays(n_member, n_outer, n_row, n_col, dtype, seed=seed)
  if not nan:
    return ens, truth
  nan_ = dtype(np.nan)
  for o, r in itertools.product(range(n_outer), range(n_row)):
    kind = (o + r) % 4
    if kind == 0:
      truth[o, r, min(1, n_col - 1)] = nan_
    elif kind == 1:
      ens[0, o, r, n_col // 2] = nan_
    elif kind == 2:
      ens[n_member - 1, o, r, n_col - 1] = nan_
    elif (o + r) % 8 == 3:
      truth[o, r, 0] = nan_
  return ens, truth
