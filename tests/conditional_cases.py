"""Shared cases of tests/test_conditional_cpu.py and
tests/test_conditional_gpu.py: seeded, all small, built on the generators of
tests/crps_decomposition_cases.py (values on a 0.25 grid, so a truth or an
ensemble mean on a bin edge occurs by itself; `classes()` with the wrapping
first class)."""
import numpy as np

from tests import crps_decomposition_cases as base

NAME = base.NAME
GRIDS = base.GRIDS          # (5, 8), (19, 72)
MEMBERS = (1, 2, 3, 7, 33, 50, 64)
DTYPES = base.DTYPES
NANS = base.NANS            # none, truth, member, both
BYS = ('spread', 'forecast', 'truth')
BINS = (1, 2, 5, 17, 64)    # no edge, one, a few, many, every lane a bin
DIMS = base.DIMS

grid = base.grid
arrays = base.arrays
datasets = base.datasets
classes = base.classes
oracle_regions = base.oracle_regions
product_regions = base.product_regions
assert_same_dataset = base.assert_same_dataset


def edges(by, n_bin):
  """`n_bin - 1` edges as the metric takes them.  'forecast' and 'truth': on
  the 0.25 grid of the values, centred on 0 (a truth on an edge occurs by
  itself; with 63 edges most bins are empty).  'spread': standard deviations
  0.25, 0.5, ... (an ensemble of the 0.25 grid has its spread about 1)."""
  n_edge = n_bin - 1
  if by == 'spread':
    return tuple(0.25 * (1 + k) for k in range(n_edge))
  return tuple(0.25 * (k - n_edge // 2) for k in range(n_edge))


def kernel_edges(by, n_bin):
  """The same edges as the kernel and `host_sums` take them (squared for
  'spread')."""
  e = np.array(edges(by, n_bin), dtype=np.float64)
  return e * e if by == 'spread' else e


def interleaved(n_col, period=(0, 1, 0, 2, 2, 1, 0)):
  """A hand-made class table without runs: the classes 0, 1, 2 interleaved
  with a period of 7, so that every class recurs within a tile and across
  every tile border (64 is no multiple of 7)."""
  return np.array([period[j % len(period)] for j in range(n_col)], np.int32)


RELIABLE_EDGES = (0.03, 0.6, 30.0)  # standard deviations


def reliable(n_point=20000, n_member=10, seed=3):
  """(ens [M, 1, 1, n], truth [1, 1, n]) float64 of a RELIABLE ensemble: the
  truth is drawn like a member, N(c, sigma^2) per point with the point's own
  centre c.  The per-point sigma spans a decade in TWO BANDS, log-uniform in
  [0.3, 0.35] and in [2.6, 3.0], and RELIABLE_EDGES puts each band into a bin
  of its own (the outer two bins stay empty).  The bands are the point: the
  bins are cut by the SAMPLE spread, and within a continuum of sigma a bin
  selects the points whose sample variance happens to lie in it, so that E[
  sigma^2 | bin] differs from E[s2 | bin] by a factor of order (M - 1) / (M -
  3) even for a perfectly reliable ensemble.  With the bands next to no point
  changes its bin by sampling: s < 0.6 under sigma >= 2.6 needs chi2_9 < 0.48
  (probability 2e-5: such a point would bring a large error into the low bin),
  s > 0.6 under sigma <= 0.35 needs chi2_9 > 26 (2e-3: such points bring next
  to nothing into the high bin).  So per bin E[se] = (1 + 1 / M) E[sigma^2]
  and E[s2] = E[sigma^2]: the debiased ratio estimates 1."""
  rs = np.random.RandomState(seed)
  low = rs.rand(n_point) < 0.5
  sigma = np.where(low, 0.3 * (0.35 / 0.3) ** rs.rand(n_point),
                   2.6 * (3.0 / 2.6) ** rs.rand(n_point))
  centre = rs.normal(size=n_point)
  ens = centre + sigma * rs.normal(size=(n_member, n_point))
  truth = centre + sigma * rs.normal(size=n_point)
  return (ens.reshape(n_member, 1, 1, n_point),
          truth.reshape(1, 1, n_point))
