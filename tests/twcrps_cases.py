"""Shared cases of tests/test_twcrps_cpu.py and tests/test_twcrps_gpu.py:
seeded, all small, built on the generators of
tests/crps_decomposition_cases.py (values on a 0.25 grid, so ties and exact
threshold hits occur by themselves; `classes()` with the wrapping first
class)."""
import numpy as np

from oracle.named import DS, NA
from tests import crps_decomposition_cases as base
from tests.events_cases import FieldThreshold

NAME = base.NAME
GRIDS = base.GRIDS
MEMBERS = base.MEMBERS  # 1, 2, 3, 7, 33, 50, 64
DTYPES = base.DTYPES
NANS = base.NANS + ('threshold',)  # none, truth, member, both, threshold
TAILS = ('upper', 'lower')
N_THRESHOLDS = (1, 4, 5)  # below, at and beyond one launch's group
DIMS = base.DIMS

grid = base.grid
datasets = base.datasets
classes = base.classes
oracle_regions = base.oracle_regions
product_regions = base.product_regions
assert_same_dataset = base.assert_same_dataset


def arrays(n_member, n_time, n_lat, n_lon, dtype, nan='none', seed=0):
  """`base.arrays`; the pattern 'threshold' has NaNs in the truth and in a
  member as 'both' does (and `threshold_fields` then adds its own)."""
  return base.arrays(n_member, n_time, n_lat, n_lon, dtype,
                     'both' if nan == 'threshold' else nan, seed)


def threshold_fields(n_threshold, n_time, n_lat, n_lon, dtype, nan='none',
                     seed=0, lead=True):
  """`n_threshold` threshold fields [time, lat, lon] (or [lat, lon] with
  lead=False) of `dtype` on the 0.25 grid of the values, spread from the lower
  to the upper tail of the members; the pattern 'threshold' plants NaNs in
  threshold 0 ONLY (in the last one too where there are several launches), so
  that validity differs between the thresholds of one launch."""
  rs = np.random.RandomState(seed + 101 * n_threshold + n_lon)
  shape = (n_time, n_lat, n_lon) if lead else (n_lat, n_lon)
  centres = np.linspace(-1.0, 1.5, n_threshold) if n_threshold > 1 else [0.5]
  fields = []
  for k, centre in enumerate(centres):
    f = (np.round((centre + 0.4 * rs.normal(size=shape)) * 4) / 4
         ).astype(dtype)
    if nan == 'threshold' and k in (0, 4):
      f[rs.rand(*shape) < 0.1] = np.nan
      f.reshape(-1)[k] = np.nan  # (at least one)
    fields.append(f)
  return fields


def thresholds(fields, oracle_truth, product, lead=True):
  """`FieldThreshold`s of such fields for the product (`product` converts an
  oracle Dataset); quantile labels 0.1, 0.2, ..."""
  dims = DIMS[1:] if lead else DIMS[2:]
  coords = {k: v for k, v in oracle_truth.coords.items() if k in dims}
  return [FieldThreshold(product(DS({NAME: NA(f, dims)}, coords)),
                         0.1 * (k + 1)) for k, f in enumerate(fields)]


def planted(dtype):
  """(ens [3, 1, 2, 6], truth [1, 2, 6], threshold value 1.0) with exact cases
  planted by hand, the same in both rows.  Column by column, tail 'upper', t =
  1.0:
    0  members and truth below t:            A = 0,         B = 0
    1  members below, truth 2.5 above:       A = 3 * 1.5,   B = 0
    2  truth exactly on t, members 0, 1, 3:  A = 2,         B = 2 * 2 = 4
    3  a member exactly on t (1, 2, 4), truth 0.5 -> v = 1:
                                             A = 0 + 1 + 3, B = 2*1 + 2*2 = 6
    4  all members equal 2.0, truth 3.0:     A = 3,         B = 0
    5  members -1, 0.5, 2 straddle, truth 0: A = 0 + 0 + 1, B = 2 * 1 = 2
  (B: k (M - k) = 2, 2 for M = 3 over the clamped gaps.)"""
  cols = [((-1.0, 0.0, 0.5), 0.25), ((0.0, -2.0, 0.75), 2.5),
          ((3.0, 0.0, 1.0), 1.0), ((4.0, 1.0, 2.0), 0.5),
          ((2.0, 2.0, 2.0), 3.0), ((2.0, -1.0, 0.5), 0.0)]
  ens = np.empty((3, 1, 2, 6), dtype=dtype)
  truth = np.empty((1, 2, 6), dtype=dtype)
  for j, (members, y) in enumerate(cols):
    ens[:, 0, :, j] = np.array(members, dtype=dtype)[:, None]
    truth[0, :, j] = y
  a = np.array([0.0, 4.5, 2.0, 4.0, 3.0, 1.0])
  b = np.array([0.0, 0.0, 4.0, 6.0, 0.0, 2.0])
  return ens, truth, 1.0, a, b
