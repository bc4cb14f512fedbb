"""Shared cases of tests/test_quantile_score_cpu.py and
tests/test_quantile_score_gpu.py: seeded, all small.  The values are rounded
to one decimal, so a truth that equals a member -- a tie with a quantile that
falls on a member -- occurs by itself; the precipitation-like field has many
exact zeros in members and truth, so ties occur at interpolated quantiles
too."""
import numpy as np

from oracle.named import DS, NA
from tests import crps_decomposition_cases as base
from tests import events_cases

NAME = base.NAME
DTYPES = base.DTYPES
METHODS = ('linear', 'hazen', 'weibull')
GRIDS = ((2, 7), (5, 30), (9, 68), (19, 72))
TERM, LEVEL, INTERVAL = 'term', 'level', 'interval'
TERMS = ('pinball', 'forecast_quantile', 'below', 'tie')
LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
QDIM = 'quantile'

grid = base.grid
datasets = base.datasets
oracle_regions = base.oracle_regions
product_regions = base.product_regions
assert_same_dataset = events_cases.assert_same_dataset
rotated = events_cases.classes   # class = column mod n_class, rotated
runs = base.classes              # classes in runs, the first one wrapping


def arrays(n_member, n_outer, n_row, n_col, dtype, nan='none', seed=0,
           kind='normal'):
  """(ens [M, O, R, C], truth [O, R, C]) of `dtype`, one decimal: `kind`
  'normal', or 'precip' (a skewed field, about half of it exact zeros).
  `nan`: 'none', 'truth', 'member' (one member of a point) or 'both', about
  8 % of the points each."""
  rs = np.random.RandomState(seed + 17 * n_member + n_row)
  shape = (n_outer, n_row, n_col)
  if kind == 'precip':
    field = lambda size: np.round(np.maximum(
        rs.gamma(0.6, 3.0, size=size) - 1.0, 0.0), 1)
  else:
    field = lambda size: np.round(rs.normal(size=size) * 2.0, 1)
  ens = field((n_member,) + shape).astype(dtype)
  truth = field(shape).astype(dtype)
  if nan in ('truth', 'both'):
    truth[rs.rand(*shape) < 0.08] = np.nan
  if nan in ('member', 'both'):
    hit = rs.rand(*shape) < 0.08
    member = rs.randint(n_member, size=shape)
    for idx in zip(*np.nonzero(hit)):
      ens[(member[idx],) + idx] = np.nan
  return ens, truth


def blank_class(truth, col_class, c):
  """`truth` with NaN in every column of class `c`: a whole class invalid."""
  out = truth.copy()
  out[..., np.asarray(col_class) == c] = np.nan
  return out


def quantile_datasets(quantiles, truth, levels):
  """Oracle (forecast, truth) of quantile forecasts [L, T, lat, lon] along the
  dim `QDIM` with the coordinate `levels`."""
  n_level, n_time, n_lat, n_lon = quantiles.shape
  lat, lon = grid(n_lat, n_lon)
  coords = {'latitude': lat, 'longitude': lon, 'time': np.arange(n_time),
            QDIM: np.asarray(levels, dtype=np.float64)}
  dims = (QDIM,) + base.DIMS[1:]
  forecast = DS({NAME: NA(quantiles, dims)}, coords)
  coords = {k: v for k, v in coords.items() if k != QDIM}
  return forecast, DS({NAME: NA(truth, dims[1:])}, coords)
