"""CRPS decomposition: per-rank-bin tables, reliability and potential CRPS.

`CRPS`, `CRPSSkill` and `CRPSSpread` give one number per (variable, lead,
region); it does not say whether a poor ensemble is miscalibrated or merely
unsharp.  Hersbach's decomposition (Wea. Forecasting 2000) does: CRPS =
reliability + potential CRPS, with the per-rank-bin widths g_i and observed
frequencies o_i -- the quantitative form of the rank histogram -- as a
by-product.  The reference has no counterpart.  `CRPSTable` computes the
sufficient statistic; `crps` and `decomposition` are host arithmetic on it.

One grid point with truth y and the members sorted x_1 <= ... <= x_M, all
arithmetic in float64 after an exact widening, bins i = 0 .. M, p_i = i / M:

  i = 0        alpha = 0                      beta = max(x_1 - y, 0)
  i = M        alpha = max(y - x_M, 0)        beta = 0
  0 < i < M    c = min(max(y, x_i), x_{i+1})  alpha = c - x_i, beta = x_{i+1} - c
  below = [y < x_1], above = [y > x_M]: strict, a tie with an extreme member is
  not an outlier.  The point is INVALID iff the truth or any member is NaN (the
  rule of `events.py`).  Points that hold +-inf are not pinned.

With the dense region weights of the other metrics, W_r[i, j] = w_lat[i] *
lat_mult_r[i] * lon_mult_r[j] (as `events.EventTable`), the table of a cell
(outer index, region) holds the area-weighted means over the valid points of
alpha_i, beta_i, below and above.  skipna=False: a cell with invalid mass is NaN
throughout.  skipna=True: the invalid points are left out; a cell without valid
mass is NaN.

The weights factor, so the points are summed per (row, column class) -- K20
(csrc/crps_bins.hip: `engine.crps_bin_sums`) for device-backed variables,
`host_sums` for host ones -- in ONE fixed order: a sequential float64 chain over
the columns of the class in increasing order.  The fold over the classes and
rows (`engine.crps_bin_fold`, `host_fold`) is ordered too, so the two paths
agree bit for bit.  Regions with a 2-D weight field (`LandRegion`) do not
factor and raise a ValueError.  The kernel takes (latitude, longitude) slabs: a
(longitude, latitude) variable costs one transposing copy here.

Uncertainty and resolution need the pooled climatological distribution of the
observations and are out of scope.
"""
from __future__ import annotations

import dataclasses
import typing as t

import numpy as np

from weatherbench2_amd import class_tables
from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import metrics as _m
from weatherbench2_amd import xarray_lite as xl

MIN_MEMBERS, MAX_MEMBERS = 1, 64  # those of wb2_crps_bins_geometry
TERM, BIN = class_tables.TERM, class_tables.BIN
TERMS = ('alpha', 'beta', 'outlier')


# ---------------------------------------------------------------------------
# the host path: same values, same summation order
# ---------------------------------------------------------------------------
def host_point_terms(x: np.ndarray, y: np.ndarray):
  """(alpha, beta float64 [M + 1, n], below, above, bad bool [n]) of n points:
  `x` [M, n] members, `y` [n] truth.  An invalid point has alpha = beta = 0."""
  x = np.asarray(x).astype(np.float64)
  y = np.asarray(y).astype(np.float64)
  n_member = x.shape[0]
  bad = np.isnan(y) | np.isnan(x).any(axis=0)
  xs = np.sort(np.where(bad[None], 0.0, x), axis=0)
  yv = np.where(bad, 0.0, y)
  alpha = np.zeros((n_member + 1,) + y.shape, dtype=np.float64)
  beta = np.zeros_like(alpha)
  beta[0] = np.maximum(xs[0] - yv, 0.0)
  alpha[n_member] = np.maximum(yv - xs[n_member - 1], 0.0)
  if n_member > 1:
    c = np.minimum(np.maximum(yv[None], xs[:-1]), xs[1:])
    alpha[1:n_member] = c - xs[:-1]
    beta[1:n_member] = xs[1:] - c
  alpha[:, bad] = 0.0
  beta[:, bad] = 0.0
  return alpha, beta, ~bad & (yv < xs[0]), ~bad & (yv > xs[-1]), bad


def host_sums(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
              truth: np.ndarray, truth_slab, n_outer: int, n_row: int,
              n_col: int, col_class, n_class: int) -> tuple:
  """`engine.crps_bin_sums` in NumPy: the same arguments (contiguous host
  arrays instead of tensors), the same (float64 [n_outer, n_row, n_class, 2,
  M + 1], int32 [n_outer, n_row, n_class, 3]) result, the same order: per
  (row, class) one sequential chain over the columns in increasing order."""
  slab = n_row * n_col
  cls = np.asarray(col_class, dtype=np.int64)
  sums = np.zeros((n_outer, n_row, n_class, 2, n_member + 1),
                  dtype=np.float64)
  cnt = np.zeros((n_outer, n_row, n_class, 3), dtype=np.int32)
  for o, x, y in events.host_members(ens, member_stride, n_member, ens_slab,
                                     truth, truth_slab, n_outer, slab):
    alpha, beta, below, above, bad = host_point_terms(x, y)
    # [row, col, term, bin]
    v = np.stack([alpha, beta]).reshape(2, n_member + 1, n_row, n_col
                                        ).transpose(2, 3, 0, 1)
    for j in range(n_col):
      sums[o, :, cls[j]] = sums[o, :, cls[j]] + v[:, j]
    flags = np.stack([below, above, ~bad], axis=-1).reshape(n_row, n_col, 3)
    for c in range(n_class):
      cnt[o, :, c] = flags[:, cls == c].sum(axis=1)
  return sums, cnt


def host_fold(sums: np.ndarray, cnt: np.ndarray, class_cols, wrow: np.ndarray,
              mult: np.ndarray) -> tuple:
  """`engine.crps_bin_fold` in NumPy: the sums as `class_tables.host_fold`
  (classes, then rows, in increasing order from 0.0); the counts (below,
  above, valid, invalid) as `events.host_fold`."""
  invalid = np.asarray(class_cols, dtype=np.int32).reshape(1, 1, -1
                                                           ) - cnt[..., 2]
  cnt4 = np.concatenate([cnt, invalid[..., None].astype(np.int32)], axis=-1)
  return (class_tables.host_fold(sums, wrow, mult),
          events.host_fold(cnt4[None], wrow, mult)[0])


def normalize(table: np.ndarray, counts: np.ndarray, skipna: bool
              ) -> np.ndarray:
  """Region sums [..., 2, M + 1] and weighted counts [..., 4] (below, above,
  valid, invalid) -> [..., 3, M + 1]: the means of alpha and beta over the
  valid mass and the outlier frequencies in bins 0 (below) and M (above)."""
  valid = counts[..., 2]
  out = np.zeros(table.shape[:-2] + (3, table.shape[-1]), dtype=np.float64)
  with np.errstate(all='ignore'):
    out[..., :2, :] = table / valid[..., None, None]
    out[..., 2, 0] = counts[..., 0] / valid
    # (M = 1 has no bin between them; M >= 1 keeps them apart)
    out[..., 2, -1] = counts[..., 1] / valid
  dead = valid == 0.0
  if not skipna:
    dead = dead | (counts[..., 3] != 0.0)
  out[dead] = np.nan
  return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class CRPSTable(class_tables.ClassSumsTable):
  """Per-rank-bin CRPS table of an ensemble forecast.

  Per common variable the result has dims (<outer dims in the order the plain
  CRPS gives them>, 'term', 'bin') -- with `regions=` a leading 'region' dim --,
  term = ('alpha', 'beta', 'outlier'), bin = 0 .. M: the area-weighted means,
  over the valid points of the region, of alpha_i and beta_i; `outlier[0]` is
  the frequency of a truth below every member, `outlier[M]` of one above, the
  bins between are 0.  Attribute: `ensemble_size`.

  `compute` is the time mean of the tables.  The scores are non-linear in the
  table, so they are taken FROM the mean table (`decomposition(metric.compute(
  ...))`) and never averaged themselves.
  """

  ensemble_dim: str = _m.REALIZATION
  # one pass over the points answers every region; no windows of chunks
  _fused_regions = True
  _reads_slabs_in_place = False
  _terms = TERMS

  def _result_attrs(self, forecast):
    return {'ensemble_size': int(forecast.sizes[self.ensemble_dim])}

  def compute_chunk(self, forecast, truth, region=None, skipna=False,
                    regions: t.Optional[dict] = None):
    forecast, truth = _m._inputs(forecast, truth)
    _m._get_n_ensemble(forecast, self.ensemble_dim)
    names = list(_m._common_vars(forecast, truth))
    for name in names:
      fvar = forecast[name]
      if self.ensemble_dim not in fvar.dims:
        raise ValueError(f'variable {name!r} has no {self.ensemble_dim!r} dim')
      class_tables.check_variable(name, fvar, truth[name], self.ensemble_dim,
                                  'the CRPS table', (MIN_MEMBERS, MAX_MEMBERS))

    def values(name, device, args, class_cols, wrow, mult):
      table, counts = class_tables.region_sums(
          device, args, (host_sums, host_fold),
          (engine.crps_bin_sums, engine.crps_bin_fold), class_cols, wrow, mult)
      return normalize(table, counts, skipna)  # [outer, R, 3, M + 1]
    out, n_member = self._tables(forecast, truth, names, region, regions,
                                 lambda n_member: n_member + 1, values)
    return out.assign_attrs(ensemble_size=n_member)


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last two dims of a table
# ---------------------------------------------------------------------------
_per_table = lambda fn: events._per_table(
    fn, trailing=((TERM, 3), (BIN, None)), noun='a CRPS table')


def _probability(p):
  n_member = p.shape[-1] - 1
  return np.arange(n_member + 1, dtype=np.float64) / n_member


@_per_table
def crps(p, dims, coords, fair: bool = False):
  """sum_i alpha_i p_i^2 + beta_i (1 - p_i)^2, p_i = i / M: the CRPS of the
  empirical CDF of the members.  fair=True subtracts sum_{0<i<M} i (M - i)
  (alpha_i + beta_i) / (M^2 (M - 1)), which gives E|X - y| - E|X - X'| / 2
  with the M (M - 1) spread (the reference's `CRPS`); NaN for M = 1."""
  n_member = p.shape[-1] - 1
  y = _probability(p)
  value = (p[..., 0, :] * y ** 2).sum(-1) + (
      p[..., 1, :] * (1.0 - y) ** 2).sum(-1)
  if fair:
    if n_member == 1:
      value = np.full_like(value, np.nan)
    else:
      i = np.arange(n_member + 1, dtype=np.float64)
      w = i * (n_member - i) / (float(n_member) ** 2 * (n_member - 1))
      value = value - ((p[..., 0, :] + p[..., 1, :]) * w).sum(-1)
  return xl.DataArray(value, dims, coords)


@_per_table
def decomposition(p, dims, coords):
  """Hersbach's decomposition: `reliability` sum_i g_i (o_i - p_i)^2 and
  `potential` sum_i g_i o_i (1 - o_i) -- their sum is `crps(table)` -- with the
  bin widths `g` and observed frequencies `o` along `bin`.  Bins 0 < i < M:
  g_i = alpha_i + beta_i, o_i = beta_i / g_i.  Bin 0: o_0 = below, g_0 =
  beta_0 / o_0.  Bin M: o_M = 1 - above, g_M = alpha_M / above.  A bin that is
  never visited (0/0) adds nothing to either sum: an outlier bin without
  outliers has g = o = NaN, an interior bin of width 0 has g = 0 and o = NaN."""
  n_member = p.shape[-1] - 1
  alpha, beta, outlier = p[..., 0, :], p[..., 1, :], p[..., 2, :]
  y = _probability(p)
  g = alpha + beta
  o = beta / g
  below, above = outlier[..., 0], outlier[..., n_member]
  g[..., 0] = beta[..., 0] / below
  o[..., 0] = np.where(below > 0, below, np.nan)
  g[..., n_member] = alpha[..., n_member] / above
  o[..., n_member] = np.where(above > 0, 1.0 - above, np.nan)
  used = ~(np.isnan(g) | np.isnan(o))
  rel = np.where(used, g * (o - y) ** 2, 0.0).sum(-1)
  pot = np.where(used, g * o * (1.0 - o), 0.0).sum(-1)
  nan = np.isnan(p).any(axis=(-2, -1))
  rel, pot = np.where(nan, np.nan, rel), np.where(nan, np.nan, pot)
  bins = dict(coords, **{BIN: np.arange(n_member + 1, dtype=np.int64)})
  out = events._dataset({'reliability': rel, 'potential': pot}, dims, bins)
  for key, value in (('g', g), ('o', o)):
    out.data_vars[key] = xl.DataArray(value, dims + (BIN,), out.coords, key)
  return out
