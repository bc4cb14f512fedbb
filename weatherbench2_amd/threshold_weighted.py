"""Threshold-weighted CRPS: the tail scores of an ensemble from one sort.

For an event `x > threshold` the event tables (`events.EventTable`,
`neighborhood.FractionsTable`) score the PROBABILITY of exceedance.  They do
not say how good the ensemble's distribution is within the tail.  The proper
score for that is the threshold-weighted CRPS (twCRPS; Gneiting & Ranjan 2011,
in the chaining-function form of Allen, Ginsbourger & Ziegel 2023) with the
weight 1[z >= t] (upper tail) or 1[z <= t] (lower tail).  The reference has
no counterpart.  `ThresholdWeightedCRPS` computes its two terms per threshold;
`twcrps` and `twcrpss` are host arithmetic on them.

One grid point with truth y, the members sorted x_1 <= ... <= x_M and the
threshold value t (`Threshold.compute(truth)` at the point), all arithmetic in
float64 after an exact widening, v(z) = max(z, t) (`upper`) or min(z, t)
(`lower`):

  A = sum_{i=1..M} |v(x_i) - v(y)|           in sorted-member order from 0.0
  B = sum_{k=1..M-1} k (M - k) (v(x_{k+1}) - v(x_k))   in increasing k from 0.0
  twCRPS = A / M - B / M^2

B is the gap form of sum_{i<j} |v(x_i) - v(x_j)|: every term is >= 0, the
integer factor is exact and a gap wholly beyond the threshold is exactly 0.
v is monotone, so clamping keeps the sorted order: the members are read once
and sorted once, and every threshold is one O(M) pass.  The point is INVALID
FOR A THRESHOLD iff the truth, any member or that threshold's value is NaN
(the rule of `events.py`, per threshold).  t = -inf (`upper`) and t = +inf
(`lower`) are ordinary values and give the plain CRPS terms; any other +-inf
in the threshold, the truth or the members is not pinned.

With the dense region weights of the other metrics, W_r[i, j] = w_lat[i] *
lat_mult_r[i] * lon_mult_r[j] (as `events.EventTable`), the table of a cell
(threshold, outer index, region) holds, along `term`,

  abs_error      the area-weighted mean over the valid points of A / M
  pair_distance  the area-weighted mean over the valid points of B / M^2

(the divisions by M and M^2 are done once, after the fold).  skipna=False: a
cell with invalid mass for that threshold is NaN.  skipna=True: the invalid
points are left out; a cell without valid mass is NaN.

The weights factor, so the points are summed per (threshold, row, column
class) -- K21 (csrc/twcrps.hip: `engine.twcrps_sums`) for device-backed
variables, `host_sums` for host ones -- in ONE fixed order: a sequential
float64 chain over the columns of the class in increasing order, where a point
that is invalid for the threshold enters as +0.0 (which changes no bit of a
sum of non-negative terms).  The fold over the classes and rows
(`engine.twcrps_fold`, `host_fold`) is ordered too, so the two paths agree bit
for bit.  Regions with a 2-D weight field (`LandRegion`) do not factor and
raise a ValueError.  The kernel takes (latitude, longitude) slabs: a
(longitude, latitude) variable costs one transposing copy here.

Interval and smooth weight functions, Gaussian forecasts and a per-point map
are out of scope.
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

MIN_MEMBERS, MAX_MEMBERS = 1, 64  # those of wb2_twcrps_geometry
TAILS = ('upper', 'lower')
TERM = 'term'
TERMS = ('abs_error', 'pair_distance')


# ---------------------------------------------------------------------------
# the host path: same values, same summation order
# ---------------------------------------------------------------------------
def host_point_terms(x: np.ndarray, y: np.ndarray, thr: np.ndarray,
                     lower: bool = False):
  """(A, B float64 [n], bad bool [n]) of n points: `x` [M, n] members, `y` [n]
  truth, `thr` [n] threshold values.  An invalid point has A = B = +0.0."""
  x = np.asarray(x).astype(np.float64)
  y = np.asarray(y).astype(np.float64)
  thr = np.asarray(thr).astype(np.float64)
  n_member = x.shape[0]
  bad = np.isnan(y) | np.isnan(x).any(axis=0) | np.isnan(thr)
  xs = np.sort(np.where(bad[None], 0.0, x), axis=0)
  yv, tv = np.where(bad, 0.0, y), np.where(bad, 0.0, thr)
  if lower:
    clamp = lambda z: np.where(z > tv, tv, z)
  else:
    clamp = lambda z: np.where(z < tv, tv, z)
  vy = clamp(yv)
  a, b = np.zeros(y.shape, np.float64), np.zeros(y.shape, np.float64)
  prev = None
  with np.errstate(invalid='ignore'):
    for m in range(n_member):
      v = clamp(xs[m])
      a = a + np.abs(v - vy)
      if m > 0:
        b = b + float(m * (n_member - m)) * (v - prev)
      prev = v
  a[bad] = 0.0
  b[bad] = 0.0
  return a, b, bad


def host_sums(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
              truth: np.ndarray, truth_slab, thresholds, thr_slabs,
              n_outer: int, n_row: int, n_col: int, col_class, n_class: int,
              lower: bool = False) -> tuple:
  """`engine.twcrps_sums` in NumPy: the same arguments (contiguous host arrays
  instead of tensors), the same (float64 [n_threshold, n_outer, n_row, n_class,
  2], int32 [n_threshold, n_outer, n_row, n_class, 1]) result, the same order:
  per (threshold, row, class, term) one sequential chain over the columns in
  increasing order, +0.0 for a point that is invalid for the threshold."""
  thresholds = list(thresholds)
  thr_slabs = (list(thr_slabs) if thr_slabs is not None
               else [None] * len(thresholds))
  slab = n_row * n_col
  cls = np.asarray(col_class, dtype=np.int64)
  sums = np.zeros((len(thresholds), n_outer, n_row, n_class, 2),
                  dtype=np.float64)
  cnt = np.zeros((len(thresholds), n_outer, n_row, n_class, 1),
                 dtype=np.int32)
  for o, x, y in events.host_members(ens, member_stride, n_member, ens_slab,
                                     truth, truth_slab, n_outer, slab):
    for ti, (thr, table) in enumerate(zip(thresholds, thr_slabs)):
      a, b, bad = host_point_terms(
          x, y, events.host_slab(thr.reshape(-1), table, o, slab), lower)
      v = np.stack([a, b], axis=-1).reshape(n_row, n_col, 2)
      for j in range(n_col):
        sums[ti, o, :, cls[j]] = sums[ti, o, :, cls[j]] + v[:, j]
      ok = ~bad.reshape(n_row, n_col)
      for c in range(n_class):
        cnt[ti, o, :, c, 0] = ok[:, cls == c].sum(axis=1)
  return sums, cnt


def host_fold(sums: np.ndarray, cnt: np.ndarray, class_cols, wrow: np.ndarray,
              mult: np.ndarray) -> tuple:
  """`engine.twcrps_fold` in NumPy: the sums as `class_tables.host_fold`
  (classes, then rows, in increasing order from 0.0); the counts (valid,
  invalid) as `events.host_fold`."""
  invalid = np.asarray(class_cols, dtype=np.int32).reshape(1, 1, 1, -1, 1
                                                           ) - cnt
  cnt2 = np.concatenate([cnt, invalid.astype(np.int32)], axis=-1)
  return (class_tables.host_fold(sums, wrow, mult, n_lead=2),
          events.host_fold(cnt2, wrow, mult))


def normalize(table: np.ndarray, counts: np.ndarray, n_member: int,
              skipna: bool) -> np.ndarray:
  """Region sums [..., 2] (A, B) and weighted counts [..., 2] (valid, invalid)
  -> [..., 2]: the means over the valid mass of A / M and B / M^2."""
  valid = counts[..., 0]
  with np.errstate(all='ignore'):
    out = table / valid[..., None]
    out[..., 0] = out[..., 0] / float(n_member)
    out[..., 1] = out[..., 1] / float(n_member * n_member)
  dead = valid == 0.0
  if not skipna:
    dead = dead | (counts[..., 1] != 0.0)
  out[dead] = np.nan
  return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class ThresholdWeightedCRPS(events.ExceedanceTable):
  """Threshold-weighted CRPS terms of a forecast against thresholds.

  Per common variable the result has dims ('quantile', <outer dims as
  `events.EventTable` orders them>, 'term') -- with `regions=` a leading
  'region' dim --, term = ('abs_error', 'pair_distance'): the area-weighted
  means, over the points of the region that are valid for the threshold, of
  A / M and B / M^2 (module docstring).  `tail` is 'upper' (the weight
  1[z >= t], v = max(z, t)) or 'lower' (1[z <= t], v = min(z, t)).  Any
  `thresholds.Threshold` works, `neighborhood.ConstantThreshold` included.  A
  forecast variable without `ensemble_dim` (or ensemble_dim=None) is a
  deterministic forecast, M = 1: the table is then a threshold-weighted
  absolute error.  Attributes: `threshold_method`, `ensemble_size`, `tail`.

  `compute` is the time mean of the tables.  Skill scores are non-linear in
  the table, so they are taken FROM the mean table (`twcrpss(metric.compute(
  ...), ...)`) and never averaged themselves.
  """

  thresholds: t.Sequence = ()
  tail: str = 'upper'
  ensemble_dim: t.Optional[str] = _m.REALIZATION
  # one pass over the points answers every region; no windows of chunks
  _fused_regions = True
  _reads_slabs_in_place = False
  _noun = 'threshold-weighted CRPS'
  _trailing_dims = (TERM,)

  def _result_attrs(self, forecast):
    return {'ensemble_size': self._ensemble_size(forecast), 'tail': self.tail}

  def compute_chunk(self, forecast, truth, region=None, skipna=False,
                    regions: t.Optional[dict] = None):
    forecast, truth = _m._inputs(forecast, truth)
    if self.tail not in TAILS:
      raise ValueError(f'tail={self.tail!r}: the {self._noun} takes '
                       f'{" or ".join(map(repr, TAILS))}')
    for name in _m._common_vars(forecast, truth):
      class_tables.check_variable(
          name, forecast[name], truth[name], self.ensemble_dim,
          f'the {self._noun}', (MIN_MEMBERS, MAX_MEMBERS))
    out = events.ExceedanceTable.compute_chunk.__wrapped__(
        self, forecast, truth, region, skipna, regions)
    return out.assign_attrs(tail=self.tail)

  def _values(self, ops, n_row, n_col, col_class, mult, wrow, skipna, setup):
    class_cols = np.bincount(col_class, minlength=mult.shape[1])
    args = ops.front(n_row, n_col) + (col_class, mult.shape[1],
                                      self.tail == 'lower')
    table, counts = class_tables.region_sums(
        ops.device, args, (host_sums, host_fold),
        (engine.twcrps_sums, engine.twcrps_fold), class_cols, wrow, mult)
    return normalize(table, counts, ops.n_member, skipna)  # [T, outer, R, 2]

  def _extra_coords(self, n_member, setup):
    return {TERM: np.array(TERMS, dtype=object)}


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last dim of a table
# ---------------------------------------------------------------------------
_per_table = lambda fn: events._per_table(fn, trailing=((TERM, 2),),
                                          noun='a twCRPS table')


def _ensemble_size(table, ensemble_size) -> int:
  if ensemble_size is None:
    ensemble_size = getattr(table, 'attrs', {}).get('ensemble_size')
  if ensemble_size is None:
    raise ValueError('fair=True needs the ensemble size: pass the table '
                     'Dataset with its `ensemble_size` attribute, or '
                     'ensemble_size=')
  return int(ensemble_size)


@_per_table
def _twcrps(p, dims, coords, n_member=None):
  pair = p[..., 1]
  if n_member is not None:
    pair = (pair * (float(n_member) / float(n_member - 1)) if n_member > 1
            else np.full_like(pair, np.nan))
  return xl.DataArray(p[..., 0] - pair, dims, coords)


def twcrps(table, fair: bool = False, ensemble_size: t.Optional[int] = None):
  """abs_error - pair_distance: the twCRPS of the empirical distribution of
  the members.  fair=True: abs_error - pair_distance * M / (M - 1), the
  estimator of the reference's `CRPS` (E|X - y| - E|X - X'| / 2 with the
  M (M - 1) spread); NaN for M = 1.  M is the table's `ensemble_size`
  attribute unless `ensemble_size` is given (a DataArray carries none)."""
  return _twcrps(table, _ensemble_size(table, ensemble_size) if fair else None)


def twcrpss(table, reference_table, fair: bool = False,
            ensemble_size: t.Optional[int] = None,
            reference_ensemble_size: t.Optional[int] = None):
  """1 - twcrps(table) / twcrps(reference_table): the skill over a reference
  forecast (a climatological ensemble, say) under the same thresholds and
  tail; 0 / 0 is NaN.  `fair` and the ensemble sizes are those of `twcrps`,
  each table with its own."""
  score = twcrps(table, fair, ensemble_size)
  ref = twcrps(reference_table, fair, reference_ensemble_size)

  def skill(a, b):
    with np.errstate(all='ignore'):
      return xl.DataArray(
          1.0 - np.asarray(a.values, np.float64) /
          np.asarray(b.values, np.float64), a.dims, a.coords, a.name)
  if isinstance(score, xl.DataArray):
    return skill(score, ref)
  return xl.Dataset({k: skill(score[k], ref[k]) for k in score.data_vars},
                    score.coords, score.attrs)
