"""Conditional verification: spread-error reliability and conditional bias.

The other tables average a score over every point of a region; none says under
WHICH CONDITIONS a forecast is good or bad.  `EnsembleVariance`,
`EnsembleMeanMSE` and `compute_spread_skill_ratio` give one number per region:
a ratio near 1 does not say whether large spread predicts large error.  The
standard diagnostic (Leutbecher & Palmer 2008) stratifies the points by the
ensemble spread and compares, per stratum, the mean variance with the mean
squared error of the ensemble mean.  The conditional bias (Murphy & Winkler
1987) compares E[truth | forecast in bin] with the forecast; the same
statistics stratified by the observed value show how bias and error grow
towards observed extremes.  All three are one operation, and the reference has
no counterpart.  `ConditionalTable` computes the sufficient statistic;
`conditional_means`, `spread_error`, `conditional_bias` and `marginal` are host
arithmetic on it.

One grid point with truth y and the members x_0 .. x_{M-1} in STORAGE order
(nothing is sorted), all arithmetic in float64 after an exact widening, no
fused multiply-add:

  S = x_0; S = S + x_m (m = 1 .. M-1);  mu = S / M
  d_m = x_m - mu;  Q = d_0 d_0;  Q = Q + d_m d_m;  s2 = Q / (M - 1)
  (M = 1: s2 = +0.0);  e = mu - y;  se = e e
  v = s2 (by='spread', against the SQUARED edges), mu ('forecast'), y ('truth')
  bin = #{k : edge_k <= v}    (`searchsorted(side='right')`: a value on an edge
                               belongs to the upper bin)

The point is INVALID iff the truth or any member is NaN (the rule of
`events.py`).  Points that hold +-inf are not pinned.

With the dense region weights of the other metrics, W_r[i, j] = w_lat[i] *
lat_mult_r[i] * lon_mult_r[j] (as `events.EventTable`), the table of a cell
(outer index, region) holds, along `term` and per bin b,

  weight         the weighted mass of the valid points of bin b / valid mass
  forecast       sum over the valid points of bin b of W mu / valid mass
  truth, variance, squared_error    likewise with y, s2, se

that is, the means of indicator x value over ALL valid points: the time mean of
tables is the right pooled table.  skipna=False: a cell with invalid mass is
NaN throughout.  skipna=True: the invalid points are left out; a cell without
valid mass is NaN.  An empty bin of a live cell is 0 in every term.

The weights factor, so the points are summed per (row, column class, bin) --
K24 (csrc/conditional_sums.hip: `engine.conditional_sums`) for device-backed
variables, `host_sums` for host ones -- in ONE fixed order: a sequential
float64 chain from +0.0 over the columns of the class in increasing order,
where a point that is invalid or lies in another bin enters as +0.0 (which
changes no bit: such a chain never holds -0.0).  The fold over the classes and
rows (`engine.conditional_fold`, `host_fold`) is ordered too, so the two paths
agree bit for bit.  Regions with a 2-D weight field (`LandRegion`) do not
factor and raise a ValueError.  The kernel takes (latitude, longitude) slabs: a
(longitude, latitude) variable costs one transposing copy here.

Out of scope: choosing the edges automatically, 2-D field regions, more than
64 members, Gaussian forecasts, a second conditioning variable and an external
conditioning field.
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

MIN_MEMBERS, MAX_MEMBERS = 1, 64  # those of wb2_conditional_geometry
MAX_EDGES = 63                    # likewise: at most 64 bins
BYS = ('spread', 'forecast', 'truth')
TERM, BIN = class_tables.TERM, class_tables.BIN
TERMS = ('weight', 'forecast', 'truth', 'variance', 'squared_error')
_NOUN = 'conditional table'


# ---------------------------------------------------------------------------
# the edges
# ---------------------------------------------------------------------------
def kernel_edges(edges, by: str) -> np.ndarray:
  """The float64 edges the sums compare against, from the edges as given:
  finite and strictly increasing, at most 63; for by='spread' they are standard
  deviations >= 0 and come back SQUARED (once, in float64), and the squares
  must still be strictly increasing.  Every violation is a ValueError."""
  try:
    e = np.asarray(edges, dtype=np.float64)
  except (TypeError, ValueError):
    raise ValueError(f'the bin edges of the {_NOUN} must be numbers') from None
  if e.ndim != 1:
    raise ValueError(f'the bin edges of the {_NOUN} must be a 1-D sequence')
  if e.size > MAX_EDGES:
    raise ValueError(f'{e.size} bin edges: the {_NOUN} takes 0 to {MAX_EDGES}')
  if not np.isfinite(e).all():
    raise ValueError(f'the bin edges of the {_NOUN} must be finite')
  if (e[1:] <= e[:-1]).any():
    raise ValueError(f'the bin edges of the {_NOUN} must be strictly '
                     'increasing')
  if by == 'spread':
    if (e < 0).any():
      raise ValueError('by=\'spread\': the bin edges are standard deviations '
                       'and must be >= 0')
    with np.errstate(over='ignore'):
      e = e * e
    if not np.isfinite(e).all() or (e[1:] <= e[:-1]).any():
      raise ValueError('by=\'spread\': the squared bin edges must be finite '
                       'and still strictly increasing')
  return np.ascontiguousarray(e)


# ---------------------------------------------------------------------------
# the host path: same values, same summation order
# ---------------------------------------------------------------------------
def host_point_terms(x: np.ndarray, y: np.ndarray):
  """(mu, s2, se float64 [n], bad bool [n]) of n points: `x` [M, n] members in
  storage order, `y` [n] truth.  An explicit loop over the members: the order
  is the contract.  The values of an invalid point are NaN."""
  x = np.asarray(x).astype(np.float64)
  y = np.asarray(y).astype(np.float64)
  n_member = x.shape[0]
  bad = np.isnan(y) | np.isnan(x).any(axis=0)
  with np.errstate(all='ignore'):
    s = x[0].copy()
    for m in range(1, n_member):
      s = s + x[m]
    mu = s / float(n_member)
    d = x[0] - mu
    q = d * d
    for m in range(1, n_member):
      d = x[m] - mu
      q = q + d * d
    s2 = q / float(n_member - 1) if n_member > 1 else np.zeros_like(q)
    e = mu - y
    se = e * e
  return mu, s2, se, bad


def host_bins(v: np.ndarray, edges: np.ndarray) -> np.ndarray:
  """#{k : edges[k] <= v} per point (a NaN lies in bin 0)."""
  with np.errstate(invalid='ignore'):
    return (np.asarray(edges, np.float64).reshape(-1, 1) <= v[None]
            ).sum(axis=0).astype(np.int64)


def host_sums(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
              truth: np.ndarray, truth_slab, n_outer: int, n_row: int,
              n_col: int, col_class, n_class: int, mode, edges) -> tuple:
  """`engine.conditional_sums` in NumPy: the same arguments (contiguous host
  arrays instead of tensors), the same (float64 [n_outer, n_row, n_class,
  n_bin, 4], int32 [n_outer, n_row, n_class, n_bin]) result, the same order:
  per (row, class, bin, term) one sequential chain over the columns in
  increasing order, +0.0 for a point that is invalid or in another bin."""
  mode = engine.CONDITIONAL_MODES.get(mode, mode)
  edges = engine.conditional_edges(edges, MAX_EDGES)
  n_bin = edges.size + 1
  slab = n_row * n_col
  cls = np.asarray(col_class, dtype=np.int64)
  sums = np.zeros((n_outer, n_row, n_class, n_bin, 4), dtype=np.float64)
  cnt = np.zeros((n_outer, n_row, n_class, n_bin), dtype=np.int32)
  rows = np.arange(n_row)
  for o, x, y in events.host_members(ens, member_stride, n_member, ens_slab,
                                     truth, truth_slab, n_outer, slab):
    y = y.astype(np.float64)
    mu, s2, se, bad = host_point_terms(x, y)
    which = host_bins((s2, mu, y)[mode], edges).reshape(n_row, n_col)
    ok = ~bad.reshape(n_row, n_col)
    v = np.stack([mu, y, s2, se], axis=-1).reshape(n_row, n_col, 4)
    for j in range(n_col):
      add = np.zeros((n_row, n_bin, 4), dtype=np.float64)
      live = ok[:, j]
      add[rows[live], which[live, j]] = v[live, j]
      sums[o, :, cls[j]] = sums[o, :, cls[j]] + add
      cnt[o, rows[live], cls[j], which[live, j]] += 1
  return sums, cnt


def host_fold(sums: np.ndarray, cnt: np.ndarray, class_cols, wrow: np.ndarray,
              mult: np.ndarray) -> tuple:
  """`engine.conditional_fold` in NumPy: the sums as `class_tables.host_fold`
  (classes, then rows, in increasing order from 0.0); the counts (the bins,
  then invalid) as `events.host_fold`."""
  invalid = np.asarray(class_cols, dtype=np.int64).reshape(1, 1, -1
                                                           ) - cnt.sum(axis=-1)
  codes = np.concatenate([cnt, invalid[..., None].astype(np.int32)], axis=-1)
  return (class_tables.host_fold(sums, wrow, mult),
          events.host_fold(codes[None], wrow, mult)[0])


def normalize(table: np.ndarray, counts: np.ndarray, skipna: bool
              ) -> np.ndarray:
  """Region sums [..., B, 4] and weighted counts [..., B + 1] (the bins, then
  invalid) -> [..., 5, B]: the bins' masses and sums over the valid mass, the
  valid mass summed over the bins in increasing order."""
  n_bin = table.shape[-2]
  valid = np.zeros(counts.shape[:-1], dtype=np.float64)
  for b in range(n_bin):
    valid = valid + counts[..., b]
  out = np.zeros(table.shape[:-2] + (len(TERMS), n_bin), dtype=np.float64)
  with np.errstate(all='ignore'):
    out[..., 0, :] = counts[..., :n_bin] / valid[..., None]
    out[..., 1:, :] = np.swapaxes(table, -1, -2) / valid[..., None, None]
  dead = valid == 0.0
  if not skipna:
    dead = dead | (counts[..., n_bin] != 0.0)
  out[dead] = np.nan
  return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class ConditionalTable(class_tables.ClassSumsTable):
  """Per-bin table of forecast, truth, variance and squared error.

  `by` is what the points are binned by: 'spread' (the ensemble standard
  deviation), 'forecast' (the ensemble mean) or 'truth'.  `bin_edges` is a 1-D
  sequence of E edges, 0 <= E <= 63, or {variable: sequence}: finite, strictly
  increasing, in the variable's units ('spread': standard deviations >= 0,
  squared once on the host); B = E + 1 bins, the first and the last open-ended.
  A forecast variable without `ensemble_dim` (or ensemble_dim=None) is a
  deterministic forecast, M = 1: its variance is +0.0 and by='spread' is a
  ValueError.

  Per common variable the result has dims (<outer dims in the order
  `crps_decomposition.CRPSTable` gives them>, 'term', 'bin') -- with `regions=`
  a leading 'region' dim --, term = ('weight', 'forecast', 'truth', 'variance',
  'squared_error'), bin = 0 .. B - 1 (module docstring).  Attributes:
  `ensemble_size`, `by`, `bin_edges` (as given, a tuple or a dict of tuples).

  `compute` is the time mean of the tables.  The scores are non-linear in the
  table, so they are taken FROM the mean table (`spread_error(metric.compute(
  ...))`) and never averaged themselves.
  """

  bin_edges: t.Any = ()
  by: str = 'spread'
  ensemble_dim: t.Optional[str] = _m.REALIZATION
  # one pass over the points answers every region; no windows of chunks
  _fused_regions = True
  _reads_slabs_in_place = False
  _terms = TERMS

  def __post_init__(self):
    self._checked(None)

  def _checked(self, names) -> dict:
    """{variable: squared-or-plain float64 edges} after every check that needs
    no data (names=None: only what is given is checked)."""
    if self.by not in BYS:
      raise ValueError(f'by={self.by!r}: the {_NOUN} takes '
                       f'{", ".join(map(repr, BYS))}')
    if isinstance(self.bin_edges, t.Mapping):
      given = dict(self.bin_edges)
      for name in names or ():
        if name not in given:
          raise ValueError(f'bin_edges has no entry for variable {name!r}')
      names = given if names is None else names
      return {name: kernel_edges(given[name], self.by) for name in names}
    e = kernel_edges(self.bin_edges, self.by)
    return {name: e for name in names or ()}

  def _edges_attr(self):
    as_tuple = lambda e: tuple(float(v) for v in np.asarray(
        e, dtype=np.float64).reshape(-1))
    if isinstance(self.bin_edges, t.Mapping):
      return {k: as_tuple(e) for k, e in self.bin_edges.items()}
    return as_tuple(self.bin_edges)

  def _result_attrs(self, forecast):
    return {'ensemble_size': self._ensemble_size(forecast), 'by': self.by,
            'bin_edges': self._edges_attr()}

  def compute_chunk(self, forecast, truth, region=None, skipna=False,
                    regions: t.Optional[dict] = None):
    forecast, truth = _m._inputs(forecast, truth)
    names = list(_m._common_vars(forecast, truth))
    edges = self._checked(names)
    n_bins = {e.size + 1 for e in edges.values()}
    if len(n_bins) > 1:
      raise ValueError(f'the variables differ in the number of bins: {n_bins}')
    # every check of the variables before anything is launched
    for name in names:
      n_member = class_tables.check_variable(
          name, forecast[name], truth[name], self.ensemble_dim,
          f'the {_NOUN}', (MIN_MEMBERS, MAX_MEMBERS))
      if n_member == 1 and self.by == 'spread':
        raise ValueError(f'variable {name!r} has one member: by=\'spread\' '
                         'needs an ensemble')
    def values(name, device, args, class_cols, wrow, mult):
      table, counts = class_tables.region_sums(
          device, args + (self.by, edges[name]), (host_sums, host_fold),
          (engine.conditional_sums, engine.conditional_fold), class_cols, wrow,
          mult)
      return normalize(table, counts, skipna)  # [outer, R, 5, B]
    n_bin = n_bins.pop() if n_bins else 1
    out, n_member = self._tables(forecast, truth, names, region, regions,
                                 lambda n_member: n_bin, values)
    return out.assign_attrs(ensemble_size=n_member, by=self.by,
                            bin_edges=self._edges_attr())


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last two dims of a table
# ---------------------------------------------------------------------------
class _ByVariable(dict):
  """{variable: result Dataset} of a table Dataset.  A FIELD of the results
  asked of it (`spread_error(tables)['ratio']`) is the Dataset of that field
  of every variable -- what `bootstrap.bootstrap` takes from a score function.
  (A variable named like a field is found as the variable.)"""

  def __missing__(self, key):
    if not self or any(key not in r.data_vars for r in self.values()):
      raise KeyError(key)
    coords = {}
    for r in self.values():
      coords.update(r.coords)
    return xl.Dataset({name: r[key] for name, r in self.items()}, coords)


def _per_table(fn):
  inner = events._per_table(fn, trailing=((TERM, len(TERMS)), (BIN, None)),
                            noun='a conditional table')

  def wrapper(table, *args, **kwargs):
    out = inner(table, *args, **kwargs)
    return _ByVariable(out) if isinstance(out, dict) else out
  wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
  return wrapper


def _bins(p, coords):
  return dict(coords, **{BIN: np.arange(p.shape[-1], dtype=np.int64)})


@_per_table
def conditional_means(p, dims, coords):
  """Per bin: `forecast`, `truth`, `variance` and `mse`, each the term divided
  by `weight` (the conditional means E[. | bin]; NaN in an empty bin), and
  `weight` itself."""
  w = p[..., 0, :]
  return events._dataset(
      {'forecast': p[..., 1, :] / w, 'truth': p[..., 2, :] / w,
       'variance': p[..., 3, :] / w, 'mse': p[..., 4, :] / w, 'weight': w},
      dims + (BIN,), _bins(p, coords))


@_per_table
def _spread_error(p, dims, coords, n_member=None):
  w = p[..., 0, :]
  variance, mse = p[..., 3, :] / w, p[..., 4, :] / w
  if n_member is not None:
    if n_member > 1:
      mse = mse - p[..., 3, :] / (w * float(n_member))
      mse = np.where(mse < 0, np.nan, mse)
    else:
      mse = np.full_like(mse, np.nan)
  spread, error = np.sqrt(variance), np.sqrt(mse)
  return events._dataset({'spread': spread, 'error': error,
                          'ratio': spread / error},
                         dims + (BIN,), _bins(p, coords))


def spread_error(table, debiased: bool = False,
                 ensemble_size: t.Optional[int] = None):
  """Per bin: `spread` = sqrt(variance / weight), `error` = sqrt(mse) with mse
  = squared_error / weight, and `ratio` = spread / error (Leutbecher & Palmer
  2008: a reliable ensemble has ratio 1 in EVERY spread bin).  debiased=True:
  error = sqrt(mse - variance / (weight M)), the reference's
  `DebiasedEnsembleMeanMSE` per bin; NaN where the argument is negative or M =
  1.  M is the table's `ensemble_size` attribute unless `ensemble_size` is
  given (a DataArray carries none).  Every 0/0 is NaN."""
  n_member = None
  if debiased:
    n_member = ensemble_size
    if n_member is None:
      n_member = getattr(table, 'attrs', {}).get('ensemble_size')
    if n_member is None:
      raise ValueError('debiased=True needs the ensemble size: pass the table '
                       'Dataset with its `ensemble_size` attribute, or '
                       'ensemble_size=')
    n_member = int(n_member)
  return _spread_error(table, n_member)


@_per_table
def conditional_bias(p, dims, coords):
  """Per bin: forecast / weight - truth / weight, E[forecast - truth | bin]
  (the sign of the reference's `Bias`); NaN in an empty bin."""
  w = p[..., 0, :]
  return xl.DataArray(p[..., 1, :] / w - p[..., 2, :] / w, dims + (BIN,),
                      _bins(p, coords))


@_per_table
def marginal(p, dims, coords):
  """The sum over the bins of each term, in increasing bin order: `weight` (1
  for a live cell), `forecast`, `truth`, `variance` (the reference's
  `EnsembleVariance`), `squared_error` (`EnsembleMeanMSE`) and `bias` =
  forecast - truth (`Bias`)."""
  total = np.zeros(p.shape[:-1], dtype=np.float64)
  for b in range(p.shape[-1]):
    total = total + p[..., b]
  fields = {name: total[..., k] for k, name in enumerate(TERMS)}
  fields['bias'] = total[..., 1] - total[..., 2]
  return events._dataset(fields, dims, coords)
