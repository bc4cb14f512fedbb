"""Quantile and interval verification: the pinball tables.

Every table here so far scores a forecast through its members (CRPS, its
decomposition, the tail scores) or through events.  None scores the QUANTILES
of a forecast: the pinball (quantile) loss -- the elementary score of the CRPS
--, the reliability of a quantile (how often the truth lies below it) and the
coverage, width and interval score (Winkler 1972; Gneiting & Raftery 2007) of
central prediction intervals.  And the forecasts that ARE quantiles --
`quantiles.py`'s output, the quantile climatology -- could not be scored at
all.  The reference has no counterpart.  `QuantileScoreTable` computes the
sufficient statistic; `quantile_score`, `observed_frequency`, `interval_width`,
`interval_coverage`, `interval_score`, `quantile_skill` and
`crps_from_quantiles` are host arithmetic on it.

ENSEMBLE mode (a variable with `ensemble_dim`; without it M = 1).  The members
are sorted x_0 <= ... <= x_{M-1}.  Level tau has the 0-based position v,
clamped to [0, M - 1]: tau (M - 1) for method 'linear' (xarray's default), M
tau - 1/2 for 'hazen', (M + 1) tau - 1 for 'weibull', in float64 on the host
(`engine.quantile_score_levels`).  lo = floor(v), t = v - lo, hi = min(lo + 1,
M - 1), and the quantile is `quantiles.py`'s interpolation: d = x_hi - x_lo in
the DATA's dtype, q = x_lo + d t where t < 1/2 and q = x_hi - d (1 - t)
otherwise, in float64.  With 'linear' q is bit-equal to `quantiles.quantile(
forecast, levels, dim=ensemble_dim)` wherever no member is NaN.

DIRECT mode (`quantile_dim` is given and a dim of the variable).  The values
along that dim are the quantile forecasts, its coordinate the levels (strictly
increasing, within [0, 1]; `levels` must be None or equal to it within 1e-12).
Nothing is sorted and nothing interpolated.  Monotone quantiles are assumed
and not checked; `interval_coverage` is stated for monotone ones.

Per valid point and level, in float64 after an exact widening, no fused
multiply-add:

  u = y - q;  pinball = tau u (u >= 0), (1 - tau) (-u) otherwise
  below = [y < q],  tie = [y == q]      (IEEE compares: -0.0 ties with +0.0)

with 1 - tau rounded once on the host.  A point is INVALID iff the truth or
any member (direct: any quantile value) is NaN (the rule of `events.py`).
Points that hold +-inf are not pinned.

The table of a cell (outer index, region) holds, along `term` and per level,
the area-weighted means over the valid points of

  pinball            the quantile score of that level
  forecast_quantile  q
  below, tie         the weighted frequencies of y < q and y == q

skipna=False: a cell with invalid mass is NaN.  skipna=True: the invalid
points are left out.  A cell without valid mass is NaN.

The weights factor, so the points are summed per (row, column class, level) --
K28 (csrc/quantile_score.hip: `engine.quantile_score_sums`) for device-backed
variables, `host_sums` for host ones -- in ONE fixed order: a sequential
float64 chain from +0.0 over the columns in increasing order, where an invalid
point enters as +0.0.  The fold over the classes and rows
(`engine.quantile_score_fold`, `host_fold`) is ordered too, so the two paths
agree bit for bit.  Regions with a 2-D weight field (`LandRegion`) do not
factor and raise a ValueError.  The kernel takes (latitude, longitude) slabs:
a (longitude, latitude) variable costs one transposing copy here.  In ensemble
mode more than 16 levels become further launches of up to 16.

Out of scope: the quantile-score decomposition, weighted quantile scores,
checking for quantile crossing, chunk programs and windows, Gaussian
forecasts.
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

# those of wb2_quantile_score_geometry
MIN_MEMBERS, MAX_MEMBERS = 1, engine.QUANTILE_SCORE_MAX_MEMBER
MAX_LEVELS = engine.QUANTILE_SCORE_MAX_LEVELS
MAX_DIRECT_LEVELS = engine.QUANTILE_SCORE_LAUNCH_LEVELS
METHODS = engine.QUANTILE_SCORE_METHODS
DEFAULT_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
TERM, LEVEL, INTERVAL = class_tables.TERM, 'level', 'interval'
TERMS = ('pinball', 'forecast_quantile', 'below', 'tie')
TIES = {'below': 0.0, 'half': 0.5, 'above': 1.0}
LEVEL_TOL = 1e-12
_NOUN = 'quantile score table'


def checked_method(method) -> str:
  if method not in METHODS:
    raise ValueError(f'method={method!r}: the {_NOUN} takes '
                     f'{", ".join(map(repr, METHODS))}')
  return method


def checked_levels(levels, direct: bool = False) -> np.ndarray:
  """`levels` as float64 [L] after every check that needs no data
  (`engine.quantile_score_levels`): finite, within [0, 1], strictly
  increasing, at most 64 (direct: 16).  Every violation is a ValueError."""
  # (direct: as many "members" as levels; their number is checked first)
  n_member = min(max(int(np.size(levels)), 1), MAX_MEMBERS) if direct else 1
  return engine.quantile_score_levels(levels, n_member, 'linear', direct)[3]


# ---------------------------------------------------------------------------
# the host path: same values, same summation order
# ---------------------------------------------------------------------------
def host_terms(x: np.ndarray, y: np.ndarray, tables, direct: bool = False
               ) -> tuple:
  """The per-point terms of `engine.quantile_score_sums` in NumPy: members x
  [M, ...] and truth y [...] of the data's dtype -> (pinball, q float64 [...,
  L], below, tie bool [..., L], ok bool [...]); the values of an invalid point
  are not defined."""
  lo, hi, tt, tau, omt = tables
  ok = ~(np.isnan(y) | np.isnan(x).any(axis=0))
  s = x if direct else np.sort(x, axis=0)  # (NaN last: the point is invalid)
  yd = y.astype(np.float64)
  shape = y.shape + (len(lo),)
  pin, q = np.empty(shape), np.empty(shape)
  below, tie = np.empty(shape, dtype=bool), np.empty(shape, dtype=bool)
  with np.errstate(all='ignore'):
    for l in range(len(lo)):
      a, b = s[lo[l]], s[hi[l]]
      if direct:
        ql = a.astype(np.float64)
      else:
        d = (b - a).astype(np.float64)  # (the difference in the data's dtype)
        low = a.astype(np.float64) + d * tt[l]
        high = b.astype(np.float64) - d * (1.0 - tt[l])
        ql = low if tt[l] < 0.5 else high
      u = yd - ql
      pin[..., l] = np.where(u >= 0.0, tau[l] * u, omt[l] * (-u))
      q[..., l] = ql
      below[..., l] = yd < ql
      tie[..., l] = yd == ql
  return pin, q, below, tie, ok


def host_sums(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
              truth: np.ndarray, truth_slab, n_outer: int, n_row: int,
              n_col: int, col_class, n_class: int, tables,
              direct: bool = False) -> tuple:
  """`engine.quantile_score_sums` in NumPy: the same arguments (contiguous host
  arrays instead of tensors), the same (float64 [n_outer, n_row, n_class,
  n_level, 2], int32 [n_outer, n_row, n_class, n_level, 2], int32 [n_outer,
  n_row, n_class, 2]) result, the same order: per (row, class, level, term)
  one sequential chain over the columns in increasing order, +0.0 for an
  invalid point."""
  tables = engine._quantile_score_tables(tables, n_member, direct)
  n_level = tables[0].size
  cls = np.asarray(col_class, dtype=np.int64)
  sums = np.zeros((n_outer, n_row, n_class, n_level, 2), dtype=np.float64)
  cnt = np.zeros((n_outer, n_row, n_class, n_level, 2), dtype=np.int32)
  valid = np.zeros((n_outer, n_row, n_class, 2), dtype=np.int32)
  for o, x, y in events.host_members(ens, member_stride, n_member, ens_slab,
                                     truth, truth_slab, n_outer,
                                     n_row * n_col):
    pin, q, below, tie, ok = host_terms(
        x.reshape(n_member, n_row, n_col), y.reshape(n_row, n_col), tables,
        direct)
    good = ok[..., None]
    val = np.stack([np.where(good, pin, 0.0), np.where(good, q, 0.0)], axis=-1)
    state = np.stack([good & below, good & tie], axis=-1).astype(np.int32)
    okay = np.stack([ok, ~ok], axis=-1).astype(np.int32)
    for j in range(n_col):
      sums[o, :, cls[j]] = sums[o, :, cls[j]] + val[:, j]
      cnt[o, :, cls[j]] += state[:, j]
      valid[o, :, cls[j]] += okay[:, j]
  return sums, cnt, valid


def host_fold(sums: np.ndarray, cnt: np.ndarray, valid: np.ndarray, class_cols,
              wrow: np.ndarray, mult: np.ndarray) -> tuple:
  """`engine.quantile_score_fold` in NumPy: the sums as
  `class_tables.host_fold` (classes, then rows, in increasing order from 0.0);
  the counts (per level below and tie, then valid and invalid) as
  `events.host_fold`."""
  del class_cols  # (the invalid points are counted, not completed)
  n_outer, n_row, n_class, n_level, _ = cnt.shape
  codes = np.concatenate(
      [cnt.reshape(n_outer, n_row, n_class, 2 * n_level), valid], axis=-1)
  return (class_tables.host_fold(sums, wrow, mult),
          events.host_fold(codes[None], wrow, mult)[0])


def normalize(table: np.ndarray, counts: np.ndarray, skipna: bool
              ) -> np.ndarray:
  """Region sums [..., L, 2] and weighted counts [..., 2 L + 2] (per level
  below, tie; valid, invalid) -> [..., 4, L]: each term over the valid mass."""
  n_level = table.shape[-2]
  mass = counts[..., 2 * n_level]
  flags = counts[..., :2 * n_level].reshape(counts.shape[:-1] + (n_level, 2))
  with np.errstate(all='ignore'):
    out = np.concatenate([table, flags], axis=-1) / mass[..., None, None]
  out = np.ascontiguousarray(np.swapaxes(out, -1, -2))
  dead = mass == 0.0
  if not skipna:
    dead = dead | (counts[..., 2 * n_level + 1] != 0.0)
  out[dead] = np.nan
  return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class QuantileScoreTable(class_tables.ClassSumsTable):
  """Per-level table of the pinball loss, the forecast quantile and the
  frequencies of the truth below / on it.

  `levels` is a strictly increasing sequence of 1 to 64 levels within [0, 1];
  `method` is 'linear', 'hazen' or 'weibull' (module docstring).  A forecast
  variable with `ensemble_dim` is an ensemble of 1 to 64 members, one without
  it a deterministic forecast, M = 1.  A variable with the dim `quantile_dim`
  holds quantile forecasts (at most 16) at the levels of that coordinate;
  `levels` must then be None or equal to it within 1e-12.

  Per common variable the result has dims (<outer dims in the order
  `crps_decomposition.CRPSTable` gives them>, 'term', 'level') -- with
  `regions=` a leading 'region' dim --, term = ('pinball',
  'forecast_quantile', 'below', 'tie'), level = the levels as float64.
  Attributes: `ensemble_size`, `method`, `levels` (a tuple of floats).

  `compute` is the time mean of the tables.
  """

  levels: t.Any = DEFAULT_LEVELS
  method: str = 'linear'
  ensemble_dim: t.Optional[str] = _m.REALIZATION
  quantile_dim: t.Optional[str] = None
  # one pass over the points answers every region; no windows of chunks
  _fused_regions = True
  _reads_slabs_in_place = False
  _terms = TERMS

  def __post_init__(self):
    checked_method(self.method)
    if self.levels is not None:
      checked_levels(self.levels)
    elif self.quantile_dim is None:
      raise ValueError(f'levels=None: the {_NOUN} takes its levels from '
                       'quantile_dim, which is None too')

  def _levels(self, forecast) -> np.ndarray:
    """The levels of a table of `forecast`: the coordinate of `quantile_dim`
    where the forecast has that dim (checked against `levels`), else
    `levels`."""
    dim = self.quantile_dim
    if dim is None or dim not in forecast.dims:
      if self.levels is None:
        raise ValueError(f'levels=None, and the forecast has no dim {dim!r}')
      return checked_levels(self.levels)
    try:
      coord = np.asarray(xl.coord_values(forecast, dim), dtype=np.float64)
    except (KeyError, TypeError, ValueError):
      raise ValueError(f'the dim {dim!r} needs a coordinate of levels'
                       ) from None
    tau = checked_levels(coord, direct=True)
    if self.levels is not None:
      given = checked_levels(self.levels)
      if given.shape != tau.shape or np.abs(given - tau).max() > LEVEL_TOL:
        raise ValueError(f'levels={tuple(given.tolist())} differ from the '
                         f'coordinate {dim!r}: {tuple(tau.tolist())}')
    return tau

  def _result_attrs(self, forecast):
    return {'ensemble_size': self._ensemble_size(forecast),
            'method': checked_method(self.method),
            'levels': tuple(self._levels(forecast).tolist())}

  def compute_chunk(self, forecast, truth, region=None, skipna=False,
                    regions: t.Optional[dict] = None):
    forecast, truth = _m._inputs(forecast, truth)
    names = list(_m._common_vars(forecast, truth))
    method = checked_method(self.method)
    tau = self._levels(forecast)
    dim = self.quantile_dim
    direct = [n for n in names if dim is not None and dim in forecast[n].dims]
    # every check of the variables before anything is launched
    sizes = set()
    for name in names:
      n_member = class_tables.check_variable(
          name, forecast[name], truth[name],
          dim if name in direct else self.ensemble_dim, f'the {_NOUN}',
          (MIN_MEMBERS, MAX_MEMBERS))
      engine.quantile_score_levels(tau, n_member, method, name in direct)
      if name not in direct:
        sizes.add(n_member)
    if len(sizes) > 1:
      raise ValueError(f'the variables differ in ensemble size: {sizes}')

    def values(is_direct):
      def one(name, device, args, class_cols, wrow, mult):
        tables = engine.quantile_score_levels(tau, args[2], method, is_direct)
        table, counts = class_tables.region_sums(
            device, args + (tables, is_direct), (host_sums, host_fold),
            (engine.quantile_score_sums, engine.quantile_score_fold),
            class_cols, wrow, mult)
        return normalize(table, counts, skipna)  # [outer, R, 4, L]
      return one
    trailing = lambda n_member: {TERM: np.array(TERMS, dtype=object),
                                 LEVEL: tau.copy()}
    parts = []
    for is_direct, group in ((True, direct),
                             (False, [n for n in names if n not in direct])):
      if not group and (is_direct or direct):
        continue
      # (the quantile dim is the member dim of a direct variable)
      metric = dataclasses.replace(self, ensemble_dim=dim) if is_direct else self
      parts.append(metric._tables(forecast, truth, group, region, regions,
                                  None, values(is_direct), trailing=trailing)[0])
    out = parts[0]
    if len(parts) > 1:
      coords = dict(parts[0].coords)
      coords.update(parts[1].coords)
      both = {name: da for part in parts for name, da in part.items()}
      out = xl.Dataset({name: both[name] for name in names}, coords)
    return out.assign_attrs(
        ensemble_size=sizes.pop() if sizes else self._ensemble_size(forecast),
        method=method, levels=tuple(tau.tolist()))


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last two dims of a table
# ---------------------------------------------------------------------------
def _per_table(fn):
  return events._per_table(fn, trailing=((TERM, len(TERMS)), (LEVEL, None)),
                           noun='a quantile score table')


def _table_levels(coords, n_level: int) -> np.ndarray:
  """The `level` coordinate of a table as float64 [n_level]."""
  if LEVEL not in coords:
    raise ValueError('the table has no level coordinate')
  c = coords[LEVEL]
  tau = np.asarray(c.values if isinstance(c, xl.DataArray) else c,
                   dtype=np.float64).reshape(-1)
  if tau.size != n_level:
    raise ValueError(f'the level coordinate holds {tau.size} levels, the '
                     f'table {n_level}')
  return tau


def _with_levels(fn):
  """`fn(p, dims, coords, tau, ...)`: `_per_table` drops the coordinates of the
  trailing dims, so the levels are taken from the table first."""
  inner = _per_table(fn)

  def wrapper(table, *args, **kwargs):
    if xl.is_xarray(table):
      tau = np.asarray(table.coords[LEVEL].values, dtype=np.float64)
    else:
      probe = table if isinstance(table, xl.DataArray) else next(
          iter(table.data_vars.values()))
      tau = _table_levels(dict(table.coords), probe.shape[-1])
    return inner(table, tau, *args, **kwargs)
  wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
  return wrapper


def _level_coords(tau, coords):
  return dict(coords, **{LEVEL: np.asarray(tau, dtype=np.float64)})


@_with_levels
def quantile_score(p, dims, coords, tau):
  """Per level: the mean pinball loss (the quantile score)."""
  return xl.DataArray(p[..., 0, :].copy(), dims + (LEVEL,),
                      _level_coords(tau, coords))


def observed_frequency(table, ties: str = 'half'):
  """Per level: below + c tie, the weighted frequency of the truth below the
  quantile, with c = 0 (`ties='below'`: y < q), 1/2 ('half') or 1 ('above': y
  <= q).  A calibrated forecast has it equal to `level`."""
  if ties not in TIES:
    raise ValueError(f'ties={ties!r}: one of {", ".join(map(repr, TIES))}')

  @_with_levels
  def frequency(p, dims, coords, tau):
    return xl.DataArray(p[..., 2, :] + TIES[ties] * p[..., 3, :],
                        dims + (LEVEL,), _level_coords(tau, coords))
  return frequency(table)


def _pairs(tau: np.ndarray) -> list:
  """[(lo index, hi index, level)] of the central intervals (tau, 1 - tau),
  tau < 1/2, whose two levels both occur (matched to 1e-12), widest last."""
  pairs = []
  for i, a in enumerate(tau.tolist()):
    if a < 0.5:
      hit = np.nonzero(np.abs(tau - (1.0 - a)) <= LEVEL_TOL)[0]
      if hit.size and hit[0] != i:
        pairs.append((i, int(hit[0]), a))
  if not pairs:
    raise ValueError('no pair of levels (tau, 1 - tau), tau < 1/2, among '
                     f'{tuple(tau.tolist())}')
  return sorted(pairs, key=lambda pr: 1.0 - 2.0 * pr[2])


def _interval(fn):
  @_with_levels
  def wrapper(p, dims, coords, tau):
    pairs = _pairs(tau)
    out = np.stack([fn(p, i, j, a) for i, j, a in pairs], axis=-1)
    nominal = np.array([1.0 - 2.0 * a for _, _, a in pairs], dtype=np.float64)
    return xl.DataArray(out, dims + (INTERVAL,),
                        dict(coords, **{INTERVAL: nominal}))
  wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
  return wrapper


@_interval
def interval_width(p, i, j, a):
  """Per central interval (tau, 1 - tau) whose levels both occur: the mean
  width forecast_quantile_hi - forecast_quantile_lo.  The new dim `interval`
  is the nominal coverage 1 - 2 tau, increasing.  No pair: ValueError."""
  return p[..., 1, j] - p[..., 1, i]


@_interval
def interval_coverage(p, i, j, a):
  """Per central interval: below_hi + tie_hi - below_lo, the weighted
  frequency of q_lo <= y <= q_hi (for monotone quantiles).  A calibrated
  forecast has it equal to `interval`."""
  return p[..., 2, j] + p[..., 3, j] - p[..., 2, i]


@_interval
def interval_score(p, i, j, a):
  """Per central interval: (pinball_lo + pinball_hi) / tau, Winkler's interval
  score: the mean of width + (2 / alpha) (distance of the truth outside), alpha
  = 2 tau.  Every 0/0 is NaN."""
  return (p[..., 0, i] + p[..., 0, j]) / a


def quantile_skill(table, reference_table):
  """Per level: 1 - pinball / pinball_ref, the skill of `table` against the
  table of a reference forecast on the same levels (1: perfect, 0: no better
  than the reference).  Differing levels are a ValueError; every 0/0 is
  NaN."""
  ours, ref = quantile_score(table), quantile_score(reference_table)

  def one(a, b):
    ta, tb = (np.asarray(v.coords[LEVEL], dtype=np.float64) for v in (a, b))
    if ta.shape != tb.shape or np.abs(ta - tb).max() > LEVEL_TOL:
      raise ValueError(f'the tables differ in levels: {tuple(ta.tolist())} '
                       f'and {tuple(tb.tolist())}')
    if a.shape != b.shape:
      raise ValueError(f'the tables differ in shape: {a.shape} and {b.shape}')
    with np.errstate(all='ignore'):
      return xl.DataArray(1.0 - a.values / b.values, a.dims, a.coords, a.name)
  if isinstance(ours, xl.DataArray) != isinstance(ref, xl.DataArray):
    raise ValueError('a table and its reference must both be DataArrays or '
                     'both Datasets')
  if isinstance(ours, xl.DataArray):
    return one(ours, ref)
  return xl.Dataset({name: one(ours[name], ref[name]) for name in ours},
                    ours.coords, getattr(ours, 'attrs', {}))


def crps_weights(tau) -> np.ndarray:
  """w_l of `crps_from_quantiles`: the width of level l's cell between the
  midpoints of adjacent levels, with 0 and 1 at the ends."""
  tau = np.asarray(tau, dtype=np.float64)
  mid = (tau[1:] + tau[:-1]) / 2.0
  edges = np.concatenate([[0.0], mid, [1.0]])
  return edges[1:] - edges[:-1]


@_with_levels
def crps_from_quantiles(p, dims, coords, tau):
  """2 sum_l w_l pinball_l, in increasing level order: the CRPS as the
  integral of the quantile score over the levels, by the midpoint rule (w_l =
  `crps_weights`).  With 'hazen' levels (i - 1/2) / M it is the CRPS of the
  ensemble's empirical CDF.  The `level` dim is removed."""
  w = crps_weights(tau)
  total = np.zeros(p.shape[:-2], dtype=np.float64)
  for l in range(p.shape[-1]):
    total = total + w[l] * p[..., 0, l]
  return xl.DataArray(2.0 * total, dims, coords)
