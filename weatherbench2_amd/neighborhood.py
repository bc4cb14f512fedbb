"""Neighbourhood verification: the fractions skill score (FSS).

Point-wise event scores (`events.EventTable`) punish a high-resolution
forecast twice for a small displacement: one miss and one false alarm.  The
fractions skill score of Roberts & Lean (2008) compares, instead, the FRACTION
of event points in a neighbourhood of every point.  The reference has no
counterpart.  `FractionsTable` computes the sufficient statistics, the score
functions below are host arithmetic on them.

One slab is (latitude, longitude) with n_row x n_col points, one threshold
field `thr` (`Threshold.compute(truth)`), M >= 1 members (a deterministic
forecast is M = 1) and an odd window n = 2 h + 1 in GRID POINTS, the same count
at every latitude.

Per point, exactly the definitions of `events`:

  k     the number of members with x > thr, 0..M
  o     1 if truth > thr else 0
  IEEE comparisons: a NaN threshold exceeds nothing, equality is not
  exceedance, +-inf are ordinary values.  A point is INVALID iff the truth or
  any member is NaN.

An invalid point is a non-event in both fields (k = o = 0), STAYS in the
window count and is left out as a window centre.  "Missing counts as below the
threshold in both fields" is this project's choice: it keeps every denominator
constant along a row.

The window of centre (i, j) is the rows max(0, i - h) .. min(n_row - 1, i + h)
(clipped at the poles) and the columns (j - h .. j + h) mod n_col (longitude is
cyclic), N_i = n * (rows of the clipped range) points.  With

  F = sum_window k  (0 .. M N_i),     O = M * sum_window o,

the neighbourhood fractions are P_f = F / (M N_i) -- for an ensemble the
neighbourhood ensemble probability -- and P_o = O / (M N_i).  Everything up to
here is integer: per (row i, column class c) the six int64 sums over the valid
centres j of the class

  q0 = sum (F - O)^2   q1 = sum F^2   q2 = sum O^2
  q3 = sum F           q4 = sum O     q5 = the number of valid centres

are taken by K19 (csrc/neighborhood.hip: `engine.event_codes`, `engine.
fss_sums`) for device-backed variables and by NumPy (`host_codes`,
`host_sums`) for host ones.  The regions are those of `events.column_classes`
(col_class, mult[r][c], wrow[r][i]).  With D_i = float(M N_i) the host forms
the row weights in float64

  g2 = wrow[r][i] / (D_i * D_i)   (the product first, then ONE division)
  g1 = wrow[r][i] / D_i
  g0 = wrow[r][i]

and the fold (`engine.fss_fold`, `host_fold`) is

  T[r][q] = sum_i g(q)[r][i] * float(sum_c mult[r][c] * sum[i][c][q])

with the inner sum in int64, the rows in increasing order (acc = acc + g * s
from 0.0, no fused multiply-add), g(q) = g2 for q = 0, 1, 2, g1 for q = 3, 4
and g0 for q = 5.  Both paths produce the same integers and fold in the same
order: they agree bit for bit.

Components of a cell (threshold, window, outer index, region):

  fbs                = T0 / T5         the fractions Brier score
  fbs_reference      = (T1 + T2) / T5  its no-overlap worst case
  forecast_fraction  = T3 / T5
  observed_fraction  = T4 / T5

T5 == 0 gives NaN.  skipna=False: ONE invalid point anywhere in the slab makes
the slab's components NaN for EVERY region -- windows cross region borders, a
per-region rule would be inconsistent.  (The slab's number of valid centres
comes from the same fold: a pseudo-region with wrow = 1, mult = 1.)
skipna=True: the rules above.

Scores are host arithmetic on a table and non-linear: fss = 1 - fbs /
fbs_reference, fss_uniform = 0.5 + observed_fraction / 2, useful_scale = the
smallest window with fss >= fss_uniform.  `FractionsTable.compute` is the time
mean of the COMPONENTS; scores are taken from the mean table and never
averaged themselves.

Limits (ValueError before any launch): windows odd, 1..255, at most n_col, no
duplicates; a cyclic longitude axis (uniform spacing d with n_col d = 360);
1..128 members; at most 64 column classes; no region with a 2-D field;
(M n^2)^2 n_col max(mult) < 2^63.  A (longitude, latitude) variable costs one
transposing device copy, as in `events`.
"""
from __future__ import annotations

import dataclasses
import numbers
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import metrics as _m
from weatherbench2_amd import thresholds as thresholds_lib
from weatherbench2_amd import xarray_lite as xl

MAX_WINDOW = 255  # (members and classes: events.MAX_MEMBERS, MAX_CLASSES)
N_SUMS = 6
NEIGHBORHOOD, COMPONENT = 'neighborhood', 'component'
COMPONENTS = ('fbs', 'fbs_reference', 'forecast_fraction',
              'observed_fraction')
CODE_OBSERVED, CODE_INVALID = 0x100, 0x200


# ---------------------------------------------------------------------------
# the host path: same integers, same fold order
# ---------------------------------------------------------------------------
def host_codes(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
               truth: np.ndarray, truth_slab, thresholds, thr_slabs,
               n_outer: int, n_row: int, n_col: int) -> np.ndarray:
  """`engine.event_codes` in NumPy: the same arguments (contiguous host arrays
  instead of tensors), the same uint16 [n_threshold, n_outer, n_row, n_col]."""
  out = np.zeros((len(thresholds), n_outer, n_row, n_col), dtype=np.uint16)
  for ti, o, k, obs, bad in events.host_exceedance(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, thresholds,
      thr_slabs, n_outer, n_row * n_col):
    code = np.where(bad, CODE_INVALID, k | obs * CODE_OBSERVED)
    out[ti, o] = code.reshape(n_row, n_col)
  return out


def _box(field: np.ndarray, h: int) -> np.ndarray:
  """int64 [..., n_row, n_col] -> its window sums: rows clipped, columns
  cyclic."""
  n_row, n_col = field.shape[-2:]
  zero = np.zeros(field.shape[:-2] + (1, n_col), dtype=np.int64)
  down = np.concatenate([zero, np.cumsum(field, axis=-2)], axis=-2)
  rows = np.arange(n_row)
  vert = (down[..., np.minimum(rows + h, n_row - 1) + 1, :] -
          down[..., np.maximum(rows - h, 0), :])
  out = np.zeros_like(vert)
  for d in range(-h, h + 1):
    out += np.roll(vert, d, axis=-1)
  return out


def host_sums(code: np.ndarray, windows, n_member: int, col_class,
              n_class: int) -> np.ndarray:
  """`engine.fss_sums` in NumPy: int64 [n_cell, n_window, n_row, n_class, 6]
  of a uint16 code plane [..., n_row, n_col]."""
  n_row, n_col = code.shape[-2:]
  code = code.reshape((-1, n_row, n_col)).astype(np.int64)
  k = code & 0xff
  obs = (code >> 8) & 1
  valid = 1 - ((code >> 9) & 1)
  onehot = (np.asarray(col_class, dtype=np.int64)[:, None] ==
            np.arange(n_class)[None, :]).astype(np.int64)
  out = np.zeros((code.shape[0], len(windows), n_row, n_class, N_SUMS),
                 dtype=np.int64)
  for wi, n in enumerate(windows):
    h = int(n) // 2
    f = _box(k, h)
    o = _box(obs, h) * int(n_member)
    terms = ((f - o) ** 2, f * f, o * o, f, o, np.ones_like(f))
    for q, term in enumerate(terms):
      out[:, wi, :, :, q] = (term * valid) @ onehot
  return out


def window_weights(wrow: np.ndarray, n_member: int, windows) -> np.ndarray:
  """float64 [n_window, 3, n_region, n_row]: g2, g1, g0 of the module
  docstring for every window."""
  wrow = np.asarray(wrow, dtype=np.float64)
  n_row = wrow.shape[1]
  rows = np.arange(n_row)
  out = np.empty((len(windows), 3) + wrow.shape, dtype=np.float64)
  for wi, n in enumerate(windows):
    h = int(n) // 2
    n_rows = np.minimum(rows + h, n_row - 1) - np.maximum(rows - h, 0) + 1
    d = (int(n_member) * int(n) * n_rows).astype(np.float64)
    out[wi, 0] = wrow / (d * d)[None, :]
    out[wi, 1] = wrow / d[None, :]
    out[wi, 2] = wrow
  return out


def host_fold(sums: np.ndarray, w: np.ndarray, mult: np.ndarray) -> np.ndarray:
  """`engine.fss_fold` in NumPy: the inner sum over the classes in int64, then
  acc = acc + w[window, g(q), r, i] * float(s) over the rows in increasing
  order: float64 [n_cell, n_window, n_region, 6]."""
  s = np.einsum('rc,nwicq->nwirq', mult.astype(np.int64),
                sums.astype(np.int64))
  group = np.array([0, 0, 0, 1, 1, 2])
  g = np.moveaxis(w[:, group], 1, -1)  # [window, region, row, q]
  acc = np.zeros(s.shape[:2] + s.shape[3:], dtype=np.float64)
  for i in range(sums.shape[2]):
    acc = acc + g[None, :, :, i, :] * s[:, :, i].astype(np.float64)
  return acc


def components(table: np.ndarray, n_point: int, skipna: bool) -> np.ndarray:
  """[..., n_region + 1, 6] fold results, the pseudo-region (wrow = 1, mult =
  1) last -> [..., n_region, 4] components."""
  real, slab_valid = table[..., :-1, :], table[..., -1:, 5]
  with np.errstate(all='ignore'):
    t5 = real[..., 5]
    out = np.stack([real[..., 0] / t5, (real[..., 1] + real[..., 2]) / t5,
                    real[..., 3] / t5, real[..., 4] / t5], axis=-1)
  dead = t5 == 0.0
  if not skipna:
    dead = dead | (slab_valid != float(n_point))
  out[dead] = np.nan
  return out


# ---------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------
def _check_windows(neighborhoods, n_col: int) -> tuple:
  windows = []
  for n in neighborhoods:
    if not isinstance(n, numbers.Integral) or isinstance(n, bool):
      raise ValueError(f'window {n!r}: a window is an odd number of grid '
                       'points')
    n = int(n)
    if n < 1 or n > MAX_WINDOW or n % 2 == 0 or n > n_col:
      raise ValueError(
          f'window {n}: a window is odd, 1 to {MAX_WINDOW} and at most the '
          f'{n_col} longitudes')
    windows.append(n)
  if not windows:
    raise ValueError('FractionsTable needs at least one window')
  if len(set(windows)) != len(windows):
    raise ValueError(f'duplicate windows: {windows}')
  return tuple(windows)


def _check_cyclic(lon: np.ndarray) -> None:
  lon = np.asarray(lon, dtype=np.float64)
  if lon.size < 2:
    return
  step = np.diff(lon)
  d = step[0]
  if not (np.all(np.abs(step - d) <= 1e-6 * abs(d)) and
          abs(lon.size * abs(d) - 360.0) <= 1e-6 * 360.0):
    raise ValueError(
        'the longitude axis is not cyclic (uniform spacing d with n_col * d = '
        '360): on a regional axis the window count would depend on the '
        'column')


def _check_range(n_member: int, windows, n_col: int, mult) -> None:
  top = int(np.max(mult)) if np.size(mult) else 1
  worst = (n_member * max(windows) ** 2) ** 2 * n_col * max(top, 1)
  if worst >= 2 ** 63:
    raise ValueError(
        f'{n_member} members, window {max(windows)}, {n_col} longitudes and '
        f'column multiplicity {top}: the int64 sums could overflow')


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
def _region_tables(ops, n_row: int, n_col: int, windows, col_class, mult,
                   wrow) -> np.ndarray:
  """float64 [n_threshold * n_outer, n_window, n_region, 6] on the host,
  through K19 for device operands and through NumPy for host ones."""
  front = ops.front(n_row, n_col)
  w = window_weights(wrow, ops.n_member, windows)
  n_class = mult.shape[1]
  if ops.device is None:
    sums = host_sums(host_codes(*front), windows, ops.n_member, col_class,
                     n_class)
    return host_fold(sums, w, mult)
  sums = engine.fss_sums(engine.event_codes(*front), windows, ops.n_member,
                         col_class, n_class)
  table = engine.fss_fold(sums, w, mult)
  engine.order_read(table)
  return table.cpu().numpy()


@dataclasses.dataclass
class FractionsTable(events.ExceedanceTable):
  """Neighbourhood fractions of a forecast against thresholds, the sufficient
  statistics of the fractions skill score.

  Per common variable the result has dims ('quantile', 'neighborhood', <outer
  dims in xarray's order>, 'component') -- with `regions=` a leading 'region'
  dim --: `neighborhood` holds the window sizes in grid points, `component`
  the names fbs, fbs_reference, forecast_fraction, observed_fraction (module
  docstring).  A forecast variable without `ensemble_dim` (or ensemble_dim=
  None) is a deterministic forecast: M = 1.  Attributes: `threshold_method`,
  `ensemble_size`.

  `compute` is the time mean of the components.  Scores are non-linear in the
  table, so they are taken FROM the mean table (`fss(metric.compute(...))`)
  and never averaged themselves.
  """

  neighborhoods: t.Sequence[int] = (1, 3, 5, 9, 17)
  ensemble_dim: t.Optional[str] = _m.REALIZATION
  _noun = 'fractions table'
  _lead_dims = (NEIGHBORHOOD,)
  _trailing_dims = (COMPONENT,)

  def _setup(self, lat, lon, mult, wrow):
    windows = _check_windows(self.neighborhoods, len(lon))
    _check_cyclic(lon)
    # the pseudo-region: its q5 is the slab's number of valid centres
    mult = np.concatenate([mult, np.ones((1, mult.shape[1]), np.int32)])
    wrow = np.concatenate([wrow, np.ones((1, len(lat)), np.float64)])
    return mult, wrow, windows

  def _values(self, ops, n_row, n_col, col_class, mult, wrow, skipna,
              windows):
    _check_range(ops.n_member, windows, n_col, mult)
    table = _region_tables(ops, n_row, n_col, windows, col_class, mult, wrow)
    c = components(table, n_row * n_col, skipna)  # [T * outer, W, R, 4]
    c = c.reshape((len(self.thresholds), ops.n_outer) + c.shape[1:])
    return np.moveaxis(c, 2, 1)  # [T, W, outer, R, 4]

  def _extra_coords(self, n_member, windows):
    return {NEIGHBORHOOD: np.array(windows, dtype=np.int64),
            COMPONENT: np.array(COMPONENTS, dtype=object)}


# ---------------------------------------------------------------------------
# absolute thresholds
# ---------------------------------------------------------------------------
@dataclasses.dataclass(init=False)
class ConstantThreshold(thresholds_lib.Threshold):
  """An absolute threshold (1 mm, 10 mm, 25 m/s): `value` is a number or a
  {variable: number} mapping.  `compute(truth)` gives one (latitude,
  longitude) field per variable of `truth`, in its dtype and where the truth
  lies; the kernels read it through a slab table that names slab 0 for every
  outer index.  `quantile` labels the `quantile` dim of a threshold metric's
  result: the value itself unless one is given (a mapping needs one)."""

  value: t.Any = None

  def __init__(self, value, quantile: t.Optional[float] = None):
    if quantile is None:
      if isinstance(value, t.Mapping):
        raise ValueError('a {variable: number} threshold needs a `quantile` '
                         'to label the result with')
      quantile = float(value)
    super().__init__(climatology=None, quantile=float(quantile))
    self.value = value

  def compute(self, truth) -> xl.Dataset:
    given = truth
    truth = xl.as_dataset(truth)
    lat = xl.coord_values(truth, 'latitude')
    lon = xl.coord_values(truth, 'longitude')
    coords = {'latitude': lat, 'longitude': lon}
    out = xl.Dataset(coords=coords)
    for name in truth.keys():
      name = str(name)
      if isinstance(self.value, t.Mapping):
        if name not in self.value:
          raise KeyError(f'no threshold value for variable {name!r}')
        value = float(self.value[name])
      else:
        value = float(self.value)
      data = truth[name].data  # (not .values: that would download it)
      shape = (len(lat), len(lon))
      dtype = events._dtype_of(data)
      if not dtype.is_floating_point:
        dtype = torch.float64
      if events._on_device(data):
        # where the truth is: the tensor's own device (a lazy container's
        # first base)
        base = (data.bases[0] if isinstance(data, xl.SlabConcat) else
                data.base if isinstance(data, xl.SlabGather) else data)
        field = torch.full(shape, value, dtype=dtype, device=base.device)
      else:
        field = np.full(shape, value,
                        dtype=torch.empty(0, dtype=dtype).numpy().dtype)
      out.data_vars[name] = xl.DataArray(field, ('latitude', 'longitude'),
                                         coords, name)
    return xl.like_input(out, given)


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last dim of a table
# ---------------------------------------------------------------------------
def _per_table(fn):
  """`events._per_table` for a fractions table: `fn(c, lead dims, coords)`."""
  return events._per_table(fn, ((COMPONENT, len(COMPONENTS)),),
                           'a fractions table')


def _fss(c):
  return 1.0 - c[..., 0] / c[..., 1]


def _fss_uniform(c):
  return 0.5 + c[..., 3] / 2.0


@_per_table
def fss(c, dims, coords):
  """1 - fbs / fbs_reference: 1 for a perfect forecast, 0 for no overlap; 0/0
  (no event in either field) is NaN."""
  return xl.DataArray(_fss(c), dims, coords)


@_per_table
def fss_uniform(c, dims, coords):
  """0.5 + observed_fraction / 2: the score above which a window is usually
  called useful (Roberts & Lean 2008)."""
  return xl.DataArray(_fss_uniform(c), dims, coords)


@_per_table
def useful_scale(c, dims, coords):
  """The smallest window (grid points, as float64) with fss >= fss_uniform
  along `neighborhood`; NaN where no window reaches it."""
  if NEIGHBORHOOD not in dims or NEIGHBORHOOD not in coords:
    raise ValueError(f'no {NEIGHBORHOOD!r} dim: dims {dims}')
  axis = dims.index(NEIGHBORHOOD)
  windows = np.asarray(coords[NEIGHBORHOOD], dtype=np.float64)
  shape = [1] * len(dims)
  shape[axis] = windows.size
  reached = _fss(c) >= _fss_uniform(c)  # (NaN compares false)
  scale = np.where(reached, windows.reshape(shape), np.inf).min(axis=axis)
  scale = np.where(np.isfinite(scale), scale, np.nan)
  rest = tuple(d for d in dims if d != NEIGHBORHOOD)
  return xl.DataArray(scale, rest,
                      {k: v for k, v in coords.items() if k != NEIGHBORHOOD})
