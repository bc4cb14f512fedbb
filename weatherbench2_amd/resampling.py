"""Resampling in time (scripts/resample_in_time.py:202-309 and the parts of
its `main` that change values or names): binned (`resample`) and rolling mean,
min, max and sum along a time axis.  No Beam, no zarr, no flags: what the
script reads from flags is a keyword argument here.

`resample_in_time_core` is the script's function of that name for one
statistic; `resample_in_time` is `resample_in_time_chunk` for a whole dataset
with the variable selection, the names and the rolling label shift of `main`.
All statistics asked of one variable come from ONE kernel launch and one read
of the variable.

Device-backed variables (torch tensors on the GPU, `SlabGather` /
`SlabConcat`) go through csrc/time_window.hip and give device tensors; host
variables take a NumPy path with the same bits (it sums in time order, where
NumPy's own `sum` along a contiguous axis goes pairwise).  Inputs are never
modified.  Where the time dim has a dim after it the variable is read in place
(a contiguous tensor as it is; a time-sliced view, a permuted time order and a
`SlabGather` over a resident base through a slab table); where it is the
innermost dim, one transposing device copy is made.  The result keeps the
input's dim order, its dtype and its other coordinates.

The bins of `method='resample'` are those of pandas' `Series.resample(period,
label=..., closed=...)` with the default origin ('start_day'), which is what
xarray groups by:
  * label_side='left': bins [T, T + period) labelled T; the first edge is
    t0 - ((t0 - midnight(t0)) % period);
  * label_side='right': bins (T - period, T] labelled T; with off = (t0 -
    midnight(t0)) % period the first edge is t0 - off if off > 0, else t0 -
    period; the first bin is dropped, as the script's isel(slice(1, None)) does.
For a timedelta axis (prediction_timedelta) midnight(t0) is t0 itself, and
pandas' right-closed binner adds one empty bin after a last time that lies on
an edge; it is kept (NaN), as everything here follows pandas' grouping.
`method='rolling'` keeps the time axis: output t is over the w = period //
delta_t steps that end at t, NaN where that window is incomplete or holds a
NaN, for both values of `skipna` (xarray's min_periods=None).

Differences from xarray:
  * integer and bool data become float64 first, for every statistic (xarray
    keeps integers for min, max and sum);
  * an empty bin (a gap in the time axis) gives NaN in every statistic, `sum`
    included.  This is this build's reading of xarray's restored empty groups;
    no reference test pins it, and pandas gives 0 for `sum` there.
"""
from __future__ import annotations

import datetime
import re
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

ALL = 'ALL'
STATISTICS = ('mean', 'min', 'max', 'sum')  # the order of the outputs
_SUFFIX = {'min': '_min', 'max': '_max', 'sum': '_sum'}
_UNIT_NS = {'w': 7 * 86400 * 10**9, 'd': 86400 * 10**9, 'h': 3600 * 10**9,
            'min': 60 * 10**9, 's': 10**9}
_DAY_NS = 86400 * 10**9
# bins a workgroup handles one after another: overlapping windows share their
# terms through its cache lines; short disjoint bins share a launch slot
_ROLLING_BINS_PER_GROUP = 32
_SHORT_BIN_STEPS = 32


def parse_period(period) -> int:
  """`period` in nanoseconds: a `np.timedelta64`, a `datetime.timedelta` or a
  string `<int><unit>` with unit w, d, h, min or s."""
  if isinstance(period, np.timedelta64):
    if np.isnat(period):
      raise ValueError('period is NaT')
    try:
      ns = int(period.astype('timedelta64[ns]').astype(np.int64))
    except (TypeError, ValueError) as e:
      raise ValueError(f'cannot express {period!r} in nanoseconds') from e
  elif isinstance(period, datetime.timedelta):
    ns = ((period.days * 86400 + period.seconds) * 10**6
          + period.microseconds) * 1000
  elif isinstance(period, str):
    m = re.fullmatch(r'\s*(\d+)\s*(w|d|h|min|s)\s*', period)
    if not m:
      raise ValueError(
          f'period {period!r} is not <int><unit> with unit w, d, h, min or s')
    ns = int(m.group(1)) * _UNIT_NS[m.group(2)]
  else:
    raise ValueError(f'period must be a timedelta or a string, not {period!r}')
  if ns <= 0:
    raise ValueError(f'period must be positive: {period!r}')
  return ns


def _time_ns(times) -> tuple:
  """(int64 nanoseconds, 'M' or 'm') of a datetime64 / timedelta64 axis."""
  times = np.asarray(times)
  if times.ndim != 1 or times.dtype.kind not in 'Mm':
    raise ValueError('the time coordinate must be a 1-D datetime64 or '
                     f'timedelta64 array, not {times.dtype} {times.shape}')
  if np.isnat(times).any():
    raise ValueError('the time coordinate holds NaT')
  kind = times.dtype.kind
  ns = times.astype(f'{"datetime64" if kind == "M" else "timedelta64"}[ns]')
  ns = ns.astype(np.int64)
  if ns.size > 1 and not np.all(np.diff(ns) > 0):
    raise ValueError('the time coordinate must increase')
  return ns, kind


def _labels(ns: np.ndarray, kind: str) -> np.ndarray:
  return np.asarray(ns, dtype=np.int64).astype(
      'datetime64[ns]' if kind == 'M' else 'timedelta64[ns]')


def plan_resample(times, period, label_side: str = 'left') -> tuple:
  """(labels, int32 [n_bin, 2] ranges [begin, end) into `times`) of
  `Series.resample(period, label=label_side, closed=label_side)`, the first
  bin dropped for label_side='right'."""
  if label_side not in ('left', 'right'):
    raise ValueError(f'Unhandled label_side={label_side!r}')
  ns, kind = _time_ns(times)
  period = parse_period(period)
  if ns.size == 0:
    raise ValueError('cannot resample an empty time axis')
  t0, t_last = int(ns[0]), int(ns[-1])
  off = ((t0 % _DAY_NS) if kind == 'M' else 0) % period
  if label_side == 'left':
    first = t0 - off
    n_bin = (t_last - first) // period + 1
    edges = first + period * np.arange(n_bin + 1, dtype=np.int64)
    at = np.searchsorted(ns, edges, side='left')
    labels, drop = edges[:-1], 0
  else:
    first = t0 - off if off > 0 else t0 - period
    n_bin = -((first - t_last) // period)  # ceil((t_last - first) / period)
    if kind == 'm' and (t_last - first) % period == 0:
      n_bin += 1  # (pandas' timedelta binner always runs one period on)
    edges = first + period * np.arange(n_bin + 1, dtype=np.int64)
    at = np.searchsorted(ns, edges, side='right')
    labels, drop = edges[1:], 1
  ranges = np.stack([at[:-1], at[1:]], axis=1).astype(np.int32)
  return _labels(labels[drop:], kind), np.ascontiguousarray(ranges[drop:])


def rolling_window(times, period) -> int:
  """w = period // delta_t, delta_t from the first two times."""
  ns, _ = _time_ns(times)
  period = parse_period(period)
  if ns.size < 2:
    raise ValueError('rolling needs at least two times to find delta_t')
  delta_t = int(ns[1] - ns[0])
  if period % delta_t:
    raise ValueError(
        f'delta_t={np.timedelta64(delta_t, "ns")!r} between chunk times did '
        f'not evenly divide period={np.timedelta64(period, "ns")!r}')
  return period // delta_t


def plan_rolling(n_time: int, w: int) -> np.ndarray:
  """int32 [n_time, 2]: output t is over [t - w + 1, t + 1); a negative begin
  marks an incomplete window."""
  end = np.arange(1, n_time + 1, dtype=np.int64)
  begin = np.maximum(end - w, -1)  # (any negative begin says the same)
  return np.ascontiguousarray(np.stack([begin, end], axis=1).astype(np.int32))


# ---------------------------------------------------------------------------
# the two paths: {statistic: array with the time axis replaced by the bins}
# ---------------------------------------------------------------------------
def _host_stats(data: np.ndarray, axis: int, ranges: np.ndarray,
                statistics: t.Sequence[str], skipna: bool) -> dict:
  """The kernel's arithmetic in NumPy: a sequential loop over the time steps
  of each bin, in the data's own float type."""
  data = np.asarray(data)
  if data.dtype not in (np.float32, np.float64):
    data = data.astype(np.float64)
  dtype = data.dtype
  x = np.moveaxis(data, axis, 0)
  n_time = x.shape[0]
  shape = (len(ranges),) + x.shape[1:]
  out = {s: np.full(shape, np.nan, dtype=dtype) for s in statistics}
  with np.errstate(all='ignore'):
    for b, (begin, end) in enumerate(np.asarray(ranges).tolist()):
      if begin < 0 or begin >= end or end > n_time:
        continue
      total = None
      low = np.full(x.shape[1:], np.inf, dtype=dtype)
      high = np.full(x.shape[1:], -np.inf, dtype=dtype)
      count = np.zeros(x.shape[1:], dtype=np.int64)
      for step in range(begin, end):
        v = x[step]
        isnan = np.isnan(v)
        term = np.where(isnan, dtype.type(0), v) if skipna else v
        total = term.copy() if total is None else total + term
        count += ~isnan
        low = np.where(v < low, v, low)
        high = np.where(v > high, v, high)
      n = count if skipna else np.full_like(count, end - begin)
      none = count == 0 if skipna else count < end - begin
      if 'sum' in out:
        out['sum'][b] = total
      if 'mean' in out:
        out['mean'][b] = np.where(n == 0, np.nan, total / n.astype(dtype))
      if 'min' in out:
        out['min'][b] = np.where(none, np.nan, low)
      if 'max' in out:
        out['max'][b] = np.where(none, np.nan, high)
  return {s: np.moveaxis(a, 0, axis) for s, a in out.items()}


def _device_stats(da: xl.DataArray, axis: int, ranges: np.ndarray,
                  statistics: t.Sequence[str], skipna: bool,
                  bins_per_group: int) -> dict:
  lay = operands.SeriesLayout.of(da.dims, da.sizes, da.dims[axis])
  n_outer, n_time, n_point = lay.n_outer, lay.n_series, lay.n_point
  n_bin = len(ranges)
  device = engine.require_gpu()
  dtype = operands.float_dtype(da.dtype)
  if n_outer * n_time * n_point * n_bin == 0:
    outs = {s: torch.full((n_outer, n_bin, n_point), float('nan'), dtype=dtype,
                          device=device) for s in statistics}
  else:
    ten, table = lay.operand(da, device, dtype)
    bins = torch.from_numpy(np.ascontiguousarray(ranges, dtype=np.int32)).to(
        device, non_blocking=True)
    outs = engine.time_bin_stats(ten, table, n_outer, n_time, n_point, bins,
                                 list(statistics), skipna, bins_per_group)
  return {s: lay.restore(a, (n_bin,)) for s, a in outs.items()}


def _bins_per_group(method: str, ranges: np.ndarray) -> int:
  if method == 'rolling':
    return _ROLLING_BINS_PER_GROUP
  longest = int(np.max(ranges[:, 1] - ranges[:, 0], initial=1))
  return max(1, min(8, _SHORT_BIN_STEPS // max(longest, 1)))


def _variable_stats(da: xl.DataArray, time_dim: str, ranges: np.ndarray,
                    statistics: t.Sequence[str], skipna: bool,
                    method: str) -> dict:
  """{statistic: data} of one variable, all from one pass over it."""
  axis = da.dims.index(time_dim)
  # xarray's rolling with min_periods=None: a NaN empties the window whatever
  # skipna says
  skipna = bool(skipna) and method != 'rolling'
  if operands.on_device(da.data):
    return _device_stats(da, axis, ranges, statistics, skipna,
                         _bins_per_group(method, ranges))
  return _host_stats(da.values, axis, ranges, statistics, skipna)


def _plan(times, method: str, period, label_side: str) -> tuple:
  """(time labels of the result, ranges) for the script's core call."""
  if method == 'rolling':
    w = rolling_window(times, period)
    ns, kind = _time_ns(times)
    return _labels(ns, kind), plan_rolling(len(ns), w)
  if method == 'resample':
    return plan_resample(times, period, label_side)
  raise ValueError(f'Unhandled method={method!r}')


def _time_values(obj, time_dim: str) -> np.ndarray:
  if time_dim not in obj.coords:
    raise ValueError(f'{time_dim!r} has no coordinate to resample by')
  return xl.coord_values(obj, time_dim)


def _new_coords(coords: dict, time_dim: str, labels: np.ndarray) -> dict:
  """The non-time coordinates as they are, the time labels replaced where
  they stood; coordinates that lie along the time dim other than its own are
  dropped."""
  kept = xl.coords_without(coords, (time_dim,))
  return {k: labels if k == time_dim else c for k, c in coords.items()
          if k == time_dim or k in kept}


def _check_statistic(statistic: str) -> None:
  if statistic not in STATISTICS:
    raise ValueError(f'Unhandled statistic={statistic!r}')


def resample_in_time_core(chunk, method: str, period, statistic: str,
                          skipna: bool, *, time_dim: str = 'time',
                          label_side: str = 'left'):
  """The script's `resample_in_time_core` (:270-309) for a `Dataset` or a
  `DataArray`: `statistic` ('mean', 'min', 'max' or 'sum') of every variable
  over the bins of `method` ('resample' or 'rolling') and `period`.  Variables
  without `time_dim` pass through unchanged.  See the module docstring."""
  if xl.is_xarray(chunk):
    if hasattr(chunk, 'data_vars'):
      return xl.like_input(resample_in_time_core(
          xl.from_xarray(chunk), method, period, statistic, skipna,
          time_dim=time_dim, label_side=label_side), chunk)
    name = chunk.name if chunk.name is not None else '_resample_input'
    lite = xl.from_xarray(chunk.to_dataset(name=name))
    return xl.like_input(resample_in_time_core(
        lite[name], method, period, statistic, skipna, time_dim=time_dim,
        label_side=label_side), chunk)
  if method not in ('resample', 'rolling'):
    raise ValueError(f'Unhandled method={method!r}')
  if label_side not in ('left', 'right'):
    raise ValueError(f'Unhandled label_side={label_side!r}')
  _check_statistic(statistic)
  if isinstance(chunk, xl.DataArray):
    if time_dim not in chunk.dims:
      raise ValueError(f'{time_dim!r} missing from {chunk.dims}')
    labels, ranges = _plan(_time_values(chunk, time_dim), method, period,
                           label_side)
    data = _variable_stats(chunk, time_dim, ranges, [statistic], skipna,
                           method)[statistic]
    return xl.DataArray(data, chunk.dims,
                        _new_coords(chunk.coords, time_dim, labels), chunk.name)
  dataset = xl.as_dataset(chunk)
  labels, ranges = _plan(_time_values(dataset, time_dim), method, period,
                         label_side)
  out = xl.Dataset(coords=_new_coords(dataset.coords, time_dim, labels),
                   attrs=dataset.attrs)
  for name, da in dataset.data_vars.items():
    if time_dim in da.dims:
      data = _variable_stats(da, time_dim, ranges, [statistic], skipna,
                             method)[statistic]
    else:
      data = da.data
    out.data_vars[name] = xl.DataArray(data, da.dims, out.coords, name)
  return out


def _get_vars(list_of_vars, time_dependent_vars: list) -> list:
  """The script's `_get_vars` (:187-199)."""
  if isinstance(list_of_vars, str):
    list_of_vars = [list_of_vars]
  list_of_vars = list(list_of_vars or [])
  if not list_of_vars:
    return []
  if len(list_of_vars) == 1 and list_of_vars[0] == ALL:
    return list(time_dependent_vars)
  if ALL in list_of_vars:
    raise ValueError(
        f'Cannot specify both {ALL} and other variables. Found {list_of_vars}')
  return list_of_vars


def resample_in_time(chunk, *, method: str, period, mean_vars=(), min_vars=(),
                     max_vars=(), sum_vars=(), add_mean_suffix: bool = False,
                     skipna: bool = False, time_dim: str = 'time',
                     label_side: str = 'left'):
  """The script's `resample_in_time_chunk` with the parts of `main` that
  change values or names.  `*_vars` are lists of variable names, or ['ALL']
  for every variable with `time_dim`; variables in no list are dropped.  Per
  input variable the outputs come in the order mean (named `<var>_mean` only
  with `add_mean_suffix`), `<var>_min`, `<var>_max`, `<var>_sum`.  For
  `method='rolling'` the spacing of the time axis must be constant and the
  labels are shifted as `main` does: by `- period + delta_t` for
  label_side='left' (the result at T is over [T, T + period)), by `+ delta_t`
  for 'right'."""
  if xl.is_xarray(chunk):
    return xl.like_input(resample_in_time(
        xl.from_xarray(chunk), method=method, period=period,
        mean_vars=mean_vars, min_vars=min_vars, max_vars=max_vars,
        sum_vars=sum_vars, add_mean_suffix=add_mean_suffix, skipna=skipna,
        time_dim=time_dim, label_side=label_side), chunk)
  dataset = xl.as_dataset(chunk)
  if method not in ('resample', 'rolling'):
    raise ValueError(f'Unhandled method={method!r}')
  if label_side not in ('left', 'right'):
    raise ValueError(f'Unhandled label_side={label_side!r}')
  time_vars = [k for k, v in dataset.data_vars.items() if time_dim in v.dims]
  nontime_vars = set(dataset.data_vars) - set(time_vars)
  asked = {'mean': _get_vars(mean_vars, time_vars),
           'min': _get_vars(min_vars, time_vars),
           'max': _get_vars(max_vars, time_vars),
           'sum': _get_vars(sum_vars, time_vars)}
  keep = set().union(*asked.values())
  if keep & nontime_vars:
    raise ValueError('Statistics asked for on some variables that did not '
                     f'contain {time_dim}: {keep & nontime_vars}')
  missing = keep - set(dataset.data_vars)
  if missing:
    raise ValueError(f'Statistics asked for on variables that are not in the '
                     f'chunk: {sorted(missing)}')
  times = _time_values(dataset, time_dim)
  period_ns = parse_period(period)
  labels, ranges = _plan(times, method, period, label_side)
  if method == 'rolling':
    ns, kind = _time_ns(times)
    deltas = np.unique(np.diff(ns))
    if len(deltas) != 1:
      raise ValueError('Input data must have constant spacing. Found '
                       f'{deltas.astype("timedelta64[ns]")}')
    delta_t = int(deltas[0])
    shift = delta_t - period_ns if label_side == 'left' else delta_t
    labels = _labels(ns + shift, kind)
  kept_dims = set()
  for name in keep:
    kept_dims.update(dataset.data_vars[name].dims)
  coords = {k: c for k, c in _new_coords(dataset.coords, time_dim,
                                         labels).items()
            if (set(c.dims) <= kept_dims if isinstance(c, xl.DataArray)
                else k in kept_dims or k not in dataset.dims)}
  out = xl.Dataset(coords=coords, attrs=dataset.attrs)
  for name, da in dataset.data_vars.items():
    mine = [s for s in STATISTICS if name in asked[s]]
    if not mine:
      continue
    stats = _variable_stats(da, time_dim, ranges, mine, skipna, method)
    for s in mine:
      new = (f'{name}_mean' if add_mean_suffix else name) if s == 'mean' \
          else f'{name}{_SUFFIX[s]}'
      out.data_vars[new] = xl.DataArray(stats[s], da.dims, out.coords, new)
  return out
