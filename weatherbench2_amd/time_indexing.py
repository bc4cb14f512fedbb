"""Time re-indexing: forecast-shaped datasets built by moving whole slabs along
time (scripts/expand_climatology.py, scripts/index_on_valid_time.py,
scripts/compute_probabilistic_climatological_forecasts.py).  No Beam, no zarr,
no flags, no pandas: what the scripts read from flags is a keyword argument
here, and year, day of year and hour come from datetime64 with NumPy.

  expand_climatology      climatology.sel(dayofyear=, hour=) for a run of valid
                          times: (hour, dayofyear, ...) -> (time, ...)
  index_on_valid_time     (init, lead) -> (valid time, lead) or (init, valid
                          time); combinations that do not exist are NaN and the
                          result is float32
  get_sampled_init_times  the sampler of the climatological ensemble, bit-equal
                          to the script's `_get_sampled_init_times`
  probabilistic_climatological_forecasts
                          the sampled ensemble itself: member r of (init time,
                          lead) is the truth at `sampled[r, init] + lead`

All three are one operation: a table over the new dims names, per output
position, the input position it is a copy of (-1: none).  With
`materialize=True` device-backed variables go through csrc/slab_scatter.hip
(K16): `plan_scatter` turns the table into a CSR over the distinct sources and
the kernel reads every source slab once, however many destinations it has.
Host variables take a NumPy path (take, fill, astype) with the same bits.  With
`materialize=False` nothing moves: every variable comes back as a `SlabGather`
over the input (its last two dims are the slab), which the metric kernels read
in place.  Inputs are never modified.

The slab of the kernel is everything behind the last re-indexed dim that input
and output share, so a variable is read where it lies: a contiguous tensor, a
view of whole slabs and a `SlabGather` over a resident base differ in the
table alone.  float32 and float64 go through the kernel; integers and bool
become the output's float type first where holes need NaN or the result is
float32, and are gathered by torch otherwise, like every other dtype.
"""
from __future__ import annotations

import math
import re
import typing as t

import numpy as np
import torch

from weatherbench2_amd import climatology as _climatology
from weatherbench2_amd import engine
from weatherbench2_amd import indexing
from weatherbench2_amd import operands
from weatherbench2_amd import resampling
from weatherbench2_amd import xarray_lite as xl

WRAP_YEAR = 'WRAP_YEAR'
NO_EDGE = 'NO_EDGE'
REFLECT_RANGE = 'REFLECT_RANGE'
EDGE_BEHAVIORS = (WRAP_YEAR, NO_EDGE, REFLECT_RANGE)

VALID_AND_DELTA = 'valid_and_delta'
VALID_AND_INIT = 'valid_and_init'

TIME = 'time'
DELTA = 'prediction_timedelta'
INIT = 'init'
REALIZATION = 'realization'
SOURCE_TIME = 'source_time'

# destinations of one CSR entry (see plan_scatter; profiles/NOTES.md has the
# launch with the holes under one entry: twice the time of the gather form)
MAX_DESTS_PER_ENTRY = 32

_HOUR_NS = 3600 * 10**9
_DAY_NS = 24 * _HOUR_NS


# ---------------------------------------------------------------------------
# the planner and the three paths of one variable
# ---------------------------------------------------------------------------
def plan_scatter(dest_to_src, n_in_slab: t.Optional[int] = None) -> tuple:
  """(src_slab, dst_begin, dst_slab) of K16 from a destination-to-source table
  (`dest_to_src[d]` = the input slab output slab d is a copy of, -1 = a hole):
  the distinct sources in ascending order, the holes first under -1, the
  destinations of a source ascending.  A source is one entry, so it is read
  once, unless it has more than `MAX_DESTS_PER_ENTRY` destinations: it then
  takes consecutive entries of that many (the workgroups of an entry store its
  destinations one after another, and one long list -- the holes of
  `index_on_valid_time` -- would outlast the rest of the launch).  This relies
  on what include/wb2hip.h allows of the tables: "an entry may repeat a
  source"; a cut source is read once per entry, and more than 32 holes are
  consecutive -1 entries, not one.  The cap was timed on the valid-time shape
  of tools/time_indexing_bench.py only (profiles/NOTES.md).  Every output slab
  is written exactly once (checked)."""
  table = np.ascontiguousarray(dest_to_src, dtype=np.int64).reshape(-1)
  if n_in_slab is None:
    n_in_slab = int(table.max(initial=-1)) + 1
  order = np.argsort(table, kind='stable')
  src, first = np.unique(table[order], return_index=True)
  begin = np.append(first, table.size).astype(np.int64)
  pieces = -(-np.diff(begin) // MAX_DESTS_PER_ENTRY)
  if pieces.size and pieces.max() > 1:
    piece = np.arange(pieces.sum()) - np.repeat(np.cumsum(pieces) - pieces,
                                                pieces)
    begin = np.append(np.repeat(begin[:-1], pieces)
                      + MAX_DESTS_PER_ENTRY * piece, table.size)
    src = np.repeat(src, pieces)
  return engine.scatter_csr(src, (begin, order.astype(np.int64)), n_in_slab,
                            table.size)


def _float_target(dtype: np.dtype, out_dtype, holes: bool):
  """The dtype a variable is brought to BEFORE it is re-indexed (None: as it
  is): integers and bool become the output's float type where the result is
  one, float64 where only the holes ask for NaN."""
  if dtype.kind == 'f':
    return None
  if out_dtype is not None:
    return np.dtype(out_dtype)
  return np.dtype(np.float64) if holes else None


def _host_reindex(values: np.ndarray, table: np.ndarray, n_point: int,
                  out_dtype) -> np.ndarray:
  """The scatter in NumPy: take, fill, astype.  [n_out_slab, n_point]."""
  idx = table.reshape(-1)
  holes = bool((idx < 0).any())
  target = _float_target(values.dtype, out_dtype, holes)
  if target is not None:
    values = values.astype(target)
  flat = np.ascontiguousarray(values).reshape(-1, n_point)
  if flat.shape[0] == 0:  # (nothing to take from: every slab is a hole)
    out = np.zeros((idx.size, n_point), dtype=flat.dtype)
  else:
    out = np.take(flat, np.maximum(idx, 0), axis=0)
  if holes:
    out[idx < 0] = np.nan
  with np.errstate(over='ignore'):  # (beyond float32's range: inf)
    return out if out_dtype is None else out.astype(out_dtype, copy=False)


def _torch_reindex(flat: torch.Tensor, table: np.ndarray, out_dtype):
  """The dtypes the kernel does not take: index_select, fill, cast."""
  idx = table.reshape(-1)
  out = torch.index_select(flat, 0, torch.as_tensor(np.maximum(idx, 0),
                                                    device=flat.device))
  if (idx < 0).any():
    out[torch.as_tensor(idx < 0, device=flat.device)] = float('nan')
  return out if out_dtype is None else out.to(operands.torch_dtype(out_dtype))


def _device_reindex(da: xl.DataArray, planned: dict, n_inner: int,
                    n_point: int, out_dtype) -> torch.Tensor:
  """[n_out_slab, n_point] on the device through K16.  `planned` holds the
  slab table and, once a variable has needed it, its CSR: variables that share
  both are planned and checked once."""
  table = planned['table']
  device = engine.require_gpu()
  np_dtype = operands.numpy_dtype(da.dtype)
  holes = bool((table < 0).any())
  target = _float_target(np_dtype, out_dtype, holes) or np_dtype
  dtype = operands.torch_dtype(target)
  out_torch = dtype if out_dtype is None else operands.torch_dtype(out_dtype)
  if (dtype, out_torch) not in engine.SCATTER_PAIRS:
    data = da.data
    if isinstance(data, xl.SlabGather):
      data = data.materialize(device)
    ten = engine.as_device_tensor(data, device)
    return _torch_reindex(ten.reshape(-1, n_point), table, out_dtype)
  ten, physical = operands.operand(da, da.dims, device, dtype, n_inner)
  if physical is not None:  # a view or a gather: where the slabs really lie
    src, begin, dst = plan_scatter(indexing.compose(table, physical))
  else:
    if 'csr' not in planned:
      planned['csr'] = plan_scatter(table)
    src, begin, dst = planned['csr']
  return engine.slab_scatter(ten, src, (begin, dst), table.size,
                             n_point=n_point, out_dtype=out_torch,
                             checked=True)


def _lazy_reindex(da: xl.DataArray, in_dims, sizes, out_dims,
                  re_: indexing.Reindex, out_dtype) -> xl.SlabGather:
  if indexing.common_tail(in_dims, out_dims, re_) < 2:
    raise ValueError(
        f'materialize=False needs the last two dims of {da.name!r} to be a '
        f'slab that is not re-indexed: its dims are {tuple(in_dims)}, '
        f'{re_.src_dims} are re-indexed')
  table = indexing.slab_table(in_dims, sizes, out_dims, re_, 2)
  data = da.data
  prior = None
  if isinstance(data, xl.SlabGather):
    data, prior = data.base, data.index.ravel()
  holes = bool((table < 0).any()) or (prior is not None
                                      and bool((prior < 0).any()))
  target = _float_target(operands.numpy_dtype(data.dtype), out_dtype, holes)
  if target is None and out_dtype is not None:
    target = np.dtype(out_dtype)
  if target is not None and operands.numpy_dtype(data.dtype) != target:
    # (one copy of the input, not of the output)
    with np.errstate(over='ignore'):  # (beyond float32's range: inf)
      data = (data.to(operands.torch_dtype(target))
              if isinstance(data, torch.Tensor) else data.astype(target))
  data = data.contiguous() if isinstance(data, torch.Tensor) \
      else np.ascontiguousarray(data)
  if prior is not None:  # a gather of a gather: compose the tables
    table = indexing.compose(table, prior)
  return xl.SlabGather(data, table)


def _reindex_variable(da: xl.DataArray, out_dims: tuple,
                      re_: indexing.Reindex, out_dtype, materialize: bool,
                      memo: dict):
  """The data of `da` re-indexed by `re_`, its dims then `out_dims`.  `memo`
  lives for one call of an entry point and one `re_`: the slab table (and its
  CSR) of variables with the same outer dims and slab depth is made once."""
  in_dims = da.dims
  sizes = dict(da.sizes)
  if isinstance(da.data, xl.SlabConcat):
    da = da.copy(da.data.materialize())
  new_sizes = dict(zip(re_.new_dims, re_.table.shape))
  out_shape = tuple(new_sizes[d] if d in new_sizes else sizes[d]
                    for d in out_dims)
  if not materialize:
    return _lazy_reindex(da, in_dims, sizes, out_dims, re_, out_dtype)
  k = indexing.common_tail(in_dims, out_dims, re_)
  if isinstance(da.data, xl.SlabGather):
    k = min(k, 2)  # (a gather's base is addressed slab by slab)
  n_point = math.prod(out_shape[len(out_shape) - k:])
  key = (tuple((d, sizes[d]) for d in in_dims[:len(in_dims) - k]),
         tuple(out_dims[:len(out_dims) - k]))
  if key not in memo:
    memo[key] = {'table': indexing.slab_table(in_dims, sizes, out_dims, re_,
                                              k)}
  table = memo[key]['table']
  if operands.on_device(da.data):
    if table.size * n_point == 0:
      dtype = operands.torch_dtype(
          out_dtype or _float_target(operands.numpy_dtype(da.dtype), None,
                                     False) or operands.numpy_dtype(da.dtype))
      return torch.zeros(out_shape, dtype=dtype, device=engine.require_gpu())
    return _device_reindex(da, memo[key], k, n_point,
                           out_dtype).reshape(out_shape)
  return _host_reindex(np.asarray(da.values), table, n_point,
                       out_dtype).reshape(out_shape)


def _ns(values, kind: str) -> np.ndarray:
  """int64 nanoseconds of a datetime64 ('M') or timedelta64 ('m') array."""
  a = np.asarray(values)
  if a.dtype.kind != kind:
    what = 'datetime64' if kind == 'M' else 'timedelta64'
    raise ValueError(f'expected {what} values, found {a.dtype}')
  return a.astype(f'{"datetime64" if kind == "M" else "timedelta64"}[ns]'
                  ).astype(np.int64)


def _datetimes(ns) -> np.ndarray:
  return np.asarray(ns, dtype=np.int64).astype('datetime64[ns]')


def _timedeltas(ns) -> np.ndarray:
  return np.asarray(ns, dtype=np.int64).astype('timedelta64[ns]')


def _timestamp_ns(value) -> int:
  """An ISO 8601 string, a datetime64 or a datetime as int nanoseconds."""
  return int(np.datetime64(value).astype('datetime64[ns]').astype(np.int64))


_UNIT_WORDS = {'weeks': 'w', 'week': 'w', 'days': 'd', 'day': 'd', 'D': 'd',
               'hours': 'h', 'hour': 'h', 'hr': 'h', 'H': 'h',
               'minutes': 'min', 'minute': 'min', 'T': 'min',
               'seconds': 's', 'second': 's', 'sec': 's', 'S': 's'}


def parse_duration(value) -> int:
  """Nanoseconds, as `resampling.parse_period` reads a period; the unit may
  also be spelled out ('15 days', '6 hours')."""
  if isinstance(value, str):
    m = re.fullmatch(r'\s*(\d+)\s*([A-Za-z]+)\s*', value)
    if m and m.group(2) in _UNIT_WORDS:
      value = m.group(1) + _UNIT_WORDS[m.group(2)]
  return resampling.parse_period(value)


def _rebuild(dataset: xl.Dataset, coords: dict, data: dict, dims: dict):
  out = xl.Dataset(coords=coords, attrs=dataset.attrs)
  for name, value in data.items():
    out.data_vars[name] = xl.DataArray(value, dims[name], out.coords, name)
  return out


# ---------------------------------------------------------------------------
# scripts/expand_climatology.py
# ---------------------------------------------------------------------------
def expand_climatology(climatology, times=None, *, time_start=None,
                       time_stop=None, materialize: bool = True):
  """The script's `select_climatology` over the time axis of its `main`:
  every variable of `climatology` (dims `dayofyear` and, where it is a
  coordinate, `hour`) at the day of year and hour of each time.  `times` is a
  datetime64 array; without it the axis runs from `time_start` to `time_stop`
  (both inclusive) in steps of `hour[1] - hour[0]` hours, 24 h without an
  `hour` coordinate.  The new `time` dim stands where the first of the two
  stood; `hour` and `dayofyear` are dropped.  A day of year or hour that the
  climatology lacks raises KeyError, as `.sel` does.  Variables with neither
  dim pass through."""
  if xl.is_xarray(climatology):
    return xl.like_input(expand_climatology(
        xl.from_xarray(climatology), times, time_start=time_start,
        time_stop=time_stop, materialize=materialize), climatology)
  dataset = xl.as_dataset(climatology)
  if 'dayofyear' not in dataset.coords:
    raise ValueError("the climatology has no 'dayofyear' coordinate")
  has_hour = 'hour' in dataset.coords
  doys = np.asarray(xl.coord_values(dataset, 'dayofyear')).astype(np.int64)
  hours = (np.asarray(xl.coord_values(dataset, 'hour')).astype(np.int64)
           if has_hour else None)
  if times is None:
    if time_start is None or time_stop is None:
      raise ValueError('either times or time_start and time_stop are needed')
    if has_hour:
      if hours.size < 2:
        raise ValueError('the hour coordinate needs two values to give the '
                         'spacing of the time axis')
      hour_delta = int(hours[1] - hours[0])
    else:
      hour_delta = 24
    if hour_delta <= 0:
      raise ValueError(f'hour[1] - hour[0] = {hour_delta} is not positive')
    start, stop = _timestamp_ns(time_start), _timestamp_ns(time_stop)
    times = _datetimes(np.arange(start, stop + 1, hour_delta * _HOUR_NS,
                                 dtype=np.int64))
  times = np.asarray(times).astype('datetime64[ns]')
  _, doy, hour, _ = _climatology.calendar(times)
  where = {'dayofyear': indexing.positions(doys, doy)}
  if has_hour:
    where['hour'] = indexing.positions(hours, hour)
  for dim, pos in where.items():
    if (pos < 0).any():
      labels = (doy if dim == 'dayofyear' else hour)[pos < 0]
      raise KeyError(f'not all values found in index {dim!r}: '
                     f'{np.unique(labels).tolist()}')
  coords = xl.coords_without(dataset.coords, tuple(where))
  coords = dict(coords, time=times)
  data, dims, memos = {}, {}, {}
  for name, da in dataset.data_vars.items():
    src = tuple(d for d in da.dims if d in where)
    if not src:
      data[name], dims[name] = da.data, da.dims
      continue
    table = np.ravel_multi_index([where[d] for d in src],
                                 [da.sizes[d] for d in src]) if times.size \
        else np.zeros(0, np.int64)
    re_ = indexing.Reindex(src, (TIME,), np.asarray(table, dtype=np.int64))
    dims[name] = indexing.in_place_dims(da.dims, src, (TIME,))
    data[name] = _reindex_variable(da, dims[name], re_, None, materialize,
                                   memos.setdefault(src, {}))
  return _rebuild(dataset, coords, data, dims)


# ---------------------------------------------------------------------------
# scripts/index_on_valid_time.py
# ---------------------------------------------------------------------------
def get_forecast_offset_and_spacing(init_times, lead_times) -> tuple:
  """The script's function of this name: (position of the first lead time
  kept, number of lead steps between two initialisations)."""
  init = _ns(init_times, 'M')
  lead = _ns(lead_times, 'm')
  init_deltas = np.unique(np.diff(init))
  if init_deltas.size != 1:
    raise ValueError('initialization times are not equidistant: '
                     f'{_timedeltas(init_deltas)}')
  lead_deltas = np.unique(np.diff(lead))
  if lead_deltas.size != 1:
    raise ValueError(f'lead times are not equidistant: '
                     f'{_timedeltas(lead_deltas)}')
  init_delta, lead_delta = int(init_deltas[0]), int(lead_deltas[0])
  spacing, remainder = divmod(init_delta, lead_delta)
  if remainder:
    raise ValueError(
        'initialization times not spaced at a multiple of lead times: '
        f'lead_delta={np.timedelta64(lead_delta, "ns")!r}, '
        f'init_delta={np.timedelta64(init_delta, "ns")!r}')
  if lead[0] == 0:
    offset = 0
  else:
    at = np.flatnonzero(lead == spacing * lead_delta)
    if not at.size:
      raise ValueError(f'{np.timedelta64(spacing * lead_delta, "ns")!r} is '
                       'not in the lead times')
    offset = int(at[0])
  return offset, int(spacing)


def index_on_valid_time(forecast, desired_time_dims: str = VALID_AND_DELTA, *,
                        materialize: bool = True):
  """The script's pipeline: `forecast` (dims `time` = initialisation time and
  `prediction_timedelta`) indexed on valid time.  'valid_and_delta' gives
  (time, prediction_timedelta) with the lead times [offset::spacing] of
  `get_forecast_offset_and_spacing`, 'valid_and_init' gives (init, time) with
  every lead time; `time` is then the sorted valid times, each new dim stands
  where the one it replaces stood.  Combinations without a forecast are NaN
  and every variable is float32."""
  if xl.is_xarray(forecast):
    return xl.like_input(index_on_valid_time(
        xl.from_xarray(forecast), desired_time_dims, materialize=materialize),
                         forecast)
  if desired_time_dims not in (VALID_AND_DELTA, VALID_AND_INIT):
    raise ValueError(f'Unhandled desired_time_dims={desired_time_dims!r}')
  dataset = xl.as_dataset(forecast)
  for dim in (TIME, DELTA):
    if dim not in dataset.coords:
      raise ValueError(f'the forecast has no {dim!r} coordinate')
  init = _ns(xl.coord_values(dataset, TIME), 'M')
  lead = _ns(xl.coord_values(dataset, DELTA), 'm')
  offset, spacing = get_forecast_offset_and_spacing(_datetimes(init),
                                                    _timedeltas(lead))
  if desired_time_dims == VALID_AND_DELTA:
    kept = np.arange(offset, lead.size, spacing)
    valid = np.unique(init[:, None] + lead[kept][None, :])
    # (valid time, lead) comes from the init time valid - lead
    at = indexing.positions(init, valid[:, None] - lead[kept][None, :])
    table = np.where(at < 0, -1, at * lead.size + kept[None, :])
    new_dims, rename = (TIME, DELTA), {TIME: TIME, DELTA: DELTA}
    new_coords = {TIME: _datetimes(valid), DELTA: _timedeltas(lead[kept])}
  else:
    valid = np.unique(init[:, None] + lead[None, :])
    # (init, valid time) comes from the lead valid - init
    at = indexing.positions(lead, valid[None, :] - init[:, None])
    table = np.where(at < 0, -1,
                     np.arange(init.size, dtype=np.int64)[:, None] * lead.size
                     + at)
    new_dims, rename = (INIT, TIME), {TIME: INIT, DELTA: TIME}
    new_coords = {INIT: _datetimes(init), TIME: _datetimes(valid)}
  re_ = indexing.Reindex((TIME, DELTA), new_dims, table.astype(np.int64))
  coords = xl.coords_without(dataset.coords, (TIME, DELTA))
  coords.update(new_coords)
  data, dims, memo = {}, {}, {}
  for name, da in dataset.data_vars.items():
    if TIME not in da.dims or DELTA not in da.dims:
      raise ValueError(f'{name!r} needs the dims {TIME!r} and {DELTA!r}: '
                       f'{da.dims}')
    dims[name] = tuple(rename.get(d, d) for d in da.dims)
    data[name] = _reindex_variable(da, dims[name], re_, np.float32,
                                   materialize, memo)
  return _rebuild(dataset, coords, data, dims)


# ---------------------------------------------------------------------------
# scripts/compute_probabilistic_climatological_forecasts.py
# ---------------------------------------------------------------------------
def _window(day_window_size: int) -> tuple:
  """(first, last) day offset of a window of that many days: centred for an
  odd size, one more day before than after for an even one."""
  if not 1 <= day_window_size <= 2 * 364:
    raise ValueError(f'day_window_size must lie in [1, 728]: {day_window_size}')
  first = -(day_window_size // 2)
  return first, first + day_window_size - 1


def get_ensemble_size(ensemble_size: int, climatology_start_year: int,
                      climatology_end_year: int, day_window_size: int,
                      leave_out_if_in_climatology: bool) -> int:
  """The number of members: `ensemble_size` itself, or, for -1, one member
  per (climatology year, day offset of the window) pair."""
  if ensemble_size > 0:
    return int(ensemble_size)
  if ensemble_size != -1:
    raise ValueError('ensemble_size must be positive, or -1 for every (year, '
                     f'day offset) pair: {ensemble_size}')
  if leave_out_if_in_climatology:
    raise ValueError('ensemble_size=-1 has no meaning with '
                     'leave_out_if_in_climatology: the years to draw from '
                     'change with the initial time')
  first, last = _window(day_window_size)
  return (max(climatology_end_year - climatology_start_year + 1, 0)
          * (last - first + 1))


def _days_in_year(year: np.ndarray) -> np.ndarray:
  leap = (year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0))
  return 365 + leap.astype(np.int64)


def get_sampled_init_times(output_times, climatology_start_year: int,
                           climatology_end_year: int, day_window_size: int,
                           ensemble_size: int, with_replacement: bool,
                           sample_hold_days: int,
                           initial_time_edge_behavior: str,
                           leave_out_if_in_climatology: bool,
                           num_years_to_exclude: int, seed: int) -> np.ndarray:
  """datetime64[ns] [n_member, len(output_times)]: entry [r, j] is the time of
  the truth that stands for member r of the forecast initialised at
  output_times[j]: a year drawn from the climatology years, the day of year
  of output_times[j] moved by a day offset drawn from the window, the hour of
  output_times[j].  Bit-equal to `_get_sampled_init_times` of the script for
  the same arguments: the draws from `np.random.default_rng(seed)` are the
  same, in the same order (see the four cases below).

  `with_replacement`: year and offset are independent uniform draws; without,
  the members of one initial time are distinct (year, offset) pairs.
  `leave_out_if_in_climatology` removes the year of the initial time and the
  `num_years_to_exclude` after it from the years of that time.  A day of year
  that leaves its year wraps inside it (WRAP_YEAR), runs on into the
  neighbouring year (NO_EDGE) or does so except at the first and last
  climatology year, where it is reflected (REFLECT_RANGE).  With
  `sample_hold_days` = h, the initial times of each run of h days share the
  shift in days of one of them.  Every misuse is a ValueError."""
  output_times = np.asarray(output_times).astype('datetime64[ns]')
  out_year, out_doy, out_hour, out_day = _climatology.calendar(output_times)
  if initial_time_edge_behavior not in EDGE_BEHAVIORS:
    raise ValueError('initial_time_edge_behavior must be one of '
                     f'{EDGE_BEHAVIORS}: {initial_time_edge_behavior!r}')
  low, high = _window(day_window_size)
  n_offset = high - low + 1
  pool = np.arange(climatology_start_year, climatology_end_year + 1)
  n_member = get_ensemble_size(ensemble_size, climatology_start_year,
                               climatology_end_year, day_window_size,
                               leave_out_if_in_climatology)
  n_time = len(output_times)
  if not pool.size:
    raise ValueError(f'no climatology years: {climatology_start_year} .. '
                     f'{climatology_end_year}')
  shape = (n_member, n_time)
  rng = np.random.default_rng(seed)

  def years_left(j):
    kept = pool[(pool < out_year[j])
                | (pool > out_year[j] + num_years_to_exclude)]
    if kept.size < (1 if with_replacement else n_member):
      raise ValueError(
          f'{kept.size} climatology years are left for the initial time '
          f'{output_times[j]} after leaving out {out_year[j]} .. '
          f'{out_year[j] + num_years_to_exclude}: {n_member} members '
          f'{"with" if with_replacement else "without"} replacement need more')
    return kept

  # the four cases, each with the generator calls the script makes
  if with_replacement and not leave_out_if_in_climatology:
    # offsets, then years: one call each for the whole sample
    shift = rng.integers(low, high + 1, size=shape)
    year = rng.integers(pool[0], pool[-1] + 1, size=shape)
  elif with_replacement:
    # offsets for the whole sample, then the years of one time after another
    shift = rng.integers(low, high + 1, size=shape)
    year = np.stack([rng.choice(years_left(j), size=n_member, replace=True)
                     for j in range(n_time)], axis=1) if n_time else \
        np.zeros(shape, dtype=np.int64)
  elif leave_out_if_in_climatology:
    # per time: its distinct years, then a draw of offsets for the WHOLE
    # sample, of which only the last time's is used
    if not n_time:
      raise ValueError('no output times to sample for')
    columns = []
    for j in range(n_time):
      columns.append(rng.choice(years_left(j), size=n_member, replace=False))
      shift = rng.integers(low, high + 1, size=shape)
    year = np.stack(columns, axis=1)
  else:
    # per time a random order of the (year, offset) grid, year-major: the
    # argsort of one uniform draw from a generator of its own on the seed;
    # the first n_member pairs of that order are the members
    n_pair = pool.size * n_offset
    if n_member > n_pair:
      raise ValueError(f'{n_member} members without replacement, but only '
                       f'{n_pair} (year, day offset) pairs')
    order = np.random.default_rng(seed).random((n_pair, n_time)).argsort(
        axis=0)[:n_member]
    year, shift = pool[order // n_offset], low + order % n_offset

  doy = out_doy[None, :] + shift
  length = _days_in_year(year)
  if initial_time_edge_behavior == WRAP_YEAR:
    doy = (doy - 1) % length + 1
  elif initial_time_edge_behavior == REFLECT_RANGE:
    doy = np.where((year == pool[0]) & (doy < 1), 2 - doy, doy)
    if pool[-1] != pool[0]:
      doy = np.where((year == pool[-1]) & (doy > length), 2 * length - doy,
                     doy)
  # whole days from here on: the sample's day number and its shift
  new_year = (year - 1970).astype('datetime64[Y]').astype('datetime64[D]')
  moved = new_year.astype(np.int64) + doy - 1 - out_day[None, :]
  if sample_hold_days:
    steps = np.unique(np.diff(output_times.astype(np.int64)))
    if steps.size != 1:
      raise ValueError('a sample hold needs equally spaced output times: the '
                       f'steps are {_timedeltas(steps)}')
    per_hold, rest = divmod(int(sample_hold_days) * _DAY_NS, int(steps[0]))
    if rest or per_hold < 1:
      raise ValueError(f'sample_hold_days={sample_hold_days} is not a '
                       f'multiple of the step {_timedeltas(steps)[0]!r} of the '
                       'output times')
    # run b of per_hold times takes the shift of time b
    moved = moved[:, np.arange(n_time) // per_hold]
  return _datetimes((out_day[None, :] + moved) * _DAY_NS
                    + out_hour[None, :] * _HOUR_NS)


def _check_spacings(times_ns: np.ndarray, lead_step: int, init_step: int,
                    time_dim: str) -> None:
  """What the ensemble asks of the three spacings (all in nanoseconds): the
  truth is equally spaced; lead step and initial-time step are whole hours,
  multiples of the truth's step, one a multiple of the other, and each a
  multiple or a divisor of a day (so that a forecast meets the same times of
  day at every initial time)."""
  truth_steps = np.unique(np.diff(times_ns))
  if truth_steps.size != 1:
    raise ValueError(f'the truth is not equally spaced along {time_dim!r}: its '
                     f'steps are {_timedeltas(truth_steps)}')
  truth_step = int(truth_steps[0])
  show = lambda ns: repr(np.timedelta64(ns, 'ns'))  # noqa: E731
  if lead_step % init_step and init_step % lead_step:
    raise ValueError(f'timedelta_spacing {show(lead_step)} and '
                     f'initial_time_spacing {show(init_step)}: one must be a '
                     'multiple of the other')
  for name, step in (('timedelta_spacing', lead_step),
                     ('initial_time_spacing', init_step)):
    if step % truth_step:
      raise ValueError(f'{name} {show(step)} is not a multiple of the '
                       f"truth's step {show(truth_step)}")
    if step % _DAY_NS and _DAY_NS % step:
      raise ValueError(f'{name} {show(step)} is neither a multiple nor a '
                       'divisor of one day')
    if step % _HOUR_NS:
      raise ValueError(f'{name} {show(step)} is not a whole number of hours')


def probabilistic_climatological_forecasts(
    truth, *, initial_time_start, initial_time_end,
    initial_time_spacing='6h', forecast_duration='15 days',
    timedelta_spacing='6h', climatology_start_year: int = 1990,
    climatology_end_year: int = 2020, day_window_size: int = 15,
    ensemble_size: int = 2, with_replacement: bool = True,
    sample_hold_days: int = 0, initial_time_edge_behavior: str = WRAP_YEAR,
    leave_out_if_in_climatology: bool = False, num_years_to_exclude: int = 0,
    seed: int = 802701, add_source_time: bool = False, time_dim: str = TIME,
    realization_name: str = REALIZATION, materialize: bool = True):
  """The script's `main`: an ensemble forecast for the initial times
  `initial_time_start` .. `initial_time_end` (inclusive, every
  `initial_time_spacing`) and the lead times 0 .. `forecast_duration` (every
  `timedelta_spacing`) whose member r at (init t, lead d) is `truth` at
  `get_sampled_init_times(...)[r, t] + d`.  The variables have the dims
  (`realization_name`, 'prediction_timedelta', `time_dim`, ...the others of
  the input in their order), as the script's template has; with
  `add_source_time`, `source_time` over the first three holds the times the
  samples were taken from.  A time the truth lacks is an error that names it.
  Variables without `time_dim` are dropped."""
  if xl.is_xarray(truth):
    kwargs = dict(locals())
    kwargs.pop('truth')
    return xl.like_input(probabilistic_climatological_forecasts(
        xl.from_xarray(truth), **kwargs), truth)
  dataset = xl.as_dataset(truth)
  if time_dim not in dataset.coords:
    raise ValueError(f'the truth has no {time_dim!r} coordinate')
  if DELTA in dataset.dims:
    raise ValueError(f'the truth already has a {DELTA!r} dim')
  times = _ns(xl.coord_values(dataset, time_dim), 'M')
  init_spacing = parse_duration(initial_time_spacing)
  delta_spacing = parse_duration(timedelta_spacing)
  duration = parse_duration(forecast_duration)
  _check_spacings(times, delta_spacing, init_spacing, time_dim)
  n_member = get_ensemble_size(ensemble_size, climatology_start_year,
                               climatology_end_year, day_window_size,
                               leave_out_if_in_climatology)
  inits = _datetimes(np.arange(_timestamp_ns(initial_time_start),
                               _timestamp_ns(initial_time_end) + 1,
                               init_spacing, dtype=np.int64))
  deltas = np.arange(0, duration + 1, delta_spacing, dtype=np.int64)
  sampled = get_sampled_init_times(
      inits, climatology_start_year, climatology_end_year, day_window_size,
      n_member, with_replacement, sample_hold_days,
      initial_time_edge_behavior, leave_out_if_in_climatology,
      num_years_to_exclude, seed)
  # [realization, lead, init]: the time of the truth each slab is a copy of
  source = (sampled.astype(np.int64)[:, None, :] + deltas[None, :, None])
  table = indexing.positions(times, source)
  if (table < 0).any():
    missing = _datetimes(np.unique(source[table < 0]))
    hint = ''
    if initial_time_edge_behavior == WRAP_YEAR and sample_hold_days:
      hint = (' (a sample hold with WRAP_YEAR can reach up to a year outside '
              'the climatology years)')
    raise ValueError(
        f'the truth lacks {missing.size} of the times the samples are taken '
        f'from{hint}: {missing[:8]}{" ..." if missing.size > 8 else ""}')
  new_dims = (realization_name, DELTA, time_dim)
  re_ = indexing.Reindex((time_dim,), new_dims, table)
  coords = xl.coords_without(dataset.coords, (time_dim,))
  coords.update({realization_name: np.arange(n_member), DELTA: _timedeltas(deltas),
                 time_dim: inits})
  data, dims, memo = {}, {}, {}
  for name, da in dataset.data_vars.items():
    if time_dim not in da.dims:
      continue
    dims[name] = new_dims + tuple(d for d in da.dims if d != time_dim)
    data[name] = _reindex_variable(da, dims[name], re_, None, materialize,
                                   memo)
  if add_source_time:
    data[SOURCE_TIME], dims[SOURCE_TIME] = _datetimes(source), new_dims
  return _rebuild(dataset, coords, data, dims)
