"""Host-side indexing shared by every module that selects by label or moves
whole slabs: NumPy only.

  calendar       year, day of year, hour and day number of datetime64 values
  positions      where labels stand in an index (-1: absent); `sel_positions`
                 raises KeyError instead, as `.sel` does
  slice_positions, list_positions
                 the positions of `.sel(dim=slice(...))` and `.sel(dim=[...])`,
                 as pandas' `Index.slice_indexer` gives them: inclusive
                 bounds, decreasing axes, partial date strings
  slab_table     the table of a vectorised selection: per output position over
                 the new dims, the input slab it is a copy of (-1: a hole),
                 described by a `Reindex`; `in_place_dims` orders the result's
                 dims by xarray's rule, `common_tail` counts the dims behind
                 the selection, `compose` reads through an earlier gather
"""
from __future__ import annotations

import re
import typing as t

import numpy as np

from weatherbench2_amd import xarray_lite as xl


def calendar(times) -> tuple:
  """(year, day of year 1..366, hour of day, day number since 1970-01-01) of
  datetime64 values of any unit and shape, each int64 with that shape; equal
  to .year / .dayofyear / .hour of a pandas index, in NumPy (building such an
  index per chunk cost 0.13 ms).  Anything else goes through
  `astype('datetime64[ns]')` first: datetime objects, Timestamps, ISO strings;
  integers are nanoseconds since 1970, as pandas reads them.  NaT is a
  ValueError."""
  times = np.asarray(times)
  if times.dtype.kind != 'M':
    times = times.astype('datetime64[ns]')
  if np.isnat(times).any():
    raise ValueError('the time coordinate holds NaT')
  day = times.astype('datetime64[D]')
  year_start = times.astype('datetime64[Y]')
  year = year_start.astype(np.int64) + 1970
  doy = (day - year_start.astype('datetime64[D]')).astype(np.int64) + 1
  hour = times.astype('datetime64[h]').astype(np.int64) % 24
  return year, doy, hour, day.astype(np.int64)


_LABEL_LUTS: dict = {}  # id(label array) -> (array, lookup table or None)


def _lookup_table(have: np.ndarray) -> t.Optional[np.ndarray]:
  """The dense table label -> position of an index of distinct small
  non-negative integers (dayofyear 1..366, hour 0..23), remembered per label
  array OBJECT: the per-chunk cost of a climatology gather is two tiny fancy
  indexings instead of two argsorts."""
  hit = _LABEL_LUTS.get(id(have))
  if hit is None or hit[0] is not have:
    lut = None
    if have.min() >= 0 and have.max() < 4096 and (
        len(np.unique(have)) == have.size):
      lut = np.full(int(have.max()) + 2, -1, dtype=np.int64)
      lut[have] = np.arange(have.size, dtype=np.int64)
    if len(_LABEL_LUTS) >= 64:
      _LABEL_LUTS.clear()
    hit = _LABEL_LUTS[id(have)] = (have, lut)
  return hit[1]


def positions(have, want) -> np.ndarray:
  """int64, shaped like `want`: the position in the index `have` of every
  label of `want`, -1 where it is absent.  datetime64 and timedelta64 of any
  unit compare as instants (int64 nanoseconds), as pandas indexes do.  Numbers
  and times go through a stable argsort and a binary search, any other kind
  through a dict over `xl.label_list`.  Of a label that `have` holds more than
  once the FIRST position is returned (pandas raises on such an index)."""
  have, want = np.asarray(have), np.asarray(want)
  kinds = have.dtype.kind + want.dtype.kind
  if kinds in ('MM', 'mm'):
    unit = 'datetime64[ns]' if kinds == 'MM' else 'timedelta64[ns]'
    have = have.astype(unit).astype(np.int64)
    want = want.astype(unit).astype(np.int64)
  elif kinds[0] not in 'iuf' or kinds[1] not in 'iuf':
    first: dict = {}
    for i, v in enumerate(xl.label_list(have)):
      first.setdefault(v, i)
    return np.array([first.get(v, -1) for v in xl.label_list(want)],
                    dtype=np.int64).reshape(want.shape)
  if not have.size:
    return np.full(want.shape, -1, dtype=np.int64)
  if kinds in ('ii', 'iu', 'ui', 'uu') and have.size <= 4096:
    lut = _lookup_table(have)
    if lut is not None:
      return lut[np.clip(want.astype(np.int64, copy=False), -1, lut.size - 1)]
  order = np.argsort(have, kind='stable')
  at = order[np.minimum(np.searchsorted(have, want, sorter=order),
                        have.size - 1)]
  return np.where(have[at] == want, at, -1).astype(np.int64)


def sel_positions(have, want, absent: str) -> np.ndarray:
  """`positions` for a caller that needs every label, as `.sel` does: a
  KeyError with the text `absent`, formatted with the first absent label as
  `label`."""
  pos = positions(have, want)
  if (pos < 0).any():
    raise KeyError(absent.format(label=np.asarray(want)[pos < 0][0]))
  return pos


_NS = {'ns': 1, 'us': 10**3, 'ms': 10**6, 's': 10**9, 'min': 60 * 10**9,
       'h': 3600 * 10**9, 'D': 86400 * 10**9, 'W': 7 * 86400 * 10**9}
_DURATION_UNITS = {
    'w': 'W', 'week': 'W', 'weeks': 'W', 'd': 'D', 'day': 'D', 'days': 'D',
    'h': 'h', 'hr': 'h', 'hour': 'h', 'hours': 'h', 'm': 'min', 'min': 'min',
    'minute': 'min', 'minutes': 'min', 't': 'min', 's': 's', 'sec': 's',
    'second': 's', 'seconds': 's', 'ms': 'ms', 'millisecond': 'ms',
    'milliseconds': 'ms', 'us': 'us', 'microsecond': 'us',
    'microseconds': 'us', 'ns': 'ns', 'nanosecond': 'ns', 'nanoseconds': 'ns'}
_DATETIME_STRING = re.compile(
    r'\s*(\d{4})(?:-(\d{2})(?:-(\d{2})(?:[T ](\d{2})(?::(\d{2})(?::(\d{2})'
    r'(?:\.(\d{1,9}))?)?)?)?)?)?\s*')


def _datetime_string_bounds(label: str) -> tuple:
  """(first, last) instant in int64 ns of the period an ISO 8601 string
  names, at the resolution it is written in: pandas' partial-string rule
  ('2020' is the year, '2020-03-01T06' that hour)."""
  m = _DATETIME_STRING.fullmatch(label)
  if not m:
    raise KeyError(f'cannot read {label!r} as a date: write it as '
                   'YYYY[-MM[-DD[THH[:MM[:SS[.f]]]]]]')
  n_given = sum(g is not None for g in m.groups())
  unit = ('Y', 'M', 'D', 'h', 'm', 's')[min(n_given, 6) - 1]
  if n_given == 7:
    unit = ('ms', 'us', 'ns')[(len(m.group(7)) - 1) // 3]
  first = np.datetime64(label.strip().replace(' ', 'T'), unit)
  as_ns = lambda v: int(v.astype('datetime64[ns]').astype(np.int64))
  return as_ns(first), as_ns(first + 1) - 1


def _duration_string_bounds(label: str) -> tuple:
  """(first, last) in int64 ns of a '<number> <unit>' string on a timedelta
  axis.  pandas widens to the resolution of the VALUE, the smallest unit of
  days / h / min / s / ms / us / ns it needs: '15 days' is that whole day, '6h'
  that whole hour, and '24h', which is one day, the whole day too."""
  m = re.fullmatch(r'\s*(-?\d+(?:\.\d+)?)\s*([A-Za-z]+)\s*', label)
  unit = m and _DURATION_UNITS.get(m.group(2).lower())
  if not unit:
    raise KeyError(f'cannot read {label!r} as a duration: write it as '
                   '"<number> <unit>", for example "15 days" or "6h"')
  number = m.group(1)
  ns = (int(number) * _NS[unit] if '.' not in number
        else int(round(float(number) * _NS[unit])))
  for res in ('ns', 'us', 'ms', 's', 'min', 'h'):
    coarser = {'ns': 'us', 'us': 'ms', 'ms': 's', 's': 'min', 'min': 'h',
               'h': 'D'}[res]
    if ns % _NS[coarser] // _NS[res]:
      return ns, ns + _NS[res] - 1
  return ns, ns + _NS['D'] - 1


def _axis_values(labels) -> tuple:
  """(values, kind): datetime64 / timedelta64 axes as int64 ns with kind 'M'
  / 'm', every other axis as it is with its dtype's kind."""
  a = np.asarray(labels)
  if a.dtype.kind == 'M':
    return a.astype('datetime64[ns]').astype(np.int64), 'M'
  if a.dtype.kind == 'm':
    return a.astype('timedelta64[ns]').astype(np.int64), 'm'
  return a, a.dtype.kind


def _bound(label, kind: str, side: int):
  """A slice bound (`side` 0: start, 1: stop) as a value of the axis: on a
  datetime or timedelta axis the int64 ns of a datetime64 / timedelta64 or of
  that end of a string's period."""
  if kind not in 'Mm':
    if isinstance(label, str) and kind in 'iuf':
      raise TypeError(f'a string bound {label!r} on a numeric axis: give it '
                      'through sel, not sel_strings')
    return label
  if isinstance(label, str):
    return (_datetime_string_bounds if kind == 'M'
            else _duration_string_bounds)(label)[side]
  v = np.asarray(label)
  if v.dtype.kind != kind:
    what = 'datetime' if kind == 'M' else 'timedelta'
    raise TypeError(
        f'the bound {label!r} on a {what} axis: give a {what}64 or a string '
        '(sel_strings / drop_sel_strings make every value a string)')
  unit = 'datetime64[ns]' if kind == 'M' else 'timedelta64[ns]'
  return int(v.astype(unit).astype(np.int64))


def _monotonic(a: np.ndarray) -> int:
  """1: non-decreasing (pandas' is_monotonic_increasing), -1: non-increasing,
  0: neither."""
  if a.size < 2 or bool(np.all(a[1:] >= a[:-1])):
    return 1
  return -1 if bool(np.all(a[1:] <= a[:-1])) else 0


def _slice_bound(a: np.ndarray, mono: int, value, side: str) -> int:
  """`Index.get_slice_bound`: where a slice that starts (`side` 'left') or
  stops ('right', exclusive position) at the label `value` is cut."""
  if mono == 1:
    return int(np.searchsorted(a, value, side=side))
  if mono == -1:
    other = 'right' if side == 'left' else 'left'
    return int(a.size - np.searchsorted(a[::-1], value, side=other))
  at = np.flatnonzero(a == value)
  if not at.size:
    raise KeyError(value)
  if at[-1] - at[0] + 1 != at.size:
    raise KeyError(f'Cannot get {side} slice bound for non-unique label: '
                   f'{value!r}')
  return int(at[0]) if side == 'left' else int(at[-1]) + 1


def slice_positions(labels, start=None, stop=None, step=None) -> np.ndarray:
  """int64 positions of `.sel(dim=slice(start, stop, step))` on the axis
  `labels`: what pandas' `Index.slice_indexer` selects.  Both bounds are
  inclusive and need not be labels on a monotonic axis (increasing or
  decreasing; on a decreasing one `slice(lo, hi)` with lo < hi is empty);
  `step` is a positional step applied after the bounds.  A bound that is not a
  label of a non-monotonic axis is a KeyError.  datetime64 / timedelta64 axes
  take datetime64 / timedelta64 bounds and strings, which are widened to their
  resolution (`_datetime_string_bounds`, `_duration_string_bounds`); an int or
  float there is a TypeError."""
  a, kind = _axis_values(labels)
  if a.ndim != 1:
    raise ValueError('labels must be one-dimensional')
  if step is not None and int(step) == 0:
    raise ValueError('slice step cannot be zero')
  step = None if step is None else int(step)
  mono = _monotonic(a)
  n = a.size
  strings = all(v is None or isinstance(v, str) for v in (start, stop))
  if kind == 'M' and mono != 1 and strings:
    # pandas' DatetimeIndex on an axis that is not increasing, string bounds:
    # a mask over the labels themselves, and both bounds must be labels
    keep = np.ones(n, dtype=bool)
    for side, v in enumerate((start, stop)):
      if v is None:
        continue
      b = _bound(v, kind, side)
      if not (a == b).any():
        raise KeyError('Value based partial slicing on non-monotonic '
                       'DatetimeIndexes with non-existing keys is not allowed.')
      keep &= (a >= b) if side == 0 else (a <= b)
    return np.flatnonzero(keep)[::step].astype(np.int64)
  inc = step is None or step >= 0
  if not inc:
    start, stop = stop, start
  lo = 0 if start is None else _slice_bound(a, mono, _bound(start, kind, 0),
                                            'left')
  hi = n if stop is None else _slice_bound(a, mono, _bound(stop, kind, 1),
                                           'right')
  if not inc:
    hi, lo = lo - 1, hi - 1
    hi = hi - n if hi == -1 else hi
    lo = lo - n if lo == -1 else lo
  return np.arange(n, dtype=np.int64)[slice(lo, hi, step)]


def list_positions(labels, wanted) -> np.ndarray:
  """int64 positions of `.sel(dim=[...])`: `sel_positions` for a list.  An
  absent label is a KeyError, a duplicated label gives its first position.
  Strings on a datetime64 / timedelta64 axis name one instant."""
  a = np.asarray(labels)
  kind = a.dtype.kind
  wanted = list(np.atleast_1d(np.asarray(wanted, dtype=object)))
  if kind in 'Mm':
    unit = 'datetime64[ns]' if kind == 'M' else 'timedelta64[ns]'
    want = np.array([_bound(w, kind, 0) for w in wanted],
                    dtype=np.int64).astype(unit)
  elif kind in 'iuf':
    if any(isinstance(w, str) for w in wanted):
      raise TypeError('string labels on a numeric axis: give them through '
                      'sel, not sel_strings')
    want = np.asarray(wanted, dtype=np.float64 if kind == 'f' or any(
        isinstance(w, float) for w in wanted) else np.int64)
  else:
    want = np.asarray(wanted, dtype=a.dtype if kind in 'US' else object)
  return sel_positions(a, want, 'not all values found in index: {label!r}')


class Reindex(t.NamedTuple):
  """`table` (int64, one axis per dim of `new_dims`) holds, per position of
  the new dims, the C-order position in the grid of `src_dims` of the input;
  -1 = none.  A name may stand in both: a dim that is re-indexed in place."""
  src_dims: tuple
  new_dims: tuple
  table: np.ndarray


def slab_table(in_dims, sizes, out_dims, re_: Reindex, n_inner: int):
  """int64 over the output's dims before the last `n_inner`: the input slab
  (C order over the input's dims before its last `n_inner`) each output slab
  is a copy of, -1 for a hole."""
  in_outer = tuple(in_dims[:len(in_dims) - n_inner])
  out_outer = tuple(out_dims[:len(out_dims) - n_inner])
  stride, s = {}, 1
  for d in reversed(in_outer):
    stride[d] = s
    s *= sizes[d]
  # the table's axes in the order the new dims stand in the output
  perm = sorted(range(len(re_.new_dims)),
                key=lambda i: out_outer.index(re_.new_dims[i]))
  table = np.transpose(re_.table, perm)
  hole = table < 0
  parts = np.unravel_index(np.where(hole, 0, table).ravel(),
                           [sizes[d] for d in re_.src_dims]) if table.size \
      else [np.zeros(0, np.int64)] * len(re_.src_dims)
  flat = np.zeros(table.size, dtype=np.int64)
  for d, p in zip(re_.src_dims, parts):
    flat += p.astype(np.int64) * stride[d]
  shape = [1] * len(out_outer)
  for i in perm:
    shape[out_outer.index(re_.new_dims[i])] = re_.table.shape[i]
  full = flat.reshape(shape)
  hole = hole.reshape(shape)
  for ax, d in enumerate(out_outer):
    if d in re_.new_dims:
      continue
    along = [1] * len(out_outer)
    along[ax] = sizes[d]
    full = full + (np.arange(sizes[d], dtype=np.int64) * stride[d]
                   ).reshape(along)
    hole = np.broadcast_to(hole, full.shape)
  return np.where(np.broadcast_to(hole, full.shape), -1, full)


def common_tail(in_dims, out_dims, re_: Reindex) -> int:
  """How many trailing dims input and output share behind the selection."""
  k = 0
  while (k < min(len(in_dims), len(out_dims))
         and in_dims[-1 - k] == out_dims[-1 - k]
         and in_dims[-1 - k] not in re_.src_dims
         and out_dims[-1 - k] not in re_.new_dims):
    k += 1
  return k


def in_place_dims(dims: tuple, src_dims: tuple, new_dims: tuple) -> tuple:
  """xarray's rule for vectorised indexing: walk the dims in order, the first
  indexed dim becomes `new_dims`, the other indexed dims go."""
  out: list = []
  for d in dims:
    if d in src_dims:
      if not any(n in out for n in new_dims):
        out.extend(new_dims)
    else:
      out.append(d)
  return tuple(out)


def compose(table: np.ndarray, prior: np.ndarray) -> np.ndarray:
  """A gather of a gather: `table` numbers the slabs of an earlier gather
  whose flat index is `prior`; the result numbers the slabs of its base.  A
  hole of either is a hole."""
  return np.where(table < 0, -1, prior[np.maximum(table, 0)])
