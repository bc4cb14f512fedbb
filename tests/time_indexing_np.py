"""The three time re-indexing scripts restated in NumPy without xarray, one
output slab at a time, and the scatter as take, fill and astype.  Written for
being obviously right, not fast: the module under test and the kernel are
compared with this as bit patterns.

A variable is (dims, array); every function returns {name: (dims, array)} and
the new coordinates.
"""
import datetime

import numpy as np

DELTA = 'prediction_timedelta'


def scatter(flat: np.ndarray, dest_to_src, out_dtype=None) -> np.ndarray:
  """[n_out_slab, n_point]: output slab d is input slab dest_to_src[d] of
  `flat` [n_in_slab, n_point] cast to `out_dtype`, NaN where it is -1."""
  table = np.asarray(dest_to_src, dtype=np.int64).reshape(-1)
  out_dtype = np.dtype(out_dtype or flat.dtype)
  if flat.shape[0]:
    out = np.take(flat, np.maximum(table, 0), axis=0)
  else:
    out = np.zeros((table.size,) + flat.shape[1:], dtype=flat.dtype)
  out[table < 0] = np.nan
  with np.errstate(over='ignore'):
    return out.astype(out_dtype)


def same_bits(a, b) -> bool:
  a, b = np.asarray(a), np.asarray(b)
  return (a.dtype == b.dtype and a.shape == b.shape
          and np.ascontiguousarray(a).tobytes()
          == np.ascontiguousarray(b).tobytes())


def _stamp(t) -> datetime.datetime:
  return np.datetime64(t, 'us').astype(datetime.datetime)


def expand_climatology(variables: dict, coords: dict, times) -> tuple:
  """Per time: the (hour, dayofyear) plane of the climatology; the new time
  dim stands where the first of the two stood."""
  doys = np.asarray(coords['dayofyear']).tolist()
  hours = np.asarray(coords['hour']).tolist() if 'hour' in coords else None
  out = {}
  for name, (dims, array) in variables.items():
    picked = [d for d in dims if d in ('hour', 'dayofyear')]
    if not picked:
      out[name] = (tuple(dims), array)
      continue
    front = np.moveaxis(array, [dims.index(d) for d in picked],
                        range(len(picked)))
    planes = []
    for t in times:
      stamp = _stamp(t)
      where = {'dayofyear': doys.index(stamp.timetuple().tm_yday)}
      if hours is not None:
        where['hour'] = hours.index(stamp.hour)
      planes.append(front[tuple(where[d] for d in picked)])
    rest = [d for d in dims if d not in picked]
    stacked = np.stack(planes, axis=0) if planes else np.zeros(
        (0,) + front.shape[len(picked):], dtype=array.dtype)
    # the dims that stay and stand before the first picked one
    at = min(dims.index(d) for d in picked)
    out[name] = (tuple(rest[:at] + ['time'] + rest[at:]),
                 np.moveaxis(stacked, 0, at))
  return out, {'time': np.asarray(times)}


def offset_and_spacing(inits, leads) -> tuple:
  step_init = (inits[1] - inits[0])
  step_lead = (leads[1] - leads[0])
  spacing = int(step_init // step_lead)
  if leads[0] == np.timedelta64(0, 'ns'):
    return 0, spacing
  return int(np.flatnonzero(leads == spacing * step_lead)[0]), spacing


def index_on_valid_time(variables: dict, coords: dict, mode: str) -> tuple:
  inits = np.asarray(coords['time']).astype('datetime64[ns]')
  leads = np.asarray(coords[DELTA]).astype('timedelta64[ns]')
  init_at = {t: i for i, t in enumerate(inits.tolist())}
  lead_at = {t: j for j, t in enumerate(leads.tolist())}
  if mode == 'valid_and_delta':
    offset, spacing = offset_and_spacing(inits, leads)
    kept = list(range(offset, len(leads), spacing))
    valid = sorted({int(a) + int(leads[j].astype(np.int64))
                    for a in inits.astype(np.int64) for j in kept})
    rows, names = [], {'time': 'time', DELTA: DELTA}
    for v in valid:  # (valid, lead) <- (init = valid - lead, lead)
      rows.append([(init_at.get(v - int(leads[j].astype(np.int64))), j)
                   for j in kept])
    new = {'time': np.array(valid, dtype=np.int64).astype('datetime64[ns]'),
           DELTA: leads[kept]}
  else:
    valid = sorted({int(a) + int(b) for a in inits.astype(np.int64)
                    for b in leads.astype(np.int64)})
    rows, names = [], {'time': 'init', DELTA: 'time'}
    for i, a in enumerate(inits.astype(np.int64)):
      rows.append([(i, lead_at.get(v - int(a))) for v in valid])
    new = {'init': inits,
           'time': np.array(valid, dtype=np.int64).astype('datetime64[ns]')}
  out = {}
  for name, (dims, array) in variables.items():
    a, b = dims.index('time'), dims.index(DELTA)
    front = np.moveaxis(array, [a, b], [0, 1])
    hole = np.full(front.shape[2:], np.nan, dtype=np.float32)
    with np.errstate(over='ignore'):
      grid = [[hole if i is None or j is None
               else front[i, j].astype(np.float32) for i, j in row]
              for row in rows]
    block = np.array(grid, dtype=np.float32).reshape(
        (len(rows), len(rows[0])) + front.shape[2:])
    # block is [valid][lead] or [init][valid]: its axes stand for the input's
    # (time, lead) in this order
    out[name] = (tuple(names.get(d, d) for d in dims),
                 np.moveaxis(block, [0, 1], [a, b]))
  return out, new


def probabilistic(variables: dict, coords: dict, sampled: np.ndarray,
                  deltas: np.ndarray, time_dim: str = 'time',
                  realization: str = 'realization') -> dict:
  """Member r of (init i, lead d) is the truth at sampled[r, i] + deltas[d];
  dims (realization, lead, time, ...the others)."""
  at = {t: k for k, t in enumerate(
      np.asarray(coords[time_dim]).astype('datetime64[ns]').tolist())}
  n_member, n_init = sampled.shape
  out = {}
  for name, (dims, array) in variables.items():
    if time_dim not in dims:
      continue
    front = np.moveaxis(array, dims.index(time_dim), 0)
    block = np.empty((n_member, len(deltas), n_init) + front.shape[1:],
                     dtype=array.dtype)
    for r in range(n_member):
      for d, delta in enumerate(deltas):
        for i in range(n_init):
          block[r, d, i] = front[at[(sampled[r, i] + delta).tolist()]]
    out[name] = ((realization, DELTA, time_dim) + tuple(
        x for x in dims if x != time_dim), block)
  return out
