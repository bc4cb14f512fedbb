"""NumPy restatement of the lead-time derived variables (test side):
PrecipitationAccumulation (weatherbench2/derived_variables.py:471-528) and
AggregatePrecipitationAccumulation (:685-720) on plain arrays with dim names.

The rolling sum is xarray's `rolling(dim=w).sum()` with its default
min_periods = w: NaN where the window is incomplete or holds a NaN.  Every
window is summed afresh, oldest term first, in the field's dtype --
((t[l-w+1] + t[l-w+2]) + ...) + t[l] -- vectorised over the field: the order
the kernel uses, so that the two can be compared bit for bit.  Integers (and
anything that is not float32 / float64) become float64 first, as xarray's
rolling sum makes them.
"""
import numpy as np


def as_float(x: np.ndarray) -> np.ndarray:
  x = np.asarray(x)
  return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def rolling_sum(terms: np.ndarray, axis: int, w: int) -> np.ndarray:
  """out[l] = the ordered sum of terms[l-w+1 .. l] along `axis`, NaN for
  l < w - 1."""
  t = np.moveaxis(as_float(terms), axis, 0)
  out = np.full(t.shape, np.nan, dtype=t.dtype)
  with np.errstate(all='ignore'):
    for l in range(w - 1, t.shape[0]):
      s = t[l - w + 1].copy()
      for j in range(l - w + 2, l + 1):
        s = s + t[j]
      out[l] = s
  return np.moveaxis(out, 0, axis)


def rolling_abs_sum(terms: np.ndarray, axis: int, w: int) -> np.ndarray:
  """Sum of |term| over each window in float64 (what the error bound of a
  reordered sum scales with); NaN where the window is incomplete."""
  with np.errstate(all='ignore'):
    return rolling_sum(np.abs(as_float(terms).astype(np.float64)), axis, w)


def _with_first_lead(acc: np.ndarray, axis: int) -> np.ndarray:
  shape = list(acc.shape)
  shape[axis] = 1
  return np.concatenate([np.full(shape, np.nan, dtype=acc.dtype), acc], axis)


def precipitation_accumulation(x, axis: int, w: int, clamp: bool = True):
  """The rolling sum over w leads of x[l] - x[l - 1]; NaN at the first w
  leads; sums below zero become 0.0 when `clamp` (NaN and -0.0 stay)."""
  x = as_float(x)
  with np.errstate(all='ignore'):
    acc = rolling_sum(np.diff(x, axis=axis), axis, w)
    if clamp:
      acc = np.where(acc < 0, np.zeros((), acc.dtype), acc)
  return _with_first_lead(acc, axis)


def precipitation_abs_sum(x, axis: int, w: int) -> np.ndarray:
  x = as_float(x)
  with np.errstate(all='ignore'):
    return _with_first_lead(rolling_abs_sum(np.diff(x, axis=axis), axis, w),
                            axis)


def steps_of(class_name: str, fields: dict, coords: dict) -> int:
  """The window in leads (derived_variables.py:510-514, :713-717)."""
  if class_name == 'PrecipitationAccumulation':
    lead = np.asarray(coords[fields['lead_time_name']])
    timestep = np.diff(lead)
    assert np.all(timestep == timestep[0]), 'All time steps must be equal.'
    steps = float(np.timedelta64(fields['accumulation_hours'], 'h')
                  / timestep[0])
  else:
    steps = float(np.timedelta64(fields['accumulation_hours'], 'h')
                  / np.timedelta64(fields['raw_accumulation_hours'], 'h'))
  assert steps.is_integer(), 'Accumulation time must be multiple of timestep.'
  return int(steps)


def compute(class_name, fields, variables, coords, with_abs: bool = False):
  """(dims, array) of class `class_name` with constructor fields `fields` on
  `variables` = {name: (dims, array)}; with_abs: (dims, array, the windows'
  sums of |term| in float64, the window in leads)."""
  w = steps_of(class_name, fields, coords)
  if class_name == 'PrecipitationAccumulation':
    dims, x = variables[fields['total_precipitation_name']]
    axis = tuple(dims).index(fields['lead_time_name'])
    out = precipitation_accumulation(x, axis, w,
                                     fields['set_negative_to_zero'])
    mag = precipitation_abs_sum(x, axis, w) if with_abs else None
  elif class_name == 'AggregatePrecipitationAccumulation':
    dims, x = variables[fields['raw_accumulation_name']]
    axis = tuple(dims).index(fields['lead_time_name'])
    out = rolling_sum(x, axis, w)
    mag = rolling_abs_sum(x, axis, w) if with_abs else None
  else:
    raise KeyError(class_name)
  return (tuple(dims), out, mag, w) if with_abs else (tuple(dims), out)
