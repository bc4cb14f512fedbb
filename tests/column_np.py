"""NumPy restatement of the level-column derived variables (test side): plain
arrays with dim names and the same expressions as
weatherbench2/derived_variables.py:179-228 and :341-430, so that NumPy's own
type promotion decides every dtype.  `integrate` is np.trapezoid along the
coordinate, `differentiate` np.gradient (edge_order=1), the zonal mean
np.nanmean (xarray's `mean` skips NaN for floats).
"""
import numpy as np
import scipy.integrate

from tests import derived_np

G = 9.81


def level_slice(level, level_min, level_max) -> slice:
  """Positions of the inclusive label slice on a monotonic coordinate, as
  pandas resolves it (an index that falls selects nothing for a (small,
  large) pair of bounds)."""
  level = np.asarray(level)
  n = len(level)
  d = np.diff(level)
  if level_min is None and level_max is None:
    return slice(0, n)
  if (d > 0).all():
    lo = 0 if level_min is None else np.searchsorted(level, level_min, 'left')
    hi = n if level_max is None else np.searchsorted(level, level_max, 'right')
  else:
    assert (d < 0).all(), 'numeric bounds need a monotonic level coordinate'
    lo = 0 if level_min is None else int((level > level_min).sum())
    hi = n if level_max is None else int((level >= level_max).sum())
  return slice(int(lo), max(int(lo), int(hi)))


def integrate(f, dims, level):
  axis = dims.index('level')
  return (tuple(d for d in dims if d != 'level'),
          np.trapezoid(f, np.asarray(level), axis=axis))


def compute(class_name, fields, variables, coords):
  """(dims, array) of class `class_name` with constructor fields `fields` on
  `variables` = {name: (dims, array)}."""
  get = lambda key: variables[fields[key]]
  level = np.asarray(coords['level'])
  with np.errstate(all='ignore'):
    if class_name == 'TotalColumnWater':
      dims, q = get('water_species_name')
      out_dims, integral = integrate(q, dims, level)
      return out_dims, 1 / G * integral
    if class_name == 'IntegratedWaterTransport':
      (dims, q), (ud, u), (vd, v) = (get('water_species_name'), get('u_name'),
                                     get('v_name'))
      assert dims == ud == vd
      axis = dims.index('level')
      sel = level_slice(level, fields['level_min'], fields['level_max'])
      at = tuple(sel if a == axis else slice(None) for a in range(len(dims)))
      out_dims, u_int = integrate((q * u)[at], dims, level[sel])
      _, v_int = integrate((q * v)[at], dims, level[sel])
      return out_dims, (1 / G) * np.sqrt(u_int**2 + v_int**2)
    if class_name == 'LapseRate':
      (dims, temperature), (zd, z) = (get('temperature_name'),
                                      get('geopotential_name'))
      assert dims == zd
      dt_dp = derived_np.differentiate(temperature, dims, coords, 'level')
      dz_dp = (1 / G) * derived_np.differentiate(z, dims, coords, 'level')
      return dims, dt_dp / dz_dp
    (dims, u), (vd, v) = get('u_name'), get('v_name')
    assert dims == vd
    if class_name == 'VerticalVelocity':
      divergence = (derived_np.d_dx(u, dims, coords)
                    + derived_np.d_dy(v, dims, coords))
      return dims, cumulative(divergence, dims, level)
    if class_name == 'EddyKineticEnergy':
      axis = dims.index('longitude')
      u_delta = u - np.nanmean(u, axis=axis, keepdims=True)
      v_delta = v - np.nanmean(v, axis=axis, keepdims=True)
      out_dims, integral = integrate(u_delta**2 + v_delta**2, dims, level)
      return out_dims, (1 / 2) * integral
  raise KeyError(class_name)


def cumulative(divergence, dims, level):
  """derived_variables.py:201-208 on a divergence field."""
  pressure = 100 * np.asarray(level)
  return scipy.integrate.cumulative_trapezoid(
      -divergence, x=pressure, axis=dims.index('level'), initial=0)
