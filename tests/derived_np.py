"""NumPy restatement of the derived variables (test side): plain arrays with
dim names, the same expressions as weatherbench2/derived_variables.py so that
NumPy's own type promotion decides every dtype.  `differentiate` is
np.gradient along the coordinate (edge_order=1), which is what xarray calls.
"""
import numpy as np

EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2
METERS_PER_DEGREE = 2 * np.pi * EARTH_RADIUS_M / 360
OMEGA = 7.292e-5


def _along(values, dims, name):
  """1-D `values` shaped to broadcast along dim `name` of `dims`."""
  shape = [1] * len(dims)
  shape[dims.index(name)] = len(values)
  return np.asarray(values).reshape(shape)


def differentiate(f, dims, coords, name):
  return np.gradient(f, np.asarray(coords[name]), axis=dims.index(name),
                     edge_order=1)


def d_dx(f, dims, coords):
  cos_theta = _along(np.cos(np.deg2rad(coords['latitude'])), dims, 'latitude')
  with np.errstate(all='ignore'):
    out = differentiate(f, dims, coords, 'longitude') / cos_theta \
        / METERS_PER_DEGREE
  return np.where(cos_theta > 1e-6, out, 0.0)


def d_dy(f, dims, coords):
  return differentiate(f, dims, coords, 'latitude') / METERS_PER_DEGREE


def geostrophic_wind(z, dims, coords):
  coriolis = _along(2 * OMEGA * np.sin(np.deg2rad(coords['latitude'])), dims,
                    'latitude')
  with np.errstate(all='ignore'):
    return (-d_dy(z, dims, coords) / coriolis,
            +d_dx(z, dims, coords) / coriolis)


def compute(class_name, fields, variables, coords):
  """(dims, array) of class `class_name` with constructor fields `fields` on
  `variables` = {name: (dims, array)}."""
  get = lambda key: variables[fields[key]]
  with np.errstate(all='ignore'):
    if class_name == 'WindSpeed':
      (dims, u), (vd, v) = get('u_name'), get('v_name')
      assert dims == vd
      return dims, np.sqrt(u**2 + v**2)
    if class_name == 'RelativeHumidity':
      (td, temperature) = get('temperature_name')
      (dims, q) = get('specific_humidity_name')
      assert dims == td
      pressure = np.asarray(coords[fields['pressure_name']])
      if len(dims) > 1 or dims != (fields['pressure_name'],):
        pressure = _along(pressure, dims, fields['pressure_name'])
      svp = 6.112 * np.exp(17.67 * (temperature - 273.15)
                           / (temperature - 29.65))
      mixing_ratio = q / (1 - q)
      saturation_mixing_ratio = 0.622 * svp / (pressure - svp)
      return dims, mixing_ratio / saturation_mixing_ratio
    if class_name in ('WindDivergence', 'WindVorticity'):
      (dims, u), (vd, v) = get('u_name'), get('v_name')
      assert dims == vd
      if class_name == 'WindDivergence':
        return dims, d_dx(u, dims, coords) + d_dy(v, dims, coords)
      return dims, d_dx(v, dims, coords) - d_dy(u, dims, coords)
    dims, z = get('geopotential_name')
    u_geo, v_geo = geostrophic_wind(z, dims, coords)
    if class_name == 'GeostrophicWindSpeed':
      return dims, np.sqrt(u_geo**2 + v_geo**2)
    if class_name == 'UComponentOfGeostrophicWind':
      return dims, u_geo
    if class_name == 'VComponentOfGeostrophicWind':
      return dims, v_geo
    (ud, u), (vd, v) = get('u_name'), get('v_name')
    assert ud == dims and vd == dims
    if class_name == 'AgeostrophicWindSpeed':
      return dims, np.sqrt((u - u_geo) ** 2 + (v - v_geo) ** 2)
    if class_name == 'UComponentOfAgeostrophicWind':
      return dims, u - u_geo
    if class_name == 'VComponentOfAgeostrophicWind':
      return dims, v - v_geo
  raise KeyError(class_name)


def apply_gradient_table(f, table, uniform, axis=0):
  """The index-clamped form wb2_derived_stencil evaluates, in float64."""
  f = np.moveaxis(np.asarray(f, dtype=np.float64), axis, 0)
  n = f.shape[0]
  i = np.arange(n)
  lo, hi = f[np.maximum(i - 1, 0)], f[np.minimum(i + 1, n - 1)]
  shape = (n,) + (1,) * (f.ndim - 1)
  a, b, c, den = (row.reshape(shape) for row in table)
  diff_form = (uniform | (i == 0) | (i == n - 1)).reshape(shape)
  with np.errstate(all='ignore'):
    out = np.where(diff_form, (hi - lo) / den, (a * lo + b * f) + c * hi)
  return np.moveaxis(out, 0, axis)
