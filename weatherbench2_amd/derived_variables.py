"""GPU derived variables with the reference's `DerivedVariable` protocol.

Every class of weatherbench2/derived_variables.py is here, with the
reference's names, dataclass fields and defaults, and is computed by a HIP
kernel (csrc/derived_fields.hip unless named):

  pointwise           WindSpeed, RelativeHumidity
  horizontal stencil  WindDivergence, WindVorticity, GeostrophicWindSpeed,
                      U/VComponentOfGeostrophicWind, AgeostrophicWindSpeed,
                      U/VComponentOfAgeostrophicWind

  level column        TotalColumnWater, IntegratedWaterTransport, LapseRate,
                      VerticalVelocity, EddyKineticEnergy
                      (csrc/derived_column.hip)

  lead time           PrecipitationAccumulation,
                      AggregatePrecipitationAccumulation
                      (csrc/derived_lead.hip)

The first three families act inside one `init_time=1,lead_time=1` chunk.  The
lead-time family needs the whole lead axis in one chunk -- what its
`core_dims` ask a chunker for: `compute()` on a dataset, the in-memory driver
and `evaluate_chunks` on chunks that hold every lead.

They MATERIALISE their result as one more field of the chunk, in the dtype the
reference's NumPy expression gives; `evaluation.evaluate_chunks` computes them
once per chunk where the chunk enters the window, so that chunk programs and
windows treat them as ordinary variables.
`ZonalEnergySpectrum` (derived_variables.py:531-626, driven by
scripts/compute_zonal_energy_spectrum.py) is the spectral one.

Names: DERIVED_VARIABLE_DICT holds the pointwise and stencil entries of the
reference's dictionary, COLUMN_VARIABLE_DICT the seven level-column ones,
ALL_DERIVED_VARIABLES both in the reference's key order, LEAD_VARIABLE_DICT
the four precipitation accumulations, and REFERENCE_DERIVED_VARIABLES all 22
keys in the reference's order: a `--derived_variables=` name is resolved
there.
"""
from __future__ import annotations

import dataclasses
import threading
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import feeder
from weatherbench2_amd import operands
from weatherbench2_amd import plan as plan_lib
from weatherbench2_amd import xarray_lite as xl

EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2  # schema.py:59


@dataclasses.dataclass
class DerivedVariable:
  """Derived variable base class (derived_variables.py:29-56)."""

  @property
  def base_variables(self) -> list:
    return []

  @property
  def core_dims(self):
    raise NotImplementedError

  @property
  def all_input_core_dims(self) -> set:
    """The set of all input core dimensions (derived_variables.py:50-52)."""
    return set().union(*self.core_dims[0])

  def compute(self, dataset):
    raise NotImplementedError


@dataclasses.dataclass
class ZonalEnergySpectrum(DerivedVariable):
  """Energy spectrum along the zonal direction (derived_variables.py:531-626).

  S[0] = C |F[0]|^2, S[k] = 2 C |F[k]|^2 with F = rfft(f, norm='forward') and C
  the circumference of the latitude circle.  The result keeps the input dims
  with `longitude` replaced by a trailing `zonal_wavenumber`, and carries the
  `frequency` / `wavelength` coordinates of the reference.
  """

  variable_name: str

  @property
  def base_variables(self) -> list:
    return [self.variable_name]

  @property
  def core_dims(self):
    return (['longitude'],), ['zonal_wavenumber']

  @staticmethod
  def _circumference(latitude: np.ndarray) -> np.ndarray:
    """derived_variables.py:578-581."""
    circum_at_equator = 2 * np.pi * EARTH_RADIUS_M
    return np.cos(np.asarray(latitude) * np.pi / 180) * circum_at_equator

  def lon_spacing_m(self, dataset) -> np.ndarray:
    """derived_variables.py:583-590 (ValueError on non-uniform spacing)."""
    dataset = xl.as_dataset(dataset)
    longitude = np.asarray(dataset.coords['longitude'])
    diffs = np.diff(longitude)
    if np.max(np.abs(diffs - diffs[0])) > 1e-3:
      raise ValueError(
          f'Expected uniform longitude spacing. {longitude=}')
    latitude = np.asarray(dataset.coords['latitude'])
    return self._circumference(latitude) * diffs[0] / 360

  def compute(self, dataset, time_mean_dim: t.Optional[str] = None,
              skipna: bool = True) -> xl.DataArray:
    """Zonal power at each wavenumber.  `time_mean_dim` (an extension) fuses
    the mean over that dim, as scripts/compute_zonal_energy_spectrum.py:234
    does afterwards with xbeam.Mean."""
    if xl.is_xarray(dataset):
      return xl.like_input(self.compute(xl.as_dataset(dataset), time_mean_dim,
                                        skipna), dataset)
    dataset = xl.as_dataset(dataset)
    spacing = self.lon_spacing_m(dataset)
    da = dataset[self.variable_name]
    for d in ('latitude', 'longitude'):
      if d not in da.dims:
        raise ValueError(f'{d!r} missing from {da.dims}')
    rest = [d for d in da.dims if d not in ('latitude', 'longitude')]
    if time_mean_dim is not None:
      if time_mean_dim not in rest:
        raise ValueError(f'{time_mean_dim!r} missing from {da.dims}')
      rest = [time_mean_dim] + [d for d in rest if d != time_mean_dim]
    order = tuple(rest) + ('latitude', 'longitude')
    moved = da if da.dims == order else da.transpose(*order)
    device = engine.require_gpu()
    x = engine.as_device_tensor(moved.data, device)
    if x.dtype not in (torch.float32, torch.float64):
      x = x.to(torch.float64)
    latitude = np.asarray(dataset.coords['latitude'])
    longitude = np.asarray(dataset.coords['longitude'])
    circ = torch.as_tensor(self._circumference(latitude).astype(np.float64)
                           ).to(device)
    n_time = x.shape[0] if time_mean_dim is not None else 0
    out = engine.zonal_spectrum(x, circ, len(latitude), n_time, skipna)
    out_dims = tuple(d for d in order[:-1] if d != time_mean_dim) + (
        'zonal_wavenumber',)
    # apply_ufunc keeps the input order with longitude moved last
    # (derived_variables.py:604-609).
    ref_dims = tuple(d for d in da.dims if d not in ('longitude',
                                                      time_mean_dim)
                     ) + ('zonal_wavenumber',)
    n_bins = len(longitude) // 2 + 1
    coords = {k: v for k, v in dataset.coords.items()
              if k not in ('longitude', time_mean_dim)}
    coords['zonal_wavenumber'] = np.arange(n_bins)
    with np.errstate(divide='ignore'):
      frequency = np.fft.rfftfreq(len(longitude))[:, None] / spacing[None, :]
      wavelength = 1 / frequency
    coords['frequency'] = xl.DataArray(frequency,
                                       ('zonal_wavenumber', 'latitude'))
    coords['wavelength'] = xl.DataArray(wavelength,
                                        ('zonal_wavenumber', 'latitude'))
    result = xl.DataArray(feeder.download(out), out_dims, coords,
                          self.variable_name)
    if out_dims != ref_dims:
      result = result.transpose(*ref_dims)
      result = xl.DataArray(np.ascontiguousarray(result.data), ref_dims,
                            coords, self.variable_name)
    return result


# ---------------------------------------------------------------------------
# Materialising derived variables (csrc/derived_fields.hip)
# ---------------------------------------------------------------------------
def _result_coords(dataset: xl.Dataset, dims: tuple) -> dict:
  return {k: v for k, v in dataset.coords.items()
          if (set(v.dims) <= set(dims) if isinstance(v, xl.DataArray)
              else k in dims)}


@dataclasses.dataclass
class _MaterializedVariable(DerivedVariable):
  """A derived variable that one kernel launch writes as a field of its own.

  `compute` follows the protocol (xarray in, xarray out; lite in, lite out; a
  device result for device inputs, a NumPy one for host inputs);
  `compute_on_device` always leaves the result in HBM: that is what
  `evaluation.evaluate_chunks` assigns into the chunk."""

  def compute(self, dataset):
    if xl.is_xarray(dataset):
      return xl.like_input(self.compute(xl.as_dataset(dataset)), dataset)
    dataset = xl.as_dataset(dataset)
    result = self.compute_on_device(dataset)
    if any(operands.on_device(dataset[name].data)
           for name in self.base_variables if name in dataset.data_vars):
      return result
    engine.order_read(result.data)
    return xl.DataArray(feeder.download(result.data.contiguous()), result.dims,
                        result.coords, result.name)

  def compute_on_device(self, dataset: xl.Dataset) -> xl.DataArray:
    raise NotImplementedError


def is_materialized(dv) -> bool:
  """True for this module's classes that `evaluate_chunks` computes up front
  (a foreign duck-typed object, or ZonalEnergySpectrum, is not)."""
  return isinstance(dv, _MaterializedVariable)


def _pointwise(mode: str, dataset: xl.Dataset, a_name: str, b_name: str,
               order_of: int, pressure_name: t.Optional[str] = None):
  device = engine.require_gpu()
  das = [dataset[a_name], dataset[b_name]]
  order = tuple(das[order_of].dims)
  if set(das[0].dims) != set(das[1].dims):
    raise ValueError(f'{a_name} {das[0].dims} and {b_name} {das[1].dims} must '
                     'have the same dims')
  sizes = das[order_of].sizes
  dtype = operands.float_dtype(das[0].dtype, das[1].dtype)
  out_dtype, n_inner, pressure = dtype, min(2, len(order)), None
  if pressure_name is not None:
    p = dataset[pressure_name]  # the COORDINATE, broadcast by name (:464)
    missing = [d for d in p.dims if d not in order]
    if missing:
      raise ValueError(f'{pressure_name} dims {missing} not in {order}')
    pvals = np.asarray(p.values)
    out_dtype = operands.float_dtype(dtype, pvals.dtype)
    # a block = the trailing dims the pressure does not vary along
    last = max([order.index(d) for d in p.dims], default=-1)
    n_inner = len(order) - 1 - last
    outer = order[:last + 1]
    pvals = np.transpose(pvals, [p.dims.index(d) for d in outer if d in p.dims])
    pvals = pvals.reshape([sizes[d] if d in p.dims else 1 for d in outer])
    pressure = np.broadcast_to(pvals, [sizes[d] for d in outer]).ravel()
  ops = [operands.operand(da, order, device, dtype, n_inner) for da in das]
  shape = tuple(sizes[d] for d in order)
  n_point = int(np.prod(shape[len(order) - n_inner:], dtype=np.int64))
  n_slab = int(np.prod(shape[:len(order) - n_inner], dtype=np.int64))
  if pressure is None and all(tab is None for _, tab in ops):
    n_slab, n_point = 1, n_slab * n_point  # one stream, wide whatever the rows
  if n_slab * n_point == 0:
    return xl.DataArray(torch.empty(shape, dtype=out_dtype, device=device),
                        order, _result_coords(dataset, order))
  scalar = None
  if pressure is not None:
    np_out = np.float32 if out_dtype == torch.float32 else np.float64
    host = np.ascontiguousarray(pressure, dtype=np_out)
    if np_out is np.float32:  # (the table upload moves 8-byte words)
      host = np.concatenate([host, np.zeros(host.size % 2, np.float32)])
    scalar = engine.upload_table(host.view(np.int64), device).view(out_dtype)[
        :n_slab]
  out = engine.derived_pointwise(
      mode, ops[0][0], operands.table_tensor(ops[0][1], device), ops[1][0],
      operands.table_tensor(ops[1][1], device), n_slab, n_point, out_dtype,
      scalar).reshape(shape)
  return xl.DataArray(out, order, _result_coords(dataset, order))


@dataclasses.dataclass
class _WindVariable(_MaterializedVariable):
  """A variable derived from U and V wind components
  (derived_variables.py:59-73)."""

  u_name: str
  v_name: str

  @property
  def base_variables(self) -> list:
    return [self.u_name, self.v_name]


@dataclasses.dataclass
class WindSpeed(_WindVariable):
  """Wind speed sqrt(u**2 + v**2) (derived_variables.py:76-99): three correctly
  rounded operations in the input dtype, bit-identical to NumPy."""

  u_name: str
  v_name: str

  @property
  def base_variables(self) -> list:
    return [self.u_name, self.v_name]

  @property
  def core_dims(self):
    return ([], []), []

  def compute_on_device(self, dataset):
    return _pointwise('wind_speed', dataset, self.u_name, self.v_name, 0)


@dataclasses.dataclass
class RelativeHumidity(_MaterializedVariable):
  """Relative humidity from specific humidity, MetPy's formula with Bolton's
  (1980) saturation vapour pressure (derived_variables.py:433-468).  Pressure
  (hPa) is the COORDINATE named `pressure_name`, temperature is in Kelvin."""

  temperature_name: str = 'temperature'
  specific_humidity_name: str = 'specific_humidity'
  pressure_name: str = 'level'

  @property
  def base_variables(self) -> list:
    return [self.temperature_name, self.specific_humidity_name,
            self.pressure_name]

  @property
  def core_dims(self):
    return ([], []), []

  def compute_on_device(self, dataset):
    return _pointwise('relative_humidity', dataset, self.temperature_name,
                      self.specific_humidity_name, 1, self.pressure_name)


_STENCIL_TABLES: dict = {}
_STENCIL_TABLES_LOCK = threading.Lock()


def _stencil_tables(rows: np.ndarray, cols: np.ndarray, latitude: np.ndarray):
  """Host tables of one coordinate set, made once (like the latitude weights
  of a plan): np.gradient coefficients of both axes, cos / Coriolis."""
  key = tuple(engine.digest(np.ascontiguousarray(x)) + str(x.dtype).encode()
              for x in (rows, cols, latitude))
  with _STENCIL_TABLES_LOCK:
    hit = _STENCIL_TABLES.get(key)
    if hit is None:
      if len(_STENCIL_TABLES) >= 64:
        _STENCIL_TABLES.clear()
      hit = _STENCIL_TABLES[key] = (plan_lib.gradient_tables(rows),
                                    plan_lib.gradient_tables(cols),
                                    plan_lib.latitude_tables(latitude))
  return hit


def _stencil_launch(mode: str, dataset: xl.Dataset, names: t.Sequence[str],
                    lead: int):
  """One launch of the stencil kernel.  `names` = (field differentiated along
  longitude, along latitude[, u, v]).  Returns (the contiguous result with its
  dims in `order` = the other dims, then the two spatial ones; order; the dims
  of `names[lead]`, the first operand of the reference's expression)."""
  device = engine.require_gpu()
  das = [dataset[n] for n in names]
  dims = tuple(das[lead].dims)
  for n, da in zip(names, das):
    if set(da.dims) != set(dims):
      raise ValueError(f'{n} {da.dims} and {names[lead]} {dims} must have the '
                       'same dims')
  spatial = tuple(d for d in dims if d in ('latitude', 'longitude'))
  if len(spatial) != 2:
    raise ValueError(f'{names[lead]}: needs latitude and longitude, has {dims}')
  order = tuple(d for d in dims if d not in spatial) + spatial
  (row_coef, row_uniform), (col_coef, col_uniform), lat_tables = _stencil_tables(
      xl.coord_values(dataset, spatial[0]),
      xl.coord_values(dataset, spatial[1]),
      xl.coord_values(dataset, 'latitude'))
  dtype = operands.float_dtype(*[da.dtype for da in das])
  seen: dict = {}
  ops = []
  for n, da in zip(names, das):  # (the geostrophic modes name one field twice)
    if n not in seen:
      seen[n] = operands.operand(da, order, device, dtype, 2)
    ops.append(seen[n])
  sizes = das[lead].sizes
  shape = tuple(sizes[d] for d in order)
  n_slab = int(np.prod(shape[:-2], dtype=np.int64))
  tabs = {n: operands.table_tensor(tab, device)
          for n, (_, tab) in seen.items()}
  out = engine.derived_stencil(
      mode, [x for x, _ in ops], [tabs[n] for n in names], n_slab, shape[-2],
      shape[-1], spatial[0] == 'latitude',
      engine.upload_f64_table(row_coef, device), row_uniform,
      engine.upload_f64_table(col_coef, device), col_uniform,
      engine.upload_f64_table(lat_tables, device), plan_lib.METERS_PER_DEGREE
  ).reshape(shape)
  return out, order, dims


def _stencil(mode: str, dataset: xl.Dataset, names: t.Sequence[str],
             lead: int) -> xl.DataArray:
  """The stencil kernel's result with the dims of `names[lead]`."""
  out, order, dims = _stencil_launch(mode, dataset, names, lead)
  if order != dims:
    out = out.permute(*[order.index(d) for d in dims])
  return xl.DataArray(out, dims, _result_coords(dataset, dims))


@dataclasses.dataclass
class _3DWindVariable(_MaterializedVariable):
  """A variable derived from 3D U and V wind components
  (derived_variables.py:132-146)."""

  u_name: str = 'u_component_of_wind'
  v_name: str = 'v_component_of_wind'

  @property
  def base_variables(self) -> list:
    return [self.u_name, self.v_name]

  @property
  def core_dims(self):
    lon_lat = ['longitude', 'latitude']
    return (lon_lat, lon_lat), lon_lat


@dataclasses.dataclass
class WindDivergence(_3DWindVariable):
  """Wind divergence d/dx u + d/dy v (derived_variables.py:124-125, 149-161).
  Derivatives are `np.gradient` along the coordinate in degrees (one-sided at
  both ends; longitude does not wrap, as in the reference); d/dx is 0.0 at the
  poles."""

  def compute_on_device(self, dataset):
    return _stencil('divergence', dataset, (self.u_name, self.v_name), 0)


@dataclasses.dataclass
class WindVorticity(_3DWindVariable):
  """Wind vorticity d/dx v - d/dy u (derived_variables.py:128-129, 164-176)."""

  def compute_on_device(self, dataset):
    return _stencil('vorticity', dataset, (self.v_name, self.u_name), 0)


@dataclasses.dataclass
class _GeostrophicWindVariable(_MaterializedVariable):
  """Base class for geostrophic wind variables (derived_variables.py:231-260):
  u_g = -d/dy geopotential / f, v_g = +d/dx geopotential / f with the Coriolis
  parameter f = 2 Omega sin(latitude).  On the equator the result is +-inf /
  NaN, as in the reference: evaluate over a region."""

  geopotential_name: str = 'geopotential'
  _mode: t.ClassVar[str] = ''

  @property
  def base_variables(self) -> list:
    return [self.geopotential_name]

  @property
  def core_dims(self):
    lon_lat = ['longitude', 'latitude']
    return (lon_lat,), lon_lat

  def compute_on_device(self, dataset):
    z = self.geopotential_name
    return _stencil(self._mode, dataset, (z, z), 0)


@dataclasses.dataclass
class GeostrophicWindSpeed(_GeostrophicWindVariable):
  """Geostrophic wind speed (derived_variables.py:263-276)."""
  _mode: t.ClassVar[str] = 'geostrophic_speed'


class UComponentOfGeostrophicWind(_GeostrophicWindVariable):
  """East-west component of geostrophic wind (derived_variables.py:279-284)."""
  _mode: t.ClassVar[str] = 'geostrophic_u'


class VComponentOfGeostrophicWind(_GeostrophicWindVariable):
  """North-south component of geostrophic wind (derived_variables.py:287-292)."""
  _mode: t.ClassVar[str] = 'geostrophic_v'


@dataclasses.dataclass
class _AgeostrophicWindVariable(_MaterializedVariable):
  """Base class for ageostrophic wind variables: the wind minus the
  geostrophic wind (derived_variables.py:295-310)."""

  u_name: str = 'u_component_of_wind'
  v_name: str = 'v_component_of_wind'
  geopotential_name: str = 'geopotential'
  _mode: t.ClassVar[str] = ''

  @property
  def base_variables(self) -> list:
    return [self.u_name, self.v_name, self.geopotential_name]

  @property
  def core_dims(self):
    lon_lat = ['longitude', 'latitude']
    return (lon_lat, lon_lat, lon_lat), lon_lat

  def compute_on_device(self, dataset):
    z = self.geopotential_name
    lead = 3 if self._mode == 'ageostrophic_v' else 2
    return _stencil(self._mode, dataset, (z, z, self.u_name, self.v_name), lead)


class AgeostrophicWindSpeed(_AgeostrophicWindVariable):
  """Ageostrophic wind speed (derived_variables.py:313-320)."""
  _mode: t.ClassVar[str] = 'ageostrophic_speed'


class UComponentOfAgeostrophicWind(_AgeostrophicWindVariable):
  """East-west component of ageostrophic wind (derived_variables.py:323-329)."""
  _mode: t.ClassVar[str] = 'ageostrophic_u'


class VComponentOfAgeostrophicWind(_AgeostrophicWindVariable):
  """North-south component of ageostrophic wind (derived_variables.py:332-338)."""
  _mode: t.ClassVar[str] = 'ageostrophic_v'


# ---------------------------------------------------------------------------
# Level-column variables (csrc/derived_column.hip)
# ---------------------------------------------------------------------------
_G = 9.81  # (derived_variables.py:357, :384, :419)


def _level_values(dataset: xl.Dataset, dims: tuple, name: str) -> np.ndarray:
  if 'level' not in dims:
    raise ValueError(f"{name}: needs a 'level' dim, has {dims}")
  if 'level' not in dataset.coords:
    raise ValueError(f"{name}: the dataset has no 'level' coordinate")
  level = xl.coord_values(dataset, 'level')
  if level.ndim != 1 or level.dtype.kind not in 'iuf':
    raise ValueError(f"{name}: 'level' must be a 1-D numeric coordinate")
  return level


def _level_range(level: np.ndarray, level_min, level_max) -> tuple:
  """Positions [begin, end) of the inclusive label slice
  `sel(level=slice(level_min, level_max))` on a monotonic coordinate, as
  pandas resolves it: on a decreasing one a bound pair (small, large) selects
  nothing."""
  n = len(level)
  if level_min is None and level_max is None:
    return 0, n
  d = np.diff(level)
  if (d > 0).all():
    begin = 0 if level_min is None else int(np.searchsorted(level, level_min,
                                                            'left'))
    end = n if level_max is None else int(np.searchsorted(level, level_max,
                                                          'right'))
  elif (d < 0).all():
    begin = 0 if level_min is None else int((level > level_min).sum())
    end = n if level_max is None else int((level >= level_max).sum())
  else:
    raise ValueError(
        f'level={level} is not monotonic: what the label slice '
        f'({level_min}, {level_max}) selects on it is not defined here (pass '
        'level_min=None, level_max=None to integrate over every level)')
  return begin, max(begin, end)


class _Columns(t.NamedTuple):
  """Operands of one column launch: dims in `order` = outer dims (with `level`
  at `at`), then `n_inner` dims of contiguous points."""
  tensors: list
  tables: list      # device int64 [n_column * n_level] per operand
  order: tuple
  shape: tuple
  at: int
  n_inner: int
  n_column: int
  n_level: int
  n_point: int
  dtype: torch.dtype
  device: t.Any


def _columns(dataset: xl.Dataset, names: t.Sequence[str],
             spatial_last: bool = False) -> _Columns:
  """The fields `names` laid out for the column kernel, in the dims of the
  first one.  Dims after `level` (two at the most) form the block of points a
  level is read in; every other dim indexes a column slab, read where it lies
  through the slab table.  `level` as the innermost dim is moved to the front
  (a copy).  `spatial_last`: latitude / longitude become the block."""
  device = engine.require_gpu()
  das = [dataset[n] for n in names]
  dims = tuple(das[0].dims)
  for n, da in zip(names, das):
    if set(da.dims) != set(dims):
      raise ValueError(f'{n} {da.dims} and {names[0]} {dims} must have the '
                       'same dims')
  order = dims
  if spatial_last:
    spatial = tuple(d for d in dims if d in ('latitude', 'longitude'))
    order = tuple(d for d in dims if d not in spatial) + spatial
    n_inner = len(spatial)
  else:
    if len(dims) > 1 and dims[-1] == 'level':
      order = ('level',) + dims[:-1]
    n_inner = min(2, len(order) - 1 - order.index('level'))
  at = order.index('level')
  sizes = das[0].sizes
  shape = tuple(sizes[d] for d in order)
  n_outer = len(order) - n_inner
  dtype = operands.float_dtype(*[da.dtype for da in das])
  n_level = shape[at]
  n_point = int(np.prod(shape[n_outer:], dtype=np.int64))
  n_column = int(np.prod(shape[:n_outer], dtype=np.int64)) // max(n_level, 1)
  tensors, tables, seen = [], [], {}
  for n, da in zip(names, das):
    if n not in seen:
      ten, table = (operands.operand(da, order, device, dtype, n_inner)
                    if n_column * n_level * n_point else (None, None))
      if table is None:
        table = np.arange(n_column * n_level, dtype=np.int64)
      # [outer dims] -> [column slab][level]
      table = np.moveaxis(table.reshape(shape[:n_outer]), at, -1)
      seen[n] = (ten, engine.upload_table(np.ascontiguousarray(table).ravel(),
                                          device)
                 if table.size else None)
    tensors.append(seen[n][0])
    tables.append(seen[n][1])
  return _Columns(tensors, tables, order, shape, at, n_inner, n_column,
                  n_level, n_point, dtype, device)


def _spacing(values: np.ndarray, device) -> t.Optional[torch.Tensor]:
  """np.diff in the coordinate's dtype, as a float64 device table."""
  if len(values) < 2:
    return None
  return engine.upload_f64_table(np.diff(values).astype(np.float64), device)


def _without_level(dataset: xl.Dataset, cols: _Columns, out: torch.Tensor,
                   dims: tuple) -> xl.DataArray:
  """[n_column, n_point] -> the operand's dims without `level`."""
  order = tuple(d for d in cols.order if d != 'level')
  out = out.reshape(tuple(n for d, n in zip(cols.order, cols.shape)
                          if d != 'level'))
  dims = tuple(d for d in dims if d != 'level')
  if order != dims:
    out = out.permute(*[order.index(d) for d in dims])
  return xl.DataArray(out, dims, _result_coords(dataset, dims))


def _column_integral(mode: str, dataset: xl.Dataset, names: t.Sequence[str],
                     scale: float, level_min=None, level_max=None,
                     label: str = '') -> xl.DataArray:
  dims = tuple(dataset[names[0]].dims)
  level = _level_values(dataset, dims, label)
  levels = _level_range(level, level_min, level_max)
  if mode == 'eddy' and 'longitude' not in dims:
    raise ValueError(f"{label}: needs a 'longitude' dim, has {dims}")
  cols = _columns(dataset, names, spatial_last=mode == 'eddy')
  out_dtype = operands.float_dtype(cols.dtype, level.dtype)
  if cols.n_column * cols.n_point == 0:
    out = torch.empty((cols.n_column, cols.n_point), dtype=out_dtype,
                      device=cols.device)
    return _without_level(dataset, cols, out, dims)
  means, mean_div = (), 1
  if mode == 'eddy':
    block = cols.order[len(cols.order) - cols.n_inner:]
    lat_rows = block[-1] == 'longitude'
    n_row = cols.shape[-2] if cols.n_inner == 2 else 1
    n_col = cols.shape[-1]
    means = [engine.zonal_mean(x, tab, cols.n_column * cols.n_level, n_row,
                               n_col, lat_rows)
             for x, tab in zip(cols.tensors, cols.tables)]
    mean_div = n_col if lat_rows else 1
  out = engine.derived_column(
      mode, cols.tensors, cols.tables, cols.n_column, cols.n_level,
      cols.n_point, out_dtype=out_dtype, levels=levels,
      spacing=_spacing(level, cols.device), means=means, mean_div=mean_div,
      scale=scale)
  return _without_level(dataset, cols, out, dims)


@dataclasses.dataclass
class VerticalVelocity(_3DWindVariable):
  r"""Vertical wind velocity under the hydrostatic approximation
  (derived_variables.py:179-209): omega = -\int dp div(u, v), scipy's
  `cumulative_trapezoid(-divergence, 100 * level, initial=0)`.  The stencil
  kernel writes the divergence, the column kernel integrates it in place;
  float64 like the divergence."""

  @property
  def core_dims(self):
    zxy = ['level', 'longitude', 'latitude']
    return (zxy, zxy), zxy

  def compute_on_device(self, dataset):
    u_dims = tuple(dataset[self.u_name].dims)
    level = _level_values(dataset, u_dims, 'VerticalVelocity')
    out, order, dims = _stencil_launch('divergence', dataset,
                                       (self.u_name, self.v_name), 0)
    at = order.index('level')
    n_level = out.shape[at]
    n_point = out.shape[-2] * out.shape[-1]
    if out.numel():
      n_column = out.numel() // (n_level * n_point)
      table = np.arange(n_column * n_level, dtype=np.int64).reshape(
          out.shape[:-2])
      table = np.ascontiguousarray(np.moveaxis(table, at, -1)).ravel()
      pascals_per_hpa = 100
      engine.derived_column(
          'cumulative', [], [engine.upload_table(table, out.device)], n_column,
          n_level, n_point, spacing=_spacing(pascals_per_hpa * level,
                                             out.device), out=out)
    if order != dims:
      out = out.permute(*[order.index(d) for d in dims])
    return xl.DataArray(out, dims, _result_coords(dataset, dims))


@dataclasses.dataclass
class EddyKineticEnergy(_3DWindVariable):
  """Eddy kinetic energy (derived_variables.py:212-228): eddies are the
  deviation from the instantaneous zonal mean (which skips NaN, as xarray's
  `mean` does), 1/2 (u'^2 + v'^2) integrated over `level` (in hPa)."""

  @property
  def core_dims(self):
    return (['level', 'longitude'], ['level', 'longitude']), ['longitude']

  def compute_on_device(self, dataset):
    return _column_integral('eddy', dataset, (self.u_name, self.v_name), 1 / 2,
                            label='EddyKineticEnergy')


@dataclasses.dataclass
class LapseRate(_MaterializedVariable):
  """Lapse rate in temperature (derived_variables.py:341-362):
  dT/dp / ((1 / g) dz/dp) with `np.gradient` along `level`, in the fields'
  dtype.  ValueError on a single level, like `np.gradient`."""

  temperature_name: str = 'temperature'
  geopotential_name: str = 'geopotential'

  @property
  def base_variables(self) -> list:
    return [self.temperature_name, self.geopotential_name]

  @property
  def core_dims(self):
    return (['level'], ['level']), ['level']

  def compute_on_device(self, dataset):
    names = (self.temperature_name, self.geopotential_name)
    dims = tuple(dataset[names[0]].dims)
    level = _level_values(dataset, dims, 'LapseRate')
    coef, uniform = plan_lib.gradient_tables(level)
    cols = _columns(dataset, names)
    if cols.n_column * cols.n_point == 0:
      out = torch.empty((cols.n_column, cols.n_level, cols.n_point),
                        dtype=cols.dtype, device=cols.device)
    else:
      out = engine.derived_column(
          'gradient_ratio', cols.tensors, cols.tables, cols.n_column,
          cols.n_level, cols.n_point,
          level_coef=engine.upload_f64_table(coef, cols.device),
          level_uniform=uniform, scale=1 / _G)
    # [column slabs][level][points] -> the temperature's dims
    n_outer = len(cols.order) - cols.n_inner
    outer = tuple(d for d in cols.order[:n_outer] if d != 'level')
    now = outer + ('level',) + cols.order[n_outer:]
    sizes = dict(zip(cols.order, cols.shape))
    out = out.reshape(tuple(sizes[d] for d in now))
    if now != dims:
      out = out.permute(*[now.index(d) for d in dims])
    return xl.DataArray(out, dims, _result_coords(dataset, dims))


@dataclasses.dataclass
class TotalColumnWater(_MaterializedVariable):
  """Total column water (derived_variables.py:365-385): (1 / g) times the
  trapezoid integral of a water species over `level` -- in hPa, as the
  reference has it.  Has the species' dims without `level`."""

  water_species_name: str = 'specific_humidity'

  @property
  def base_variables(self) -> list:
    return [self.water_species_name]

  @property
  def core_dims(self):
    return (['level'],), []

  def compute_on_device(self, dataset):
    return _column_integral('integral', dataset, (self.water_species_name,),
                            1 / _G, label='TotalColumnWater')


@dataclasses.dataclass
class IntegratedWaterTransport(_MaterializedVariable):
  """Integrated horizontal water transport of a column
  (derived_variables.py:388-430): (1 / g) |(trapz(q u), trapz(q v))| over the
  levels of the inclusive label slice [level_min, level_max] (None = open; the
  defaults are the GraphCast paper's).  One selected level, or none, gives 0.0.
  A non-monotonic `level` with a numeric bound is refused (ValueError)."""

  u_name: str = 'u_component_of_wind'
  v_name: str = 'v_component_of_wind'
  water_species_name: str = 'specific_humidity'
  level_min: t.Optional[float] = 300
  level_max: t.Optional[float] = 1000

  @property
  def base_variables(self) -> list:
    return [self.u_name, self.v_name, self.water_species_name]

  @property
  def core_dims(self):
    return (['level'], ['level']), []

  def compute_on_device(self, dataset):
    return _column_integral(
        'transport', dataset,
        (self.water_species_name, self.u_name, self.v_name), 1 / _G,
        self.level_min, self.level_max, label='IntegratedWaterTransport')


# ---------------------------------------------------------------------------
# Lead-time variables (csrc/derived_lead.hip)
# ---------------------------------------------------------------------------
def _lead_window(mode: str, dataset: xl.Dataset, name: str, lead_name: str,
                 window: int, clamp_negative: bool = False) -> xl.DataArray:
  """One launch of the lead-window kernel over the field `name`: the dims
  after `lead_name` form the block of points a lead is read in, the dims
  before it index the outer slabs, read where they lie through the slab table
  (a contiguous tensor needs none).  `lead_name` as the innermost of several
  dims is moved to the front (a copy): `operands.SeriesLayout`.  The result
  has the field's dims."""
  da = dataset[name]
  dims = tuple(da.dims)
  if lead_name not in dims:
    raise ValueError(f'{name}: needs a {lead_name!r} dim, has {dims}')
  device = engine.require_gpu()
  lay = operands.SeriesLayout.of(dims, da.sizes, lead_name)
  dtype = operands.float_dtype(da.dtype)
  n_outer, n_lead, n_point = lay.n_outer, lay.n_series, lay.n_point
  if n_outer * n_lead * n_point == 0:
    out = torch.empty(lay.shape, dtype=dtype, device=device)
  else:
    ten, table = lay.operand(da, device, dtype)
    out = engine.derived_lead_window(mode, ten, table, n_outer, n_lead,
                                     n_point, window, clamp_negative)
  return xl.DataArray(lay.restore(out, (n_lead,)), dims,
                      _result_coords(dataset, dims))


def _whole_steps(numerator, denominator) -> int:
  """derived_variables.py:513-514, :713-717."""
  steps = float(numerator / denominator)
  assert steps.is_integer(), 'Accumulation time must be multiple of timestep.'
  if steps < 1:
    raise ValueError(f'a window of {int(steps)} steps cannot be accumulated')
  return int(steps)


@dataclasses.dataclass
class PrecipitationAccumulation(_MaterializedVariable):
  """Precipitation accumulated over the `accumulation_hours` leading up to and
  including each lead time, from the cumulative `total_precipitation_name`
  (derived_variables.py:471-528): the rolling sum of the lead-to-lead
  differences, NaN where the window is not complete (the first lead included),
  negative sums set to zero unless `set_negative_to_zero` is False.

  Needs the whole lead axis in one chunk; fewer than two leads raise a
  ValueError (the reference fails there with an IndexError)."""

  total_precipitation_name: str
  accumulation_hours: int
  lead_time_name: str = 'prediction_timedelta'
  set_negative_to_zero: bool = True

  @property
  def base_variables(self) -> list:
    return [self.total_precipitation_name]

  @property
  def core_dims(self):
    return ([self.lead_time_name],), [self.lead_time_name]

  def compute_on_device(self, dataset):
    lead_name = self.lead_time_name
    if lead_name not in dataset.coords:
      raise ValueError(
          f'PrecipitationAccumulation: the dataset has no {lead_name!r} '
          'coordinate to take the time step from')
    lead = xl.coord_values(dataset, lead_name)
    if lead.ndim != 1 or lead.size < 2:
      raise ValueError(
          f'PrecipitationAccumulation: {lead_name!r} holds {lead.size} lead '
          'time(s); the variable needs the whole lead axis in one chunk (at '
          'least two leads, equally spaced)')
    timestep = np.diff(lead)
    assert np.all(timestep == timestep[0]), 'All time steps must be equal.'
    steps = _whole_steps(np.timedelta64(self.accumulation_hours, 'h'),
                         timestep[0])
    return _lead_window('diff_sum', dataset, self.total_precipitation_name,
                        lead_name, steps, self.set_negative_to_zero)


@dataclasses.dataclass
class AggregatePrecipitationAccumulation(_MaterializedVariable):
  """A longer accumulation period from existing shorter accumulations
  (derived_variables.py:685-720): the rolling sum of `raw_accumulation_name`
  over accumulation_hours / raw_accumulation_hours leads, NaN where the window
  is not complete.  As in the reference the lead coordinate is not looked
  at."""

  accumulation_hours: int
  raw_accumulation_name: str = 'total_precipitation_6hr'
  raw_accumulation_hours: int = 6
  lead_time_name: str = 'prediction_timedelta'

  @property
  def base_variables(self) -> list:
    return [self.raw_accumulation_name]

  @property
  def core_dims(self):
    return ([self.lead_time_name],), [self.lead_time_name]

  def compute_on_device(self, dataset):
    steps = _whole_steps(np.timedelta64(self.accumulation_hours, 'h'),
                         np.timedelta64(self.raw_accumulation_hours, 'h'))
    return _lead_window('sum', dataset, self.raw_accumulation_name,
                        self.lead_time_name, steps)


# The reference's dictionary of common derived variables
# (derived_variables.py:724-773) without the level-column and the
# precipitation entries, which live in the two dictionaries below.
DERIVED_VARIABLE_DICT = {
    'wind_speed': WindSpeed(
        u_name='u_component_of_wind', v_name='v_component_of_wind'),
    '10m_wind_speed': WindSpeed(
        u_name='10m_u_component_of_wind', v_name='10m_v_component_of_wind'),
    'divergence': WindDivergence(),
    'vorticity': WindVorticity(),
    'geostrophic_wind_speed': GeostrophicWindSpeed(),
    'u_component_of_geostrophic_wind': UComponentOfGeostrophicWind(),
    'v_component_of_geostrophic_wind': VComponentOfGeostrophicWind(),
    'ageostrophic_wind_speed': AgeostrophicWindSpeed(),
    'u_component_of_ageostrophic_wind': UComponentOfAgeostrophicWind(),
    'v_component_of_ageostrophic_wind': VComponentOfAgeostrophicWind(),
    'relative_humidity': RelativeHumidity(),
}

# The level-column entries of the reference's dictionary, with its constructor
# arguments.  They are kept apart from DERIVED_VARIABLE_DICT for now (DESIGN.md
# section 7); a `--derived_variables=` name is resolved in
# ALL_DERIVED_VARIABLES.
COLUMN_VARIABLE_DICT = {
    'vertical_velocity': VerticalVelocity(),
    'eddy_kinetic_energy': EddyKineticEnergy(),
    'lapse_rate': LapseRate(),
    'total_column_vapor': TotalColumnWater(
        water_species_name='specific_humidity'),
    'total_column_liquid': TotalColumnWater(
        water_species_name='specific_cloud_liquid_water_content'),
    'total_column_ice': TotalColumnWater(
        water_species_name='specific_cloud_ice_water_content'),
    'integrated_vapor_transport': IntegratedWaterTransport(),
}

# Both dictionaries in the reference's key order (derived_variables.py:724-752)
_REFERENCE_KEY_ORDER = (
    'wind_speed', '10m_wind_speed', 'divergence', 'vorticity',
    'vertical_velocity', 'eddy_kinetic_energy', 'geostrophic_wind_speed',
    'u_component_of_geostrophic_wind', 'v_component_of_geostrophic_wind',
    'ageostrophic_wind_speed', 'u_component_of_ageostrophic_wind',
    'v_component_of_ageostrophic_wind', 'lapse_rate', 'total_column_vapor',
    'total_column_liquid', 'total_column_ice', 'integrated_vapor_transport',
    'relative_humidity')
ALL_DERIVED_VARIABLES = {
    k: {**DERIVED_VARIABLE_DICT, **COLUMN_VARIABLE_DICT}[k]
    for k in _REFERENCE_KEY_ORDER}
assert len(ALL_DERIVED_VARIABLES) == (len(DERIVED_VARIABLE_DICT)
                                      + len(COLUMN_VARIABLE_DICT))

# The lead-time entries of the reference's dictionary (derived_variables.py:
# 753-772), with its constructor arguments.  They need the whole lead axis in
# one chunk, so they stay out of ALL_DERIVED_VARIABLES, whose entries all act
# inside an `init_time=1,lead_time=1` chunk.
LEAD_VARIABLE_DICT = {
    'total_precipitation_6hr': PrecipitationAccumulation(
        total_precipitation_name='total_precipitation',
        accumulation_hours=6,
        lead_time_name='prediction_timedelta'),
    'total_precipitation_24hr': PrecipitationAccumulation(
        total_precipitation_name='total_precipitation',
        accumulation_hours=24,
        lead_time_name='prediction_timedelta'),
    'total_precipitation_24hr_from_6hr': AggregatePrecipitationAccumulation(
        accumulation_hours=24,
        lead_time_name='prediction_timedelta'),
    'total_precipitation_24hr_from_12hr': AggregatePrecipitationAccumulation(
        accumulation_hours=24,
        lead_time_name='prediction_timedelta',
        raw_accumulation_name='total_precipitation_12hr',
        raw_accumulation_hours=12),
}

# Every key of the reference's dictionary, in its order, with the objects of
# the three family dictionaries: what a `--derived_variables=` name may be
# resolved in.
REFERENCE_DERIVED_VARIABLES = {**ALL_DERIVED_VARIABLES, **LEAD_VARIABLE_DICT}
assert len(REFERENCE_DERIVED_VARIABLES) == 22


def zonal_energy_spectrum_area_mean(dataset, variable_name: str) -> xl.DataArray:
  """Area-weighted latitude mean of `ZonalEnergySpectrum(variable_name)`:
  sum_lat w(lat) S(..., lat, k) / sum_lat w(lat), w = the latitude weights of
  metrics.py:35-60 -- BASELINE configs[3] ("zonal energy spectrum + lat-weighted
  reduce").  The reference has no such function (it averages spectra in
  notebooks); here it is ONE kernel for float32 0.25 / 0.5-degree rows: the
  per-latitude spectra are reduced in registers and never written
  (engine.zonal_spectrum_lat_mean).  Result dims: the variable's dims without
  latitude / longitude, plus `zonal_wavenumber` last."""
  from weatherbench2_amd import plan as plan_lib
  if xl.is_xarray(dataset):
    return xl.like_input(
        zonal_energy_spectrum_area_mean(xl.as_dataset(dataset), variable_name),
        dataset)
  dataset = xl.as_dataset(dataset)
  zes = ZonalEnergySpectrum(variable_name)
  zes.lon_spacing_m(dataset)  # same uniform-spacing check as the spectrum itself
  da = dataset[variable_name]
  for d in ('latitude', 'longitude'):
    if d not in da.dims:
      raise ValueError(f'{d!r} missing from {da.dims}')
  rest = tuple(d for d in da.dims if d not in ('latitude', 'longitude'))
  order = rest + ('latitude', 'longitude')
  moved = da if da.dims == order else da.transpose(*order)
  device = engine.require_gpu()
  x = engine.as_device_tensor(moved.data, device)
  if x.dtype not in (torch.float32, torch.float64):
    x = x.to(torch.float64)
  latitude = np.asarray(dataset.coords['latitude'])
  n_bins = len(np.asarray(dataset.coords['longitude'])) // 2 + 1
  circ = torch.as_tensor(zes._circumference(latitude).astype(np.float64)
                         ).to(device)
  w_host = np.asarray(plan_lib.get_lat_weights(latitude), dtype=np.float64)
  w = torch.as_tensor(w_host).to(device)
  out = engine.zonal_spectrum_lat_mean(x.contiguous(), circ, w, len(latitude),
                                       weight_sum=float(np.sum(w_host)))
  coords = {k: v for k, v in dataset.coords.items()
            if k not in ('longitude', 'latitude')
            and not (isinstance(v, xl.DataArray)
                     and ({'longitude', 'latitude'} & set(v.dims)))}
  coords['zonal_wavenumber'] = np.arange(n_bins)
  return xl.DataArray(feeder.download(out), rest + ('zonal_wavenumber',), coords,
                      variable_name)


def interpolate_spectral_frequencies(
    spectrum: xl.DataArray,
    wavenumber_dim: str,
    frequencies: t.Optional[t.Sequence[float]] = None,
    method: str = 'linear',
) -> xl.DataArray:
  """Interpolate frequencies in `spectrum` to common values
  (derived_variables.py:629-683).

  `spectrum` is what ZonalEnergySpectrum.compute returns: its `frequency`
  coordinate depends on latitude (the circles shrink towards the poles), so
  spectra of different latitudes are only comparable after this step.  Host
  post-processing of an already reduced result: linear interpolation per
  latitude, NaN outside that latitude's frequency range (xarray's `interp`
  default), `frequency` replaces `wavenumber_dim` in place.
  """
  if method != 'linear':
    raise NotImplementedError("only method='linear' is implemented")
  freq = spectrum.coords.get('frequency')
  if not isinstance(freq, xl.DataArray) or set(freq.dims) != {
      wavenumber_dim, 'latitude'}:
    raise ValueError(
        f'spectrum.frequency.dims={getattr(freq, "dims", None)} was not a '
        f'permutation of ("{wavenumber_dim}", "latitude")')
  fr = np.asarray(freq.transpose(wavenumber_dim, 'latitude').values)
  if frequencies is None:
    freq_min = fr.max(axis=1).min()
    freq_max = fr.min(axis=1).max()
    frequencies = np.linspace(freq_min, freq_max,
                              num=spectrum.sizes[wavenumber_dim])
  if isinstance(frequencies, xl.DataArray):
    frequencies = frequencies.values
  frequencies = np.asarray(frequencies, dtype=np.float64)
  if frequencies.ndim != 1:
    raise ValueError(f'Expected 1-D frequencies, found {frequencies.shape=}')
  ax_w = spectrum.dims.index(wavenumber_dim)
  ax_l = spectrum.dims.index('latitude')
  values = np.moveaxis(np.asarray(spectrum.values), (ax_l, ax_w), (-2, -1))
  out = np.empty(values.shape[:-1] + (len(frequencies),), dtype=np.float64)
  flat_in = values.reshape(-1, values.shape[-2], values.shape[-1])
  flat_out = out.reshape(-1, values.shape[-2], len(frequencies))
  for j in range(values.shape[-2]):
    xp = fr[:, j]
    for i in range(flat_in.shape[0]):
      flat_out[i, j] = np.interp(frequencies, xp, flat_in[i, j],
                                 left=np.nan, right=np.nan)
  out = np.moveaxis(out, (-2, -1), (ax_l, ax_w))
  dims = tuple('frequency' if d == wavenumber_dim else d
               for d in spectrum.dims)
  coords = {k: v for k, v in spectrum.coords.items()
            if k not in (wavenumber_dim, 'frequency', 'wavelength')}
  coords['frequency'] = frequencies
  with np.errstate(divide='ignore'):
    # interp does not deal well with the infinite wavelength: reset it (:676)
    coords['wavelength'] = xl.DataArray(1 / frequencies, ('frequency',))
  return xl.DataArray(out, dims, coords, spectrum.name)
