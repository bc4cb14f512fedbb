"""Horizontal regridding on the MI355X: the public surface of the reference's
weatherbench2/regridding.py (nearest neighbour, bilinear, first-order
conservative; rectilinear grids, irregular spacing allowed).

The weights are host NumPy in float64 and banded; the field never leaves the
device: csrc/regrid.hip (K11 of include/wb2hip.h) reads every slab where it
lies -- a contiguous tensor, a strided view of whole slabs, a gather and a
decreasing latitude axis differ in the tables alone -- in (lat, lon) or
(lon, lat) layout, and writes the result in the same layout.

What differs from the reference on purpose:
  * dtype: float32 in -> float32 out, float64 in -> float64 out, integers and
    bool are computed as float64 by the bilinear and conservative regridders;
    the nearest regridder keeps the input dtype.  All arithmetic is float64.
    (The reference under jax's default demotes everything to float32.)
  * +-inf reaches only the target cells it overlaps (the reference's dense
    contraction turns it into NaN for every other cell of the slab: 0 * inf).
  * a bilinear target node that coincides with a source node takes that
    node's value even where the neighbour is NaN (what np.interp does).
  * the nearest-neighbour table is an exact brute-force search (no BallTree):
    ties go to the lowest source index, see `nearest_neighbor_indices`.
"""
from __future__ import annotations

import dataclasses
import enum
import functools
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import feeder
from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

Array = t.Union[np.ndarray, torch.Tensor]


class LongitudeScheme(enum.Enum):
  START_AT_ZERO = enum.auto()   # [0, d, 2d, ..., 360 - d]
  CENTER_AT_ZERO = enum.auto()  # [-180 + d/2, ..., 180 - d/2]


class LatitudeSpacing(enum.Enum):
  EQUIANGULAR_WITH_POLES = enum.auto()
  EQUIANGULAR_WITHOUT_POLES = enum.auto()
  CUSTOM = enum.auto()  # e.g. Gaussian grids


def latitude_values(latitude_spacing: LatitudeSpacing, num: int) -> np.ndarray:
  """Latitude node values given spacing and number of nodes."""
  if latitude_spacing == LatitudeSpacing.EQUIANGULAR_WITH_POLES:
    start, stop = -90, 90
  elif latitude_spacing == LatitudeSpacing.EQUIANGULAR_WITHOUT_POLES:
    start = -90 + 0.5 * 180 / num
    stop = 90 - 0.5 * 180 / num
  else:
    raise ValueError(f'Unhandled {latitude_spacing=}')
  return np.linspace(start, stop, num=num)


def longitude_values(longitude_scheme: LongitudeScheme, num: int) -> np.ndarray:
  """Longitude node values given scheme and number of nodes."""
  delta = 360 / num
  if longitude_scheme == LongitudeScheme.START_AT_ZERO:
    start, stop = 0, 360 - delta
  elif longitude_scheme == LongitudeScheme.CENTER_AT_ZERO:
    start, stop = -180 + delta / 2, 180 - delta / 2
  else:
    raise ValueError(f'Unhandled {longitude_scheme=}')
  return np.linspace(start, stop, num=num)


def _assert_increasing(x: np.ndarray) -> None:
  if not (np.diff(x) > 0).all():
    raise ValueError(f'array is not increasing: {x}')


@dataclasses.dataclass(frozen=True)
class Grid:
  """A rectilinear grid: 1-D longitudes and (increasing) latitudes in degrees,
  whether longitude is periodic and whether the grid covers the poles."""

  longitudes: np.ndarray = dataclasses.field(kw_only=True)
  latitudes: np.ndarray = dataclasses.field(kw_only=True)
  periodic: bool = dataclasses.field(kw_only=True)
  includes_poles: bool = dataclasses.field(kw_only=True)

  def __post_init__(self):
    _assert_increasing(self.latitudes)

  @property
  def lat(self):
    raise AttributeError(
        'lat/lon attributes (in radians) is no longer supported. '
        'Use latitude/longitude (in degrees) instead')

  @property
  def lon(self):
    raise AttributeError(
        'lat/lon attributes (in radians) is no longer supported. '
        'Use latitude/longitude (in degrees) instead')

  @classmethod
  def from_degrees(cls, lon: np.ndarray, lat: np.ndarray) -> 'Grid':
    """Legacy constructor."""
    return cls(longitudes=lon, latitudes=lat, periodic=True,
               includes_poles=True)

  @property
  def shape(self) -> tuple:
    return (len(self.longitudes), len(self.latitudes))

  def _to_tuple(self) -> tuple:
    return (tuple(np.asarray(self.longitudes).tolist()),
            tuple(np.asarray(self.latitudes).tolist()),
            self.periodic, self.includes_poles)

  def __eq__(self, other):
    return isinstance(other, Grid) and self._to_tuple() == other._to_tuple()

  def __hash__(self):
    return hash(self._to_tuple())


# ---------------------------------------------------------------------------
# Conservative weights (host, float64, dense (target, source))
# ---------------------------------------------------------------------------
def _latitude_cell_bounds(x, include_poles: bool = True) -> np.ndarray:
  x = np.asarray(x)
  if include_poles:
    first, last = np.array([-90]), np.array([90])
  else:
    first = x[:1] - (x[1] - x[0]) / 2
    last = x[-1:] + (x[-1] - x[-2]) / 2
  return np.concatenate([first, (x[:-1] + x[1:]) / 2, last])


def _latitude_area_from_bounds(lower, upper) -> np.ndarray:
  # the integral of cos(latitude) between the bounds
  return np.sin(np.deg2rad(upper)) - np.sin(np.deg2rad(lower))


def _latitude_area(points, include_poles: bool) -> np.ndarray:
  bounds = _latitude_cell_bounds(points, include_poles)
  return _latitude_area_from_bounds(bounds[:-1], bounds[1:])


def _conservative_latitude_weights(source_points, target_points,
                                   source_includes_poles: bool,
                                   target_includes_poles: bool) -> np.ndarray:
  """(target, source) weights of the area overlap along latitude; rows sum to
  one.  Where the source does not reach the poles, a target cell whose overlap
  is not its own area (to rtol 1e-3) is uncovered: its row is NaN."""
  source_points = np.asarray(source_points)
  target_points = np.asarray(target_points)
  _assert_increasing(source_points)
  _assert_increasing(target_points)
  sb = _latitude_cell_bounds(source_points, source_includes_poles)
  tb = _latitude_cell_bounds(target_points, target_includes_poles)
  upper = np.minimum(tb[1:, np.newaxis], sb[np.newaxis, 1:])
  lower = np.maximum(tb[:-1, np.newaxis], sb[np.newaxis, :-1])
  overlap = (upper > lower) * _latitude_area_from_bounds(lower, upper)
  coverage = np.sum(overlap, axis=1, keepdims=True)
  with np.errstate(invalid='ignore', divide='ignore'):
    weights = overlap / coverage
  if not source_includes_poles:
    areas = _latitude_area(target_points, target_includes_poles)[:, np.newaxis]
    weights = np.where(np.isclose(coverage, areas, rtol=1e-3), weights, np.nan)
  assert weights.shape == (target_points.size, source_points.size)
  return weights


def _align_phase_with(x, target, period):
  """`x` shifted by a whole `period` up or down, or not at all, whichever is
  nearest to `target`."""
  if period is None:
    return x
  shift_down = x > target + period / 2
  shift_up = x < target - period / 2
  return x + period * shift_up - period * shift_down


def _periodic_upper_lower_bounds(x, period) -> tuple:
  """Cell bounds half-way to the neighbours; the end cells are extrapolated
  (period None) or wrap."""
  x = np.asarray(x)
  if period is None:
    nxt = np.concatenate([x[1:], x[-1:] + (x[-1] - x[-2])])
    prv = np.concatenate([x[:1] - (x[1] - x[0]), x[:-1]])
  else:
    x = x % period
    nxt = _align_phase_with(np.roll(x, -1), x, period)
    prv = _align_phase_with(np.roll(x, +1), x, period)
  return (x + nxt) / 2, (prv + x) / 2


def _longitude_length(points, periodic: bool) -> np.ndarray:
  upper, lower = _periodic_upper_lower_bounds(points, 360 if periodic else None)
  return upper - lower


def _conservative_longitude_weights(source_points, target_points,
                                    source_periodic: bool,
                                    target_periodic: bool) -> np.ndarray:
  """(target, source) weights of the overlap of the cells along longitude
  (intervals on the circle, none longer than half of it); rows sum to one.
  Where the source is not periodic, a target cell whose overlap is not its own
  length (to rtol 1e-3) is uncovered: its row is NaN."""
  source_points = np.asarray(source_points)
  target_points = np.asarray(target_points)
  if len(target_points) < 3 and target_periodic:
    raise ValueError(
        'Need 3 or more target points else overlap is not well defined. Found'
        f' {len(target_points)}')
  _assert_increasing(source_points)
  _assert_increasing(target_points)
  t_up, t_lo = _periodic_upper_lower_bounds(
      target_points, 360 if target_periodic else None)
  s_up, s_lo = _periodic_upper_lower_bounds(
      source_points, 360 if source_periodic else None)
  x0, x1 = t_lo[:, np.newaxis], t_up[:, np.newaxis]
  y0 = _align_phase_with(s_lo[np.newaxis, :], x0, 360)
  y1 = _align_phase_with(s_up[np.newaxis, :], x0, 360)
  overlap = np.maximum(np.minimum(x1, y1) - np.maximum(x0, y0), 0)
  coverage = np.sum(overlap, axis=1, keepdims=True)
  with np.errstate(invalid='ignore', divide='ignore'):
    weights = overlap / coverage
  if not source_periodic:
    lengths = _longitude_length(target_points, target_periodic)[:, np.newaxis]
    weights = np.where(np.isclose(coverage, lengths, rtol=1e-3), weights,
                       np.nan)
  assert weights.shape == (target_points.size, source_points.size)
  return weights


# ---------------------------------------------------------------------------
# The per-axis tables of K11 (include/wb2hip.h)
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class AxisTable:
  """One axis of wb2_regrid_separable: entries ptr[k] .. ptr[k + 1] of `idx`
  and `w` belong to target index k; `nan[k]` marks an uncovered one."""
  ptr: np.ndarray  # int32[n_target + 1]
  idx: np.ndarray  # int32[ptr[-1]]
  w: np.ndarray    # float64[ptr[-1]]
  nan: np.ndarray  # uint8[n_target]

  @property
  def longest(self) -> int:
    return int(np.diff(self.ptr).max()) if len(self.ptr) > 1 else 0


def csr_from_dense(weights: np.ndarray, wrap: bool = False) -> AxisTable:
  """The entries with w != 0 of a dense (target, source) matrix, row by row; a
  row that holds a NaN is uncovered and has no entries.  Entries are in
  ascending source index; with `wrap` (longitude of a periodic source) a band
  that runs over the seam starts behind its largest gap, so that it is in
  ascending position within the band."""
  weights = np.asarray(weights, dtype=np.float64)
  n_target, n_source = weights.shape
  ptr, idx, w, nan = [0], [], [], np.zeros(n_target, dtype=np.uint8)
  for k in range(n_target):
    row = weights[k]
    if np.isnan(row).any():
      nan[k] = 1
    else:
      at = np.flatnonzero(row != 0)
      if wrap and at.size > 1:
        gaps = np.diff(at)
        if gaps.max() > at[0] + n_source - at[-1]:
          at = np.roll(at, -(int(np.argmax(gaps)) + 1))
      idx.extend(at.tolist())
      w.extend(row[at].tolist())
    ptr.append(len(idx))
  return AxisTable(np.asarray(ptr, dtype=np.int32),
                   np.asarray(idx, dtype=np.int32),
                   np.asarray(w, dtype=np.float64), nan)


def linear_taps(source_points, target_points, clamp: bool,
                period: t.Optional[float] = None) -> AxisTable:
  """np.interp as two taps per target point: idx = (i0, i1), w = (t, 0) with
  the value f[i0] + t * (f[i1] - f[i0]); t == 0 (i1 == i0) where the point
  coincides with a node, and where it lies outside a clamped axis (`clamp`:
  the ends' values, as np.interp's default; otherwise uncovered, as
  left = right = NaN).  With `period` the points are taken modulo the period
  and the axis wraps (np.interp's `period`)."""
  xp = np.asarray(source_points, dtype=np.float64)
  x = np.asarray(target_points, dtype=np.float64)
  index = np.arange(len(xp))
  if period is not None:
    x, xp = x % period, xp % period
    order = np.argsort(xp)
    xp, index = xp[order], index[order]
    xp = np.concatenate([xp[-1:] - period, xp, xp[:1] + period])
    index = np.concatenate([index[-1:], index, index[:1]])
  n = len(xp)
  idx = np.zeros((len(x), 2), dtype=np.int32)
  w = np.zeros((len(x), 2), dtype=np.float64)
  nan = np.zeros(len(x), dtype=np.uint8)
  for k, v in enumerate(x):
    if v < xp[0] or v > xp[-1]:
      if clamp:
        idx[k] = index[0 if v < xp[0] else n - 1]
      else:
        nan[k] = 1
      continue
    j = int(np.searchsorted(xp, v, side='right')) - 1
    if j == n - 1 or xp[j] == v:
      idx[k] = index[j]
    else:
      idx[k] = index[j], index[j + 1]
      w[k, 0] = (v - xp[j]) / (xp[j + 1] - xp[j])
  return AxisTable(np.arange(len(x) + 1, dtype=np.int32) * 2, idx.ravel(),
                   w.ravel(), nan)


def _haversine(lat_a, lat_b, dlon):
  a = (np.sin((lat_a - lat_b) / 2) ** 2
       + np.cos(lat_a) * np.cos(lat_b) * np.sin(dlon / 2) ** 2)
  return 2 * np.arcsin(np.sqrt(a))


def nearest_neighbor_indices(source_grid: Grid, target_grid: Grid) -> np.ndarray:
  """Flat indices into the raveled (lon, lat) source of the haversine-nearest
  source node of every target node, in raveled (lon, lat) target order.

  Exact brute force in float64.  On a rectilinear grid the distance grows
  with sin^2(dlon / 2) whatever the latitudes are, so the nearest longitude is
  found once per target longitude and the latitude then among the nodes of
  that meridian.  Ties go to the lowest index: the lowest longitude index
  among equal sin^2(dlon / 2), then the lowest latitude index among equal
  distances."""
  s_lat = np.deg2rad(np.asarray(source_grid.latitudes, dtype=np.float64))
  s_lon = np.deg2rad(np.asarray(source_grid.longitudes, dtype=np.float64))
  t_lat = np.deg2rad(np.asarray(target_grid.latitudes, dtype=np.float64))
  t_lon = np.deg2rad(np.asarray(target_grid.longitudes, dtype=np.float64))
  dlon = t_lon[:, np.newaxis] - s_lon[np.newaxis, :]
  lon_index = np.argmin(np.sin(dlon / 2) ** 2, axis=1)
  out = np.empty((len(t_lon), len(t_lat)), dtype=np.int64)
  for a, b in enumerate(lon_index):
    dist = _haversine(t_lat[:, np.newaxis], s_lat[np.newaxis, :], dlon[a, b])
    out[a] = b * len(s_lat) + np.argmin(dist, axis=1)
  return out.ravel()


# ---------------------------------------------------------------------------
# Regridders
# ---------------------------------------------------------------------------
_HORIZONTAL = ('longitude', 'latitude')


def _flip(table: AxisTable, n_source: int) -> AxisTable:
  """The same table for a source axis stored in reverse."""
  return AxisTable(table.ptr, (n_source - 1 - table.idx).astype(np.int32),
                   table.w, table.nan)


@dataclasses.dataclass(frozen=True)
class Regridder:
  """Base class for regridding."""

  source: Grid
  target: Grid

  # -- what a subclass provides ---------------------------------------------
  def _device_regrid(self, x: torch.Tensor, slab, n_slab: int, lat_rows: bool,
                     lat_reversed: bool) -> torch.Tensor:
    """[n_slab, target slab] from the slabs of `x` (float32 / float64 for the
    separable regridders), in the layout of the input."""
    raise NotImplementedError

  def _compute_dtype(self, dtype: torch.dtype) -> torch.dtype:
    return dtype if dtype in (torch.float32, torch.float64) else torch.float64

  # -- shared plumbing --------------------------------------------------------
  def _cache(self) -> dict:
    return self.__dict__.setdefault('_device_tables', {})

  def _run(self, x: torch.Tensor, lat_rows: bool, lat_reversed: bool = False,
           table=None, outer=None) -> torch.Tensor:
    """`x`: (..., lat, lon) when lat_rows else (..., lon, lat), on the device,
    in its compute dtype; `table` its slab table and `outer` the leading
    shape where the slabs are picked from `x` (a view, a gather)."""
    n_lon, n_lat = self.source.shape
    want = (n_lat, n_lon) if lat_rows else (n_lon, n_lat)
    if tuple(x.shape[-2:]) != want:
      raise ValueError(f'expected {tuple(x.shape)=} to end in the source '
                       f'grid\'s {want}')
    outer = tuple(x.shape[:-2]) if outer is None else tuple(outer)
    if table is None and not x.is_contiguous():
      table = operands.stride_table(x, 2)
      if table is None:
        x = x.contiguous()
    n_slab = int(np.prod(outer, dtype=np.int64))
    slab = operands.table_tensor(table, x.device)
    out = self._device_regrid(x, slab, n_slab, lat_rows, lat_reversed)
    t_lon, t_lat = self.target.shape
    return out.reshape(outer + ((t_lat, t_lon) if lat_rows else (t_lon, t_lat)))

  def regrid_array(self, field: Array) -> Array:
    """Regrid an array with dimensions (..., lon, lat) from source to target:
    a device tensor stays on the device, a NumPy array (or a host tensor)
    comes back as NumPy (a host tensor)."""
    shape = tuple(np.shape(field))
    if shape[-2:] != self.source.shape:
      raise ValueError(f'expected {shape=} to match {self.source.shape=}')
    device = engine.require_gpu()
    on_device = isinstance(field, torch.Tensor) and field.is_cuda
    if on_device:
      x = field
    else:
      x = engine.as_device_tensor(
          field.numpy() if isinstance(field, torch.Tensor) else
          np.asarray(field), device)
    dtype = self._compute_dtype(x.dtype)
    out = self._run(x if x.dtype == dtype else x.to(dtype), lat_rows=False)
    if on_device:
      return out
    engine.order_read(out)
    host = feeder.download(out)
    return torch.from_numpy(host) if isinstance(field, torch.Tensor) else host

  def regrid_dataset(self, dataset):
    """Regrid a Dataset (xarray_lite, or xarray where present) from source to
    target.  A decreasing latitude is read in reverse; the result carries the
    target's coordinates and every variable keeps its own dimension order;
    variables without both horizontal dims pass through unchanged.  Device
    data stays on the device, host data comes back on the host."""
    if xl.is_xarray(dataset):
      return xl.like_input(self.regrid_dataset(xl.as_dataset(dataset)), dataset)
    ds = xl.as_dataset(dataset)
    lat = xl.coord_values(ds, 'latitude')
    reverse = not (np.diff(lat) > 0).all()
    if reverse:
      _assert_increasing(lat[::-1])
    coords = xl.coords_without(ds.coords, _HORIZONTAL)
    coords['latitude'] = np.asarray(self.target.latitudes)
    coords['longitude'] = np.asarray(self.target.longitudes)
    out = xl.Dataset(coords=coords, attrs=dict(ds.attrs))
    device = None
    for name, da in ds.data_vars.items():
      if not all(d in da.dims for d in _HORIZONTAL):
        out.data_vars[name] = xl.DataArray(
            da.data, da.dims, {k: v for k, v in coords.items()
                               if k not in _HORIZONTAL}, name)
        continue
      device = device or engine.require_gpu()
      pair = tuple(d for d in da.dims if d in _HORIZONTAL)
      order = tuple(d for d in da.dims if d not in _HORIZONTAL) + pair
      dtype = self._compute_dtype(operands.torch_dtype(da.dtype))
      x, table = operands.operand(da, order, device, dtype, 2)
      res = self._run(x, lat_rows=pair[0] == 'latitude', lat_reversed=reverse,
                      table=table,
                      outer=tuple(da.sizes[d] for d in order[:-2]))
      res_da = xl.DataArray(res, order, coords, name)
      if order != da.dims:
        res_da = res_da.transpose(*da.dims)
      if not operands.on_device(da.data):
        engine.order_read(res_da.data)
        res_da = xl.DataArray(feeder.download(res_da.data.contiguous()),
                              da.dims, coords, name)
      out.data_vars[name] = xl.DataArray(res_da.data, da.dims, coords, name)
    return out


class _SeparableRegridder(Regridder):
  """Regridders that act on each axis in turn (wb2_regrid_separable)."""

  _MODE = None

  def _axis_tables(self) -> tuple:
    """(longitude table, latitude table) for an increasing source latitude."""
    raise NotImplementedError

  @functools.cached_property
  def axis_tables(self) -> tuple:
    return self._axis_tables()

  def _tables_on(self, device, lat_reversed: bool) -> tuple:
    key = (str(device), bool(lat_reversed))
    cache = self._cache()
    if key not in cache:
      lon, lat = self.axis_tables
      if lat_reversed:
        lat = _flip(lat, self.source.shape[1])
      up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
      cache[key] = tuple(up(a) for tab in (lon, lat)
                         for a in (tab.ptr, tab.idx, tab.w, tab.nan))
    return cache[key]

  def _device_regrid(self, x, slab, n_slab, lat_rows, lat_reversed):
    tables = self._tables_on(x.device, lat_reversed)
    return engine.regrid_separable(self._MODE, x, slab, n_slab, lat_rows,
                                   self.source.shape, self.target.shape,
                                   tables)


class ConservativeRegridder(_SeparableRegridder):
  """Regrid with linear conservative regridding: the area-weighted mean of the
  source cells a target cell overlaps, NaNs skipped as np.nanmean does (NaN
  where nothing else is left)."""

  _MODE = 'nanmean'

  @functools.cached_property
  def weights(self) -> tuple:
    """The dense (target, source) matrices: (longitude, latitude)."""
    return (_conservative_longitude_weights(
        self.source.longitudes, self.target.longitudes, self.source.periodic,
        self.target.periodic), _conservative_latitude_weights(
            self.source.latitudes, self.target.latitudes,
            self.source.includes_poles, self.target.includes_poles))

  def _axis_tables(self):
    lon, lat = self.weights
    return (csr_from_dense(lon, wrap=bool(self.source.periodic)),
            csr_from_dense(lat))


class BilinearRegridder(_SeparableRegridder):
  """Regrid with bilinear interpolation: latitude first (clamped at the poles
  when the source includes them, NaN outside otherwise), then longitude
  (wrapping for a periodic source, NaN outside otherwise)."""

  _MODE = 'linear'

  def _axis_tables(self):
    return (linear_taps(self.source.longitudes, self.target.longitudes,
                        clamp=False,
                        period=360 if self.source.periodic else None),
            linear_taps(self.source.latitudes, self.target.latitudes,
                        clamp=bool(self.source.includes_poles)))


class NearestRegridder(Regridder):
  """Regrid with nearest neighbor interpolation (a gather: any dtype of 1, 2,
  4 or 8 bytes per element)."""

  @functools.cached_property
  def indices(self) -> np.ndarray:
    """Flat indices into the raveled (lon, lat) source, per raveled (lon, lat)
    target node."""
    return nearest_neighbor_indices(self.source, self.target)

  def _compute_dtype(self, dtype):
    return dtype

  def _index_on(self, device, lat_rows: bool, lat_reversed: bool):
    key = (str(device), bool(lat_rows), bool(lat_reversed))
    cache = self._cache()
    if key not in cache:
      n_lon, n_lat = self.source.shape
      b, d = np.divmod(self.indices.reshape(self.target.shape), n_lat)
      if lat_reversed:
        d = n_lat - 1 - d
      index = (d * n_lon + b).T if lat_rows else b * n_lat + d
      cache[key] = torch.from_numpy(
          np.ascontiguousarray(index, dtype=np.int32).ravel()).to(device)
    return cache[key]

  def _device_regrid(self, x, slab, n_slab, lat_rows, lat_reversed):
    n_lon, n_lat = self.source.shape
    return engine.regrid_gather(
        x, slab, n_slab, n_lon * n_lat,
        self._index_on(x.device, lat_rows, lat_reversed))
