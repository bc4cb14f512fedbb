"""Pooled verification: any metric of this package on box-pooled fields.

Point scores punish a displaced feature twice.  `neighborhood.FractionsTable`
removes that double penalty for threshold events only.  Here the FIELDS are
aggregated first -- "upscaling" in the neighbourhood-verification literature
(Ebert 2008), the average- and max-pooled CRPS over a ladder of scales of ML
ensemble evaluation (Price et al. 2025) -- and any `Metric` scores the pooled
forecast against the pooled truth.  The reference has no counterpart.

One slab is (latitude, longitude) with n_row x n_col points and an odd window
n = 2 h + 1 in GRID POINTS, the window of `neighborhood.py`: for centre (i, j)
the rows r0 = max(0, i - h) .. r1 = min(n_row - 1, i + h) (clipped at the
poles) and the columns (j - h .. j + h) mod n_col (longitude is cyclic), N_i =
n (r1 - r0 + 1) points.

pooling='mean'.  float64 after an exact widening, in ONE fixed order:

  H[r][j] = the sequential chain s = s + x[r][(j + d) mod n_col] over the
            offsets d = -h, ..., +h in that order, started from the first term
  V[i][j] = the sequential chain of H[r][j] over r = r0 .. r1, increasing
  result  = V / float(N_i), rounded once to the input dtype

No fused multiply-add.  NaN and +-inf follow IEEE: a window that holds a NaN
is NaN, nothing is special-cased (no NaN-skipping pooling); the payload and
sign of a NaN are not pinned.

pooling='max'.  The input dtype, the same two passes with

  m = first; for each next v: m = v if (v > m or v != v) else m

A NaN propagates; the sign of a zero result is that of the first zero met.

n = 1 returns the input's values (-0.0 stays -0.0).  Running or prefix sums
round differently and are not used on either path: K22 (csrc/pool.hip:
`engine.pool_fields`) pools device-backed float32 / float64 variables,
`host_pool` walks the same chains in NumPy for host ones, and the two agree
bit for bit.

Limits (ValueError before any launch): `pooling` 'mean' or 'max'; windows
odd, 1..255, at most n_col, no duplicates (`neighborhood._check_windows`) and
at most the kernel's `max_window` (its halo must fit the LDS: 123 for float32,
87 for float64 -- on either path, so that a result does not depend on where
the data lies); a cyclic longitude axis; float32 and float64.  The kernel
takes (latitude, longitude) slabs: **a (longitude, latitude) variable costs
one transposing device copy on the way in and one on the way out.**  Windows
in kilometres, strided pooling and masked pooling are out of scope.
"""
from __future__ import annotations

import dataclasses
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import events
from weatherbench2_amd import metrics as _m
from weatherbench2_amd import neighborhood as _nb
from weatherbench2_amd import plan as plan_lib
from weatherbench2_amd import threshold_weighted as _tw
from weatherbench2_amd import xarray_lite as xl

NEIGHBORHOOD = _nb.NEIGHBORHOOD
POOLINGS = ('mean', 'max')
_SPATIAL = ('latitude', 'longitude')


# ---------------------------------------------------------------------------
# the host path: the same chains
# ---------------------------------------------------------------------------
def _step(kind: str, m: np.ndarray, v: np.ndarray) -> np.ndarray:
  if kind == 'mean':
    return m + v
  return np.where((v > m) | (v != v), v, m)


def host_pool(x: np.ndarray, windows, kind: str = 'mean') -> np.ndarray:
  """`engine.pool_fields` in NumPy: [n_window, ..., n_row, n_col] in the dtype
  of the float32 / float64 array `x` [..., n_row, n_col], the chains of the
  module docstring in the same order."""
  x = np.asarray(x)
  n_row, n_col = x.shape[-2:]
  work = x.astype(np.float64) if kind == 'mean' else x
  out = np.empty((len(windows),) + x.shape, dtype=x.dtype)
  rows = np.arange(n_row)
  with np.errstate(all='ignore'):
    for wi, n in enumerate(windows):
      h = int(n) // 2
      # np.roll(a, -d)[j] = a[(j + d) mod n_col]
      hor = np.roll(work, h, axis=-1)
      for d in range(-h + 1, h + 1):
        hor = _step(kind, hor, np.roll(work, -d, axis=-1))
      ver = np.zeros_like(hor)
      started = np.zeros(n_row, dtype=bool)
      for k in range(n):
        r = rows - h + k
        ok = (r >= 0) & (r < n_row)
        term = hor[..., np.clip(r, 0, n_row - 1), :]
        nxt = _step(kind, ver, term)
        first = (ok & ~started)[:, None]
        ver = np.where(first, term, np.where((ok & started)[:, None], nxt,
                                             ver))
        started |= ok
      if kind == 'mean':
        count = (n * (np.minimum(rows + h, n_row - 1) -
                      np.maximum(rows - h, 0) + 1)).astype(np.float64)
        ver = ver / count[:, None]
      out[wi] = ver.astype(x.dtype)
  return out


# ---------------------------------------------------------------------------
# pool(): Datasets and DataArrays
# ---------------------------------------------------------------------------
def _is_spatial(da: xl.DataArray) -> bool:
  return all(d in da.dims for d in _SPATIAL)


def _np_float(data) -> t.Optional[torch.dtype]:
  dtype = _m._torch_dtype_of(data)
  return dtype if dtype in (torch.float32, torch.float64) else None


def _pool_variable(da: xl.DataArray, windows: tuple, kind: str
                   ) -> xl.DataArray:
  """One variable with both spatial dims: ('neighborhood',) + its dims, its
  dtype, where it lies."""
  data, rest, _ = _m._spatial_last(da, plan_lib.LATLON)
  n_row, n_col = (int(n) for n in data.shape[-2:])
  lead = tuple(int(n) for n in data.shape[:-2])
  n_outer = int(np.prod(lead, dtype=np.int64))
  if events._on_device(data):
    device = engine.require_gpu()
    table = None
    if isinstance(data, xl.SlabGather):
      # read where it lies: the gather's index is the slab table
      data = _m._to_device(data, device, allow_gather=True)
      if isinstance(data, xl.SlabGather) and data.base.is_contiguous():
        table, data = data.index.reshape(-1), data.base
    if isinstance(data, (xl.SlabGather, xl.SlabConcat)):
      data = _m._to_device(data, device)
    if table is None and not data.is_contiguous():
      # a view whose slabs are whole (a slice of the leading dims)
      strides = events._intact_strides(data, n_row * n_col)
      if strides is None:
        data = data.contiguous()
      else:
        table = np.zeros(lead, dtype=np.int64)
        for ax, (n, s) in enumerate(zip(lead, strides)):
          shape = [1] * len(lead)
          shape[ax] = n
          table = table + (np.arange(n, dtype=np.int64) * s).reshape(shape)
        table = table.reshape(-1)
    pooled = engine.pool_fields(data, 0, 1, table, n_outer, n_row, n_col,
                                windows, kind)
    pooled = pooled.reshape((len(windows),) + lead + (n_row, n_col))
  else:
    pooled = host_pool(np.ascontiguousarray(np.asarray(data)), windows, kind)
  dims = (NEIGHBORHOOD,) + tuple(rest) + _SPATIAL
  want = (NEIGHBORHOOD,) + tuple(da.dims)
  if dims != want:
    perm = [dims.index(d) for d in want]
    pooled = (pooled.permute(*perm).contiguous()
              if isinstance(pooled, torch.Tensor)
              else np.ascontiguousarray(np.transpose(pooled, perm)))
  return xl.DataArray(pooled, want, da.coords, da.name)


def _checked_windows(variables, lon, neighborhoods, kind: str) -> tuple:
  """Every ValueError of `pool`, before anything is pooled."""
  if kind not in POOLINGS:
    raise ValueError(f'pooling={kind!r}: the pooling is '
                     f'{" or ".join(map(repr, POOLINGS))}')
  windows = _nb._check_windows(neighborhoods, len(lon))
  _nb._check_cyclic(lon)
  for da in variables:
    dtype = _np_float(da.data)
    if dtype is None:
      raise ValueError(f'variable {da.name!r} is {da.data.dtype}: the pooling '
                       'takes float32 and float64')
    max_window = engine.pool_geometry(dtype)['max_window']
    if max(windows) > max_window:
      raise ValueError(
          f'window {max(windows)}: the pooling of a {da.data.dtype} variable '
          f'takes windows up to {max_window} (the halo must fit the LDS)')
  return windows


def pool(obj, neighborhoods, pooling: str = 'mean'):
  """`obj` (a Dataset or a DataArray) with every variable that has both
  `latitude` and `longitude` pooled over the windows `neighborhoods` (module
  docstring): such a variable gets a leading dim `neighborhood`, whose
  coordinate is the window sizes, and keeps its other dims, their order, its
  dtype and its device.  Variables without both spatial dims are returned
  unchanged, without the new dim."""
  given = obj
  if isinstance(obj, xl.DataArray):
    ds = xl.Dataset({obj.name or 'data': obj}, obj.coords)
  else:
    ds = xl.as_dataset(obj)
  spatial = [da for da in ds.data_vars.values() if _is_spatial(da)]
  lon = xl.coord_values(ds, 'longitude') if spatial else np.zeros(0)
  if spatial:
    windows = _checked_windows(spatial, lon, neighborhoods, pooling)
  elif pooling not in POOLINGS:
    raise ValueError(f'pooling={pooling!r}: the pooling is '
                     f'{" or ".join(map(repr, POOLINGS))}')
  else:
    windows = tuple(int(n) for n in neighborhoods)
  coords = dict(ds.coords)
  coords[NEIGHBORHOOD] = np.array(windows, dtype=np.int64)
  out = xl.Dataset(coords=coords, attrs=ds.attrs)
  for name, da in ds.data_vars.items():
    if _is_spatial(da):
      da = _pool_variable(da, windows, pooling)
    out.data_vars[name] = xl.DataArray(da.data, da.dims, coords, name)
  if isinstance(given, xl.DataArray):
    return out.data_vars[given.name or 'data']
  return xl.like_input(out, given)


# ---------------------------------------------------------------------------
# the wrapper metric
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class Pooled(_m.Metric):
  """`metric` -- any `Metric` of this package -- on the pooled fields: every
  entry point pools the common variables of forecast and truth ONCE (one
  `pool` call each, all windows), calls the wrapped metric's entry point of
  the same name on each window's pair and concatenates along a leading
  `neighborhood` dim.  So `compute_chunk_regions` (what `evaluation.
  _metric_and_region_loop` calls) never pools per region, and `compute` is
  the wrapped metric's own `compute` -- for the table metrics the time mean of
  the tables, as they require.

  **Thresholds and climatologies held by the wrapped metric are NOT pooled**:
  they are applied to the pooled fields as they are.  The NaN rule is the
  wrapped metric's own, applied to the pooled fields (where a window that
  holds a NaN is NaN).  `compute` / `compute_regions` carry the wrapped
  metric's attributes and `pooling`.  The generic path: no fused regions of
  its own, no windows of chunks, no chunk programs."""

  metric: t.Optional[_m.Metric] = None
  neighborhoods: t.Sequence[int] = (1, 3, 5, 9, 17)
  pooling: str = 'mean'

  def _result_attrs(self, forecast):
    return {**self.metric._result_attrs(forecast), 'pooling': self.pooling}

  def _each(self, call, forecast, truth):
    if not isinstance(self.metric, _m.Metric):
      raise ValueError(f'Pooled wraps a Metric of this package, not '
                       f'{type(self.metric).__name__}')
    from weatherbench2_amd import program
    rec = program.recorder()
    if rec is not None:
      # the wrapped metric reads pooled fields, which are no input of the
      # chunk: nothing a chunk program could replay
      rec.record(kind='unsupported')
    forecast, truth = _m._inputs(forecast, truth)
    names = _m._common_vars(forecast, truth)
    common = lambda ds: xl.Dataset({k: ds[k] for k in names}, ds.coords,
                                   ds.attrs)
    pooled_f = pool(common(forecast), self.neighborhoods, self.pooling)
    pooled_t = pool(common(truth), self.neighborhoods, self.pooling)
    parts = []
    for k, n in enumerate(xl.coord_values(pooled_f, NEIGHBORHOOD)):
      part = xl.as_dataset(call(pooled_f.isel(**{NEIGHBORHOOD: k}),
                                pooled_t.isel(**{NEIGHBORHOOD: k})))
      if part.has_dim(NEIGHBORHOOD):
        raise ValueError(f'{type(self.metric).__name__} has a '
                         f'{NEIGHBORHOOD!r} dim of its own')
      parts.append(part.expand_dims({NEIGHBORHOOD: [int(n)]}))
    return xl.concat(parts, NEIGHBORHOOD)

  def compute_chunk(self, forecast, truth, region=None, skipna=False):
    return self._each(
        lambda f, t_: self.metric.compute_chunk(f, t_, region=region,
                                                skipna=skipna),
        forecast, truth)

  def compute_chunk_regions(self, forecast, truth, regions, skipna=False):
    return self._each(
        lambda f, t_: self.metric.compute_chunk_regions(f, t_, regions,
                                                        skipna),
        forecast, truth)

  def compute(self, forecast, truth, region=None, skipna=False):
    out = self._each(
        lambda f, t_: self.metric.compute(f, t_, region=region, skipna=skipna),
        forecast, truth)
    return out.assign_attrs(**self._result_attrs(xl.as_dataset(forecast)))

  def compute_regions(self, forecast, truth, regions, skipna=False):
    out = self._each(
        lambda f, t_: self.metric.compute_regions(f, t_, regions, skipna),
        forecast, truth)
    return out.assign_attrs(**self._result_attrs(xl.as_dataset(forecast)))


# ---------------------------------------------------------------------------
# the pooled CRPS
# ---------------------------------------------------------------------------
def pooled_crps(table, fair: bool = False,
                ensemble_size: t.Optional[int] = None):
  """`threshold_weighted.twcrps` of a `PooledCRPS` (or pooled
  `ThresholdWeightedCRPS`) table, along `neighborhood` as along every other
  leading dim: abs_error - pair_distance, with fair=True the estimator of the
  reference's `CRPS`."""
  return _tw.twcrps(table, fair, ensemble_size)


@dataclasses.dataclass(init=False)
class PooledCRPS(Pooled):
  """The CRPS terms of the pooled ensemble: `Pooled(ThresholdWeightedCRPS(
  ConstantThreshold(-inf), 'upper'), neighborhoods, pooling)` without the
  singleton `quantile` dim.  Dims per variable: ('neighborhood', [region,]
  <outer dims>, 'term'); `pooled_crps` turns the table into scores."""

  def __init__(self, neighborhoods=(1, 3, 5, 9, 17), pooling: str = 'mean',
               ensemble_dim: t.Optional[str] = _m.REALIZATION):
    super().__init__(
        _tw.ThresholdWeightedCRPS(
            thresholds=[_nb.ConstantThreshold(-np.inf)], tail='upper',
            ensemble_dim=ensemble_dim),
        neighborhoods, pooling)

  def _each(self, call, forecast, truth):
    out = Pooled._each(self, call, forecast, truth)
    dropped = out.isel(quantile=0)
    return xl.Dataset(dict(dropped.data_vars), dropped.coords, out.attrs)
