"""Threshold-event verification: joint exceedance tables and their scores.

The reference reduces an event `x > threshold` to one number per threshold
(Brier, ignorance, RPS; metrics.py:1524-1891).  Reliability diagrams, ROC
curves, the Brier decomposition and contingency tables (POD, FAR, CSI, ETS,
frequency bias) are all functions of one small sufficient statistic it never
forms: the region-weighted joint frequency of (number of members exceeding,
observation exceeds).  `EventTable` computes that table; the score functions
below are host arithmetic on it.

One grid point under one threshold field `thr` (`Threshold.compute(truth)`):

  k     number of members with x > thr, 0..M
  o     1 if truth > thr else 0
  IEEE comparisons: a NaN threshold makes both false (as the reference's
  `xr.where(x > threshold, 1.0, 0.0)`), equality is not exceedance, +-inf are
  ordinary values.  The point is INVALID iff the truth or any member is NaN.
  code  o * (M + 1) + k for a valid point, 2 (M + 1) for an invalid one;
        n_code = 2 (M + 1) + 1.

A deterministic forecast is the case M = 1.  With the dense region weights of
the other metrics, W_r[i, j] = w_lat[i] * lat_mult_r[i] * lon_mult_r[j]
(`plan.get_lat_weights`, `regions.decompose_region`; repeated rows / columns
count twice), the table of a cell (outer index, region) is
N[code] = sum_ij W_r[i, j] [code_ij == code] and the result is

  p[o, k] = N[o (M + 1) + k] / sum_valid N

the area-weighted mean of the one-hot indicator over the valid points.
skipna=False: a cell with invalid mass is NaN throughout.  skipna=True: the
invalid points are left out; a cell without valid mass is NaN.

The weights factor, so the points are only COUNTED (integers) per (row,
column class) -- a class being a set of columns on which every region has the
same multiplicity -- by the K18 kernel (csrc/event_table.hip) for
device-backed variables and by NumPy for host ones; the float work is one
ordered fold over the rows.  Both paths produce the same integers and fold in
the same order, so they agree bit for bit.  Regions with a 2-D weight field
(`LandRegion`) do not factor and raise a ValueError.

The kernel takes (latitude, longitude) slabs: a (longitude, latitude) variable
costs one transposing copy here.
"""
from __future__ import annotations

import dataclasses
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import metrics as _m
from weatherbench2_amd import plan as plan_lib
from weatherbench2_amd import regions as regions_lib
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.metrics import Metric, ThresholdMetric

MAX_MEMBERS = 128  # limits of wb2_event_counts
MAX_CLASSES = 64
OBSERVED, EXCEEDING = 'observed', 'members_exceeding'


def n_codes(n_member: int) -> int:
  return 2 * (n_member + 1) + 1


# ---------------------------------------------------------------------------
# regions -> row weights, column classes
# ---------------------------------------------------------------------------
def column_classes(regions: t.Mapping[str, t.Any], latitude, longitude):
  """(col_class int32[n_lon], mult int32[n_region, n_class], wrow float64
  [n_region, n_lat]) of the regions (None = global), in their order: region
  r weighs point (i, j) with wrow[r, i] * mult[r, col_class[j]].  Classes are
  numbered by first appearance and need not be contiguous (`europe` wraps)."""
  lat, lon = np.asarray(latitude), np.asarray(longitude)
  w_lat = np.asarray(plan_lib.get_lat_weights(lat), dtype=np.float64)
  lon_mults, wrow = [], []
  for name, region in regions.items():
    spec = regions_lib.decompose_region(region, lat, lon)
    if spec.field is not None:
      raise ValueError(
          f'region {name!r} ({type(region).__name__}) has a 2-D weight field: '
          'its weights do not factor into a row weight and a column '
          'multiplicity, which the event table counts by')
    lon_mults.append(spec.lon_mult)
    wrow.append(w_lat * spec.lat_mult.astype(np.float64))
  per_col = np.stack(lon_mults, axis=1) if lon_mults else np.zeros(
      (len(lon), 0), dtype=np.int64)
  seen: dict = {}
  col_class = np.empty(len(lon), dtype=np.int32)
  for j, key in enumerate(map(tuple, per_col.tolist())):
    col_class[j] = seen.setdefault(key, len(seen))
  if len(seen) > MAX_CLASSES:
    raise ValueError(f'the regions split the columns into {len(seen)} classes;'
                     f' the event table takes {MAX_CLASSES}')
  mult = np.array(list(seen), dtype=np.int32).reshape(len(seen), -1).T
  return (col_class, np.ascontiguousarray(mult),
          np.array(wrow, dtype=np.float64).reshape(len(regions), len(lat)))


# ---------------------------------------------------------------------------
# the host path: same integers, same fold order
# ---------------------------------------------------------------------------
def host_slab(x: np.ndarray, table, o: int, slab: int) -> np.ndarray:
  """Slab `o` of the flat host array `x` (`table`: None = identity)."""
  first = (o if table is None else int(table[o])) * slab
  return x[first:first + slab]


def host_members(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
                 truth: np.ndarray, truth_slab, n_outer: int, slab: int):
  """The slab addressing of the host paths, from the leading arguments of
  `engine.event_counts` (host arrays): yields (outer index, members [n_member,
  slab], truth [slab])."""
  ens, truth = ens.reshape(-1), truth.reshape(-1)
  for o in range(n_outer):
    x = np.stack([host_slab(ens[m * member_stride:], ens_slab, o, slab)
                  for m in range(n_member)])
    yield o, x, host_slab(truth, truth_slab, o, slab)


def host_exceedance(ens: np.ndarray, member_stride: int, n_member: int,
                    ens_slab, truth: np.ndarray, truth_slab, thresholds,
                    thr_slabs, n_outer: int, slab: int):
  """The per-point definition on the host, from the leading arguments of
  `engine.event_counts` (host arrays): yields (threshold index, outer index,
  k, obs, bad) over the `slab` points of every slab."""
  thr_slabs = thr_slabs if thr_slabs is not None else [None] * len(thresholds)
  for o, x, tv in host_members(ens, member_stride, n_member, ens_slab, truth,
                               truth_slab, n_outer, slab):
    bad = np.isnan(tv) | np.isnan(x).any(axis=0)
    for ti, (thr, table) in enumerate(zip(thresholds, thr_slabs)):
      hv = host_slab(thr.reshape(-1), table, o, slab)
      with np.errstate(invalid='ignore'):
        k, obs = (x > hv[None]).sum(axis=0), tv > hv
      yield ti, o, k, obs, bad


def host_counts(ens: np.ndarray, member_stride: int, n_member: int, ens_slab,
                truth: np.ndarray, truth_slab, thresholds, thr_slabs,
                n_outer: int, n_row: int, n_col: int, col_class,
                n_class: int) -> np.ndarray:
  """`engine.event_counts` in NumPy: the same arguments (contiguous host
  arrays instead of tensors), the same int32 [n_threshold, n_outer, n_row,
  n_class, n_code] result."""
  n_code = n_codes(n_member)
  out = np.zeros((len(thresholds), n_outer, n_row, n_class, n_code),
                 dtype=np.int32)
  cls = np.asarray(col_class, dtype=np.int64)
  bin0 = ((np.arange(n_row)[:, None] * n_class + cls[None, :]) * n_code
          ).reshape(-1)
  for ti, o, k, obs, bad in host_exceedance(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, thresholds,
      thr_slabs, n_outer, n_row * n_col):
    code = np.where(bad, 2 * (n_member + 1), obs * (n_member + 1) + k)
    out[ti, o] = np.bincount(bin0 + code, minlength=n_row * n_class *
                             n_code).reshape(n_row, n_class, n_code)
  return out


def host_fold(cnt: np.ndarray, wrow: np.ndarray, mult: np.ndarray
              ) -> np.ndarray:
  """`engine.event_fold` in NumPy: the inner sum over the classes in int64,
  then acc = acc + wrow[r, i] * float(s) over the rows in increasing order."""
  s = np.einsum('rc,toicd->toird', mult.astype(np.int64),
                cnt.astype(np.int64))
  acc = np.zeros(s.shape[:2] + s.shape[3:], dtype=np.float64)
  for i in range(cnt.shape[2]):
    acc = acc + wrow[None, None, :, i, None] * s[:, :, i].astype(np.float64)
  return acc


def normalize(table: np.ndarray, n_member: int, skipna: bool) -> np.ndarray:
  """[..., n_code] region sums -> p[..., 2, M + 1] = N / sum_valid N, the
  valid mass summed over the codes in increasing order."""
  n_valid = 2 * (n_member + 1)
  valid = np.zeros(table.shape[:-1], dtype=np.float64)
  for code in range(n_valid):
    valid = valid + table[..., code]
  with np.errstate(all='ignore'):
    p = table[..., :n_valid] / valid[..., None]
  dead = valid == 0.0
  if not skipna:
    dead = dead | (table[..., n_valid] != 0.0)
  p[dead] = np.nan
  return p.reshape(table.shape[:-1] + (2, n_member + 1))


# ---------------------------------------------------------------------------
# operands: (lat, lon) slabs and their tables
# ---------------------------------------------------------------------------
def _on_device(data) -> bool:
  if isinstance(data, xl.SlabConcat):
    return data.on_device
  base = data.base if isinstance(data, xl.SlabGather) else data
  return isinstance(base, torch.Tensor) and base.device.type == 'cuda'


def _dtype_of(data) -> torch.dtype:
  dtype = _m._torch_dtype_of(data)
  return torch.float64 if dtype is None else dtype


@dataclasses.dataclass
class _Operands:
  out_dims: tuple
  out_shape: tuple
  n_member: int
  member_stride: int            # elements
  arrays: list                  # members, truth, thresholds: tensors / ndarrays
  tables: list                  # host int64 slab tables (None: identity)
  device: t.Optional[torch.device]

  @property
  def n_outer(self) -> int:
    return int(np.prod(self.out_shape, dtype=np.int64))

  def front(self, n_row: int, n_col: int) -> tuple:
    """The leading arguments of `engine.event_counts` and `event_codes`."""
    return (self.arrays[0], self.member_stride, self.n_member, self.tables[0],
            self.arrays[1], self.tables[1], self.arrays[2:], self.tables[2:],
            self.n_outer, n_row, n_col)


def _intact_strides(x: torch.Tensor, slab: int) -> t.Optional[tuple]:
  """Outer strides in slabs of a view whose 2-D slabs are whole."""
  st = x.stride()
  if slab > 0 and st[-1] == 1 and st[-2] == x.shape[-1] and all(
      s >= 0 and s % slab == 0 for s in st[:-2]):
    return tuple(s // slab for s in st[:-2])
  return None


def _operands(forecast, fvar, others, ensemble_dim) -> _Operands:
  """The layout of one variable: `others` = [truth, threshold, ...].  The
  outer dims are the forecast's without the ensemble dim, then the unseen
  dims of the others in their order."""
  has_ens = ensemble_dim is not None and ensemble_dim in fvar.dims
  prepared = [_m._spatial_last(da, plan_lib.LATLON)[:2]
              for da in [fvar] + list(others)]
  fdata, frest = prepared[0]
  if has_ens and ensemble_dim in prepared[1][1]:
    raise ValueError(
        f'truth must not have the ensemble dim {ensemble_dim!r}')
  fsizes = dict(zip(frest, fdata.shape[:-2]))
  out_dims = [d for d in frest if not (has_ens and d == ensemble_dim)]
  sizes = {d: fsizes[d] for d in out_dims}
  for data, rest in prepared[1:]:
    for d, n in zip(rest, data.shape[:-2]):
      if d not in out_dims:
        out_dims.append(d)
        sizes[d] = n
  out_dims = tuple(out_dims)
  out_shape = tuple(sizes[d] for d in out_dims)
  n_member = fsizes[ensemble_dim] if has_ens else 1
  n_row, n_col = (int(n) for n in fdata.shape[-2:])
  slab = n_row * n_col
  for data, _ in prepared:
    if tuple(data.shape[-2:]) != (n_row, n_col):
      raise ValueError(f'spatial shape {tuple(data.shape[-2:])} does not '
                       f'match the forecast\'s {(n_row, n_col)}')

  dtype = _dtype_of(fdata)
  for data, _ in prepared[1:]:
    dtype = torch.promote_types(dtype, _dtype_of(data))
  if dtype not in (torch.float32, torch.float64):
    dtype = torch.float64
  on_device = any(_on_device(data) for data, _ in prepared[:2])
  device = engine.require_gpu() if on_device else None

  def dense(data):
    """A contiguous array of the common dtype where the variable lives."""
    if device is None:
      np_dtype = np.float32 if dtype == torch.float32 else np.float64
      return np.ascontiguousarray(np.asarray(data), dtype=np_dtype)
    return _m._to_device(data, device).to(dtype).contiguous()

  # the forecast: read where it lies when only its slab table differs
  strides = index = None
  if device is not None and _dtype_of(fdata) == dtype:
    if isinstance(fdata, torch.Tensor) and fdata.device == device and (
        not fdata.is_contiguous()):
      strides = _intact_strides(fdata, slab)
    elif isinstance(fdata, xl.SlabGather):
      gathered = _m._to_device(fdata, device, allow_gather=True)
      if isinstance(gathered, xl.SlabGather) and (
          gathered.base.is_contiguous()):
        moved = gathered.index
        if has_ens:
          moved = np.moveaxis(moved, frest.index(ensemble_dim), -1)
        else:
          moved = moved[..., None]
        step = np.diff(moved, axis=-1)
        if step.size == 0 or (step.min() == step.max() and step.min() >= 0):
          index = moved[..., 0]
          fdata = gathered.base
          member_slabs = int(step.flat[0]) if step.size else 0
      else:
        fdata = gathered
  if index is not None:
    extra = len(out_dims) - index.ndim
    ens_table = np.broadcast_to(index.reshape(index.shape + (1,) * extra),
                                out_shape).reshape(-1)
  else:
    if strides is None:
      fdata = dense(fdata)
      stride, c_strides = 1, []
      for n in reversed(fdata.shape[:-2]):
        c_strides.append(stride)
        stride *= int(n)
      strides = tuple(reversed(c_strides))
    by_dim = dict(zip(frest, strides))
    member_slabs = by_dim[ensemble_dim] if has_ens else 0
    table = np.zeros(out_shape, dtype=np.int64)
    for d in out_dims:
      if d in by_dim:
        shape = [1] * len(out_shape)
        shape[out_dims.index(d)] = fsizes[d]
        table = table + (np.arange(fsizes[d], dtype=np.int64) * by_dim[d]
                         ).reshape(shape)
    ens_table = table.reshape(-1)
  n_outer = int(np.prod(out_shape, dtype=np.int64))
  if np.array_equal(ens_table, np.arange(n_outer)):
    ens_table = None
  arrays, tables = [fdata], [ens_table]
  for data, rest in prepared[1:]:
    arrays.append(dense(data))
    tables.append(_m._slab_table(out_dims, out_shape, rest, data.shape[:-2]))
  return _Operands(out_dims, out_shape, n_member, member_slabs * slab, arrays,
                   tables, device)


def _region_tables(ops: _Operands, n_row: int, n_col: int, col_class,
                   mult, wrow) -> np.ndarray:
  """float64 [n_threshold, n_outer, n_region, n_code] on the host, through
  K18 for device operands and through NumPy for host ones."""
  args = ops.front(n_row, n_col) + (col_class, mult.shape[1])
  if ops.device is None:
    return host_fold(host_counts(*args), wrow, mult)
  table = engine.event_fold(engine.event_counts(*args), wrow, mult)
  engine.order_read(table)
  return table.cpu().numpy()


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
class ExceedanceTable(ThresholdMetric):
  """What the tables over the per-point exceedance share (`EventTable`,
  `neighborhood.FractionsTable`): the operands of every common variable, the
  checks on the ensemble, the forecast-led order of the outer dims, the
  `region` / `quantile` coords and the attrs.  A subclass states its noun, the
  dims around the outer ones, its checks before the loop (`_setup`) and

    _values(ops, n_row, n_col, col_class, mult, wrow, skipna, setup)
        one variable: [n_threshold, <lead dims>, n_outer, n_region, <trailing
        dims>]
    _extra_coords(n_member, setup)
        {dim: coord} of the lead and trailing dims, in that order."""

  ensemble_dim = _m.REALIZATION  # (a dataclass field of each subclass)
  # one pass over the points answers every region; no windows of chunks
  _fused_regions = True
  _reads_slabs_in_place = False
  _noun = 'exceedance table'
  # the dims of a result: [region,] quantile, lead, <outer dims>, trailing
  _lead_dims = ()
  _trailing_dims = ()

  def _ensemble_size(self, forecast) -> int:
    if self.ensemble_dim is not None and self.ensemble_dim in forecast.dims:
      return int(forecast.sizes[self.ensemble_dim])
    return 1

  def _result_attrs(self, forecast):
    return {'ensemble_size': self._ensemble_size(forecast)}

  def _setup(self, lat, lon, mult, wrow):
    """The checks before the loop over the variables: (mult, wrow) as the
    kernels get them and whatever `_values` and `_extra_coords` need."""
    return mult, wrow, None

  def compute_chunk(self, forecast, truth, region=None, skipna=False,
                    regions: t.Optional[dict] = None):
    forecast, truth = _m._inputs(forecast, truth)
    if not self.thresholds:
      raise ValueError(f'{type(self).__name__} needs at least one threshold')
    region_set = regions if regions is not None else {'region': region}
    lat = xl.coord_values(forecast, 'latitude')
    lon = xl.coord_values(forecast, 'longitude')
    col_class, mult, wrow = column_classes(region_set, lat, lon)
    mult, wrow, setup = self._setup(lat, lon, mult, wrow)
    threshold_ds = [xl.as_dataset(th.compute(truth))
                    for th in self.thresholds]
    out = xl.Dataset()
    sizes = set()
    per_var = {}
    for name in _m._common_vars(forecast, truth):
      fvar = forecast[name]
      ops = _operands(forecast, fvar,
                      [truth[name]] + [ds[name] for ds in threshold_ds],
                      self.ensemble_dim)
      if not 1 <= ops.n_member <= MAX_MEMBERS:
        raise ValueError(f'{ops.n_member} members: the {self._noun} takes 1 '
                         f'to {MAX_MEMBERS}')
      sizes.add(ops.n_member)
      v = self._values(ops, len(lat), len(lon), col_class, mult, wrow, skipna,
                       setup)
      first = 1 + len(self._lead_dims)
      v = v.reshape(v.shape[:first] + ops.out_shape + v.shape[first + 1:])
      # outer dims as xarray orders the plain Brier score (forecast-led)
      fdims = tuple(d for d in fvar.dims if d in ops.out_dims)
      order = []
      for operand in (fdims, threshold_ds[0][name].dims, truth[name].dims):
        order += [d for d in operand if d in ops.out_dims and d not in order]
      # [T, lead.., outer.., R, trailing..] -> ([R,] T, lead.., outer.., ..)
      at_region = first + len(ops.out_dims)
      axes = (list(range(first)) +
              [first + ops.out_dims.index(d) for d in order] +
              list(range(at_region + 1, v.ndim)))
      if regions is not None:
        v = np.transpose(v, [at_region] + axes)
      else:
        v = np.transpose(v, axes + [at_region])[..., 0]
      per_var[name] = (tuple(order), np.ascontiguousarray(v))
      out.coords.update(_m._result_coords(forecast, tuple(order)))
    if len(sizes) > 1:
      raise ValueError(f'the variables differ in ensemble size: {sizes}')
    n_member = sizes.pop() if sizes else self._ensemble_size(forecast)
    front = ('region', 'quantile') if regions is not None else ('quantile',)
    if regions is not None:
      out.coords['region'] = np.array(list(regions), dtype=object)
    out.coords['quantile'] = np.array(
        [th.quantile for th in self.thresholds], dtype=np.float64)
    out.coords.update(self._extra_coords(n_member, setup))
    for name, (order, v) in per_var.items():
      out.data_vars[name] = xl.DataArray(
          v, front + self._lead_dims + order + self._trailing_dims, out.coords,
          name)
    return out.assign_attrs(
        threshold_method=type(self.thresholds[0]).__name__,
        ensemble_size=n_member)


@dataclasses.dataclass
class EventTable(ExceedanceTable):
  """Joint exceedance table of a forecast against climatological thresholds.

  Per common variable the result is p with dims ('quantile', <outer dims in
  xarray's order>, 'observed', 'members_exceeding') -- with `regions=` a
  leading 'region' dim --: p[.., o, k] is the area-weighted frequency, over
  the valid points of the region, of "k members exceed the threshold and the
  observation does (o = 1) or does not (o = 0)".  A forecast variable without
  `ensemble_dim` (or ensemble_dim=None) is a deterministic forecast: M = 1.
  Attributes: `threshold_method`, `ensemble_size`.

  `compute` is the time mean of the tables.  Scores are non-linear in the
  table, so they are taken FROM the mean table (`brier_score(metric.compute(
  ...))`) and never averaged themselves.
  """

  ensemble_dim: t.Optional[str] = _m.REALIZATION
  _noun = 'event table'
  _trailing_dims = (OBSERVED, EXCEEDING)

  def _values(self, ops, n_row, n_col, col_class, mult, wrow, skipna, setup):
    table = _region_tables(ops, n_row, n_col, col_class, mult, wrow)
    return normalize(table, ops.n_member, skipna)  # [T, outer, R, 2, M + 1]

  def _extra_coords(self, n_member, setup):
    return {OBSERVED: np.array([0, 1], dtype=np.int64),
            EXCEEDING: np.arange(n_member + 1, dtype=np.int64)}


# ---------------------------------------------------------------------------
# scores: host arithmetic over the last two dims of a table
# ---------------------------------------------------------------------------
def _per_table(fn, trailing=((OBSERVED, 2), (EXCEEDING, None)),
               noun='an event table'):
  """`fn(p, lead dims, coords)` over a table DataArray, or over every variable
  of a table Dataset ({name: result} where a result is itself a Dataset).
  `trailing`: the (dim, size or None) pairs a table ends with, which are
  checked and left to `fn`; `noun` names the table in the error."""
  n_trail = len(trailing)

  def wrapper(table, *args, **kwargs):
    if xl.is_xarray(table):
      table = (xl.from_xarray(table) if hasattr(table, 'data_vars') else
               xl.DataArray(table.values, tuple(table.dims),
                            {k: np.asarray(table.coords[k].values)
                             for k in table.dims if k in table.coords},
                            table.name))
    def one(da):
      lead = tuple(da.dims[:-n_trail])
      if tuple(da.dims[-n_trail:]) != tuple(d for d, _ in trailing) or any(
          n is not None and da.shape[i - n_trail] != n
          for i, (_, n) in enumerate(trailing)):
        raise ValueError(f'not {noun}: dims {da.dims}')
      p = np.asarray(da.values, dtype=np.float64)
      coords = {k: c for k, c in da.coords.items() if
                (isinstance(c, xl.DataArray) and
                 all(d in lead for d in c.dims)) or
                (not isinstance(c, xl.DataArray) and k in lead)}
      with np.errstate(all='ignore'):
        return fn(p, lead, coords, *args, **kwargs)
    if isinstance(table, xl.DataArray):
      return one(table)
    results = {name: one(da) for name, da in table.items()}
    if all(isinstance(r, xl.DataArray) for r in results.values()):
      coords = {}
      for r in results.values():
        coords.update(r.coords)
      return xl.Dataset(results, coords, table.attrs)
    return results
  wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
  return wrapper


def _dataset(fields: dict, dims, coords) -> xl.Dataset:
  return xl.Dataset({k: xl.DataArray(v, dims, coords, k)
                     for k, v in fields.items()}, coords)


def _abcd(p, min_members):
  m = int(min_members)
  if not 0 <= m <= p.shape[-1]:
    raise ValueError(f'min_members={m} outside 0..{p.shape[-1]}')
  return (p[..., 1, m:].sum(-1), p[..., 0, m:].sum(-1),
          p[..., 1, :m].sum(-1), p[..., 0, :m].sum(-1))


@_per_table
def contingency(p, dims, coords, min_members: int = 1):
  """2 x 2 contingency frequencies: the event is forecast iff at least
  `min_members` members exceed.  hits a, false_alarms b, misses c,
  correct_negatives d (a + b + c + d = 1)."""
  a, b, c, d = _abcd(p, min_members)
  return _dataset({'hits': a, 'false_alarms': b, 'misses': c,
                   'correct_negatives': d}, dims, coords)


@_per_table
def categorical_scores(p, dims, coords, min_members: int = 1):
  """pod a/(a+c), far b/(a+b), pofd b/(b+d), csi a/(a+b+c), frequency_bias
  (a+b)/(a+c), ets (a-a_r)/(a+b+c-a_r) with a_r = (a+b)(a+c).  0/0 is NaN."""
  a, b, c, d = _abcd(p, min_members)
  a_r = (a + b) * (a + c)
  return _dataset({'pod': a / (a + c), 'far': b / (a + b),
                   'pofd': b / (b + d), 'csi': a / (a + b + c),
                   'frequency_bias': (a + b) / (a + c),
                   'ets': (a - a_r) / (a + b + c - a_r)}, dims, coords)


def _probability(p):
  n_member = p.shape[-1] - 1
  return np.arange(n_member + 1, dtype=np.float64) / n_member


@_per_table
def reliability(p, dims, coords):
  """The reliability diagram: forecast_probability y_k = k / M,
  forecast_frequency f_k = p[0, k] + p[1, k] and observed_frequency
  p[1, k] / f_k (NaN where f_k = 0), along `members_exceeding`."""
  f = p[..., 0, :] + p[..., 1, :]
  y = _probability(p)
  coords = dict(coords, **{EXCEEDING: np.arange(p.shape[-1], dtype=np.int64)})
  out = _dataset({'forecast_frequency': f,
                  'observed_frequency': p[..., 1, :] / f},
                 dims + (EXCEEDING,), coords)
  out.data_vars['forecast_probability'] = xl.DataArray(
      y, (EXCEEDING,), out.coords, 'forecast_probability')
  return out


@_per_table
def brier_score(p, dims, coords):
  """sum_k sum_o p[o, k] (k / M - o)^2: the Brier score of the ensemble
  frequency k / M as the forecast probability."""
  y = _probability(p)
  value = (p[..., 0, :] * (y - 0.0) ** 2).sum(-1) + (
      p[..., 1, :] * (y - 1.0) ** 2).sum(-1)
  return xl.DataArray(value, dims, coords)


@_per_table
def brier_decomposition(p, dims, coords):
  """reliability sum f_k (y_k - o_k)^2, resolution sum f_k (o_k - o)^2 and
  uncertainty o (1 - o), with o_k = p[1, k] / f_k and o = sum_k p[1, k]; terms
  with f_k = 0 are dropped.  brier_score = reliability - resolution +
  uncertainty."""
  f = p[..., 0, :] + p[..., 1, :]
  y = _probability(p)
  obar_k = p[..., 1, :] / f
  obar = p[..., 1, :].sum(-1)
  used = f > 0
  rel = np.where(used, f * (y - obar_k) ** 2, 0.0).sum(-1)
  res = np.where(used, f * (obar_k - obar[..., None]) ** 2, 0.0).sum(-1)
  nan = np.isnan(p).any(axis=(-2, -1))
  rel, res = np.where(nan, np.nan, rel), np.where(nan, np.nan, res)
  return _dataset({'reliability': rel, 'resolution': res,
                   'uncertainty': obar * (1.0 - obar)}, dims, coords)


@_per_table
def roc(p, dims, coords):
  """pofd and pod for min_members = M + 1 ... 0, that is from (0, 0) to
  (1, 1), along `min_members`, and auc, the area below by the trapezoid
  rule."""
  n = p.shape[-1]
  pofd, pod = [], []
  for m in range(n, -1, -1):
    a, b, c, d = _abcd(p, m)
    pod.append(a / (a + c))
    pofd.append(b / (b + d))
  pofd, pod = np.stack(pofd, -1), np.stack(pod, -1)
  auc = (0.5 * (pod[..., 1:] + pod[..., :-1]) *
         (pofd[..., 1:] - pofd[..., :-1])).sum(-1)
  coords = dict(coords, min_members=np.arange(n, -1, -1, dtype=np.int64))
  out = _dataset({'pofd': pofd, 'pod': pod}, dims + ('min_members',), coords)
  out.data_vars['auc'] = xl.DataArray(auc, dims, out.coords, 'auc')
  return out
