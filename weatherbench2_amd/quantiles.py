"""Quantiles along named dims (scripts/compute_quantiles.py:168-183).

`compute_quantiles` is the reference's `_evaluate_chunk_core`: one call of
xarray's `Dataset.quantile` and a rename, which with `name_suffix='_quantile'`
yields the climatology that `thresholds.QuantileThreshold` reads.  `quantile`
is that xarray call with `method='linear'` (the only method here).

Device-backed variables (torch tensors on the GPU, `SlabGather` /
`SlabConcat`) go through the exact-selection kernel of csrc/quantile.hip and
give device tensors; host variables take NumPy's `quantile` / `nanquantile`
and give NumPy arrays.  Inputs are never modified.  The two paths agree bit for
bit but for the sign of a zero result where +0.0 and -0.0 both occur in a
series, which NumPy does not pin either.

Several reduced dims merge into one sample axis (the order of the samples
cannot matter).  Which reductions copy on the device:

  * reduced dims that are adjacent in the variable, with at least one
    preserved dim after them: nothing is copied.  A contiguous tensor is read
    as it is; a view whose blocks of the trailing preserved dims are intact (a
    time slice, a strided selection of whole blocks) and a `SlabGather` over a
    resident base are read through a slab table;
  * preserved dims between the reduced ones, or a reduced dim that is the
    innermost of several: the reduced dims are moved to the front, which is a
    transposing device copy unless the moved view still has intact blocks;
  * every dim reduced: the variable is flattened (a copy only where it is not
    contiguous).
Integer data is converted to float64 first, as NumPy does, which copies.
"""
from __future__ import annotations

import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

QUANTILE_DIM = 'quantile'


def _dims_list(dim, have) -> list:
  if dim is None:
    return list(have)
  dims = [dim] if isinstance(dim, str) else list(dim)
  missing = [d for d in dims if d not in have]
  if missing:
    raise ValueError(f'dims {missing} not found in {tuple(have)}')
  return dims


def _skip(skipna, dtype) -> bool:
  """xarray's default: skip NaN for floating data."""
  if skipna is None:
    return operands.numpy_dtype(dtype).kind in 'fc'
  return bool(skipna)


def _device_quantile(da: xl.DataArray, qs: np.ndarray, reduced: list,
                     skipna: bool) -> tuple:
  """(device tensor [n_q, *preserved shape], preserved dims)."""
  keep = tuple(d for d in da.dims if d not in reduced)
  lay = operands.SeriesLayout.of(da.dims, da.sizes, reduced)
  n_outer, n_red, n_inner = lay.n_outer, lay.n_series, lay.n_point
  if n_red == 0:
    raise ValueError(f'cannot take a quantile over {reduced}: no samples')
  device = engine.require_gpu()
  if n_outer * n_inner == 0:
    out = torch.empty((len(qs), n_outer, n_inner), dtype=torch.float64,
                      device=device)
    return lay.restore(out, (), (len(qs),)), keep
  dtype = operands.float_dtype(da.dtype)
  if lay.n_inner_dims == 0:  # every dim reduced: flattened, no table
    ten, _ = operands.operand(da, lay.order, device, dtype, 0)
    ten, table = ten.contiguous(), None
  else:
    ten, table = lay.operand(da, device, dtype)
  out =engine.quantile_select(ten, table, n_outer, n_red, n_inner, qs, skipna)
  return lay.restore(out, (), (len(qs),)), keep


def _host_quantile(da: xl.DataArray, qs: np.ndarray, reduced: list,
                   skipna: bool) -> tuple:
  import warnings
  data = np.asarray(da.values)
  axes = tuple(da.dims.index(d) for d in reduced)
  keep = tuple(d for d in da.dims if d not in reduced)
  fn = np.nanquantile if skipna else np.quantile
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')  # (all-NaN slices; inf - inf)
    return np.asarray(fn(data, qs, axis=axes, method='linear')), keep


def _array_quantile(da: xl.DataArray, q, reduced: list, skipna,
                    coords: dict) -> xl.DataArray:
  scalar = np.ndim(q) == 0
  qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
  if qs.ndim != 1 or qs.size == 0:
    raise ValueError('q must be a number or a non-empty sequence of numbers')
  if not np.all((qs >= 0) & (qs <= 1)):
    raise ValueError('Quantiles must be in the range [0, 1]')
  skip = _skip(skipna, da.dtype)
  if operands.on_device(da.data):
    out, keep = _device_quantile(da, qs, reduced, skip)
  else:
    out, keep = _host_quantile(da, qs, reduced, skip)
  coords = dict(coords)
  if scalar:
    coords[QUANTILE_DIM] = xl.DataArray(np.asarray(qs[0]), ())
    return xl.DataArray(out[0], keep, coords, da.name)
  coords[QUANTILE_DIM] = qs
  return xl.DataArray(out, (QUANTILE_DIM,) + keep, coords, da.name)


def _kept_coords(coords: dict, reduced: t.Sequence[str]) -> dict:
  """Coordinates that touch no reduced dim."""
  return {k: c for k, c in coords.items()
          if not (set(c.dims) & set(reduced) if isinstance(c, xl.DataArray)
                  else k in reduced)}


def quantile(obj, q, dim=None, *, skipna=None):
  """`xr.Dataset.quantile` / `xr.DataArray.quantile` with method='linear'.

  `dim` is a name or a list of names (None: every dim).  A scalar `q` gives a
  scalar `quantile` coordinate, a sequence a leading `quantile` dim with a
  float64 coordinate.  Preserved dims keep their order; coordinates that touch
  a reduced dim and all attributes are dropped; variables of a dataset with
  none of the reduced dims pass through unchanged.  `skipna=None` skips NaN
  for floating data.  The result is float64.  See the module docstring for
  where the result lives and which reductions copy."""
  if xl.is_xarray(obj):
    if hasattr(obj, 'data_vars'):
      return xl.like_input(quantile(xl.from_xarray(obj), q, dim,
                                    skipna=skipna), obj)
    name = obj.name if obj.name is not None else '_quantile_input'
    lite = xl.from_xarray(obj.to_dataset(name=name))
    return xl.like_input(quantile(lite[name], q, dim, skipna=skipna), obj)
  if isinstance(obj, xl.DataArray):
    reduced = _dims_list(dim, obj.dims)
    return _array_quantile(obj, q, reduced, skipna,
                           _kept_coords(obj.coords, reduced))
  dataset = xl.as_dataset(obj)
  reduced = _dims_list(dim, dataset.dims)
  coords = _kept_coords(dataset.coords, reduced)
  out = xl.Dataset(coords=coords)
  for name, da in dataset.data_vars.items():
    mine = [d for d in reduced if d in da.dims]
    if not mine:
      out.data_vars[name] = xl.DataArray(da.data, da.dims, out.coords, name)
      continue
    res = _array_quantile(da, q, mine, skipna, {})
    out.coords.setdefault(QUANTILE_DIM, res.coords[QUANTILE_DIM])
    out.data_vars[name] = xl.DataArray(res.data, res.dims, out.coords, name)
  return out


def compute_quantiles(chunk, quantiles, dim, skipna: bool = False,
                      name_suffix: str = ''):
  """The reference's `_evaluate_chunk_core` (compute_quantiles.py:168-183):
  the quantiles `quantiles` of every variable of `chunk` over the dims `dim`
  (those not in `dim` are preserved), `name_suffix` appended to every variable
  name.  `name_suffix='_quantile'` gives the climatology of
  `thresholds.QuantileThreshold`."""
  given = chunk
  chunk = xl.as_dataset(chunk)
  dims = [dim] if isinstance(dim, str) else list(dim)
  have = set(chunk.dims)
  preserve_dims = {d for d in chunk.dims if d not in dims}
  if not preserve_dims.issubset(have):
    raise ValueError(
        f'User specified dim={dims}, which results in preserved dims '
        f'{preserve_dims} , not being a subset of {have}')
  if not set(dims).issubset(have):  # (what xarray's quantile raises)
    raise ValueError(f'Dimensions {sorted(set(dims) - have)} not found in '
                     f'the chunk, whose dims are {sorted(have)}')
  quantiles = [float(v) for v in quantiles]
  if any(v < 0 or v > 1 for v in quantiles):
    raise ValueError(
        f'Expected all quantiles to be in [0, 1]. Found {quantiles=}')
  values = quantile(chunk, quantiles, dims, skipna=skipna)
  out = xl.Dataset(coords=values.coords)
  for name, da in values.data_vars.items():
    new = str(name) + name_suffix
    out.data_vars[new] = xl.DataArray(da.data, da.dims, out.coords, new)
  return xl.like_input(out, given)
