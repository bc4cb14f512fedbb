"""Dataset slicing: the numerical content of scripts/slice_dataset.py.

`slice_dataset` applies the script's selection sequence -- make some dims
increasing, drop or keep variables, `isel`, `sel`, `sel_strings`, `drop_isel`,
`drop_sel`, `drop_sel_strings` -- to an `xarray_lite.Dataset`.  All label work
is host work (`indexing.slice_positions`, `indexing.list_positions`): every
step only rewrites ONE int64 position vector per dim, holding positions into
the original axis, and nothing moves until all steps are composed.  Then each
variable is moved once:

  * no dim of it is touched: the same array object comes back;
  * only dims before the last two are touched: whole slabs move, by a slab
    table (`indexing.slab_table`); `materialize=False` returns a `SlabGather`
    over the input, `materialize=True` goes through csrc/slab_scatter.hip with
    one destination per source;
  * one of the last two dims is touched: csrc/box_gather.hip (K17) for device
    arrays of 4- or 8-byte elements, one launch per variable, a bit copy;
  * everything else (host arrays, other device dtypes, variables of fewer than
    two dims): a chain of `np.take` / `torch.index_select`, the same bits.

Coordinates are sliced on the host.  The `_start/_stop/_step` forms of the
three drop options are refused: what xarray's `drop_sel` / `drop_isel` do with
a slice is pinned by no reference test.
"""
from __future__ import annotations

import math
import re
import typing as t

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import indexing
from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

DimValue = t.Union[int, float, str]
Selector = t.Union[None, str, t.Mapping[str, DimValue]]


def get_dim_value(value_string) -> DimValue:
  """int, then float, then the string itself (flag_utils.get_dim_value)."""
  value_string = str(value_string)
  for cast in (int, float):
    try:
      return cast(value_string)
    except ValueError:
      pass
  return value_string


def parse_dim_value_pairs(dim_value_string: str) -> dict:
  """'a=1,b=2.5,c=x' -> {'a': 1, 'b': 2.5, 'c': 'x'}."""
  pairs = {}
  if dim_value_string:
    for entry in dim_value_string.split(','):
      key, value = entry.split('=')
      pairs[key] = get_dim_value(value)
  return pairs


def get_selections(flag_values: t.Mapping[str, DimValue],
                   force_string: bool) -> list:
  """The script's `_get_selections`: [{dim: list}] for every `dim_list` key,
  then [{dim: slice(start, stop, step)}] for the dims with `_start`, `_stop` or
  `_step` keys, each group in the order its dim first appears.  Values are
  strings throughout with `force_string`; a step is always an int."""
  tostr = str if force_string else (lambda v: v)
  list_selectors: dict = {}
  value_selectors: dict = {}
  for k, v in flag_values.items():
    match = re.search(r'^(.*)_(start|stop|step|list)$', k)
    if not match:
      raise ValueError(f'Flag {k} did not end in _(start|stop|step|list)')
    dim, placement = match.groups()
    if placement == 'list':
      v = str(v)  # (a one-item list may have been parsed as a number)
      if '++' in v:
        raise ValueError(f'Found ambiguous "++" in {dim=} flag value {v}')
      list_selectors[dim] = [tostr(get_dim_value(v_i)) for v_i in v.split('+')]
    else:
      v = get_dim_value(v)
      parts = value_selectors.setdefault(dim, [None, None, None])
      if placement == 'step':
        parts[2] = int(v)
      else:
        parts[placement == 'stop'] = tostr(v)
  return ([{dim: sel} for dim, sel in list_selectors.items()] +
          [{dim: slice(*sel)} for dim, sel in value_selectors.items()])


def output_chunks(input_chunks: t.Mapping[str, int],
                  sizes: t.Mapping[str, int],
                  overrides: t.Optional[t.Mapping[str, int]] = None) -> dict:
  """The script's output chunk sizes: the input's, for the dims the sliced
  dataset still has, each cut to the sliced size unless `overrides` names
  it."""
  overrides = overrides or {}
  return {k: overrides[k] if k in overrides else min(v, sizes[k])
          for k, v in input_chunks.items() if k in sizes}


def _as_pairs(selector: Selector) -> dict:
  if selector is None:
    return {}
  return parse_dim_value_pairs(selector) if isinstance(selector, str) \
      else dict(selector)


def _as_names(names) -> list:
  if names is None:
    return []
  return [n for n in names.split(',') if n] if isinstance(names, str) \
      else list(names)


class _Composer:
  """One int64 vector per dim: the positions into the ORIGINAL axis that the
  steps so far have kept, in order."""

  def __init__(self, sizes: dict, labels: dict):
    self.sizes = dict(sizes)
    self.labels = labels  # dim -> labels of the original axis
    self.pos: dict = {}

  def current(self, dim: str) -> np.ndarray:
    if dim not in self.sizes:
      raise ValueError(f'Dimensions {{{dim!r}}} do not exist. Expected one or '
                       f'more of {tuple(self.sizes)}')
    if dim not in self.pos:
      return np.arange(self.sizes[dim], dtype=np.int64)
    return self.pos[dim]

  def labels_now(self, dim: str) -> np.ndarray:
    pos = self.current(dim)
    if dim not in self.labels:
      raise KeyError(f'no index found for coordinate {dim!r}')
    return np.asarray(self.labels[dim])[pos]

  def keep(self, dim: str, sub) -> None:
    """`sub`: positions into the axis as it stands now."""
    self.pos[dim] = self.current(dim)[np.asarray(sub, dtype=np.int64)]

  def _listed(self, dim: str, values) -> np.ndarray:
    """A list of positions into the present axis, negatives from the end."""
    n = self.current(dim).size
    idx = np.asarray(values)
    if idx.dtype.kind not in 'iu':
      raise TypeError(f'positions along {dim!r} must be integers: {values!r}')
    idx = idx.astype(np.int64)
    if idx.size and (idx.min() < -n or idx.max() >= n):
      raise IndexError(f'position out of range for {dim!r} of size {n}: '
                       f'{values!r}')
    return np.where(idx < 0, idx + n, idx)

  def isel(self, dim: str, sel) -> None:
    n = self.current(dim).size
    self.keep(dim, np.arange(n)[sel] if isinstance(sel, slice)
              else self._listed(dim, sel))

  def sel(self, dim: str, sel) -> None:
    labels = self.labels_now(dim)
    self.keep(dim, indexing.slice_positions(
        labels, sel.start, sel.stop, sel.step) if isinstance(sel, slice)
              else indexing.list_positions(labels, sel))

  def drop(self, dim: str, sel, by_label: bool, option: str) -> None:
    if isinstance(sel, slice):
      raise ValueError(
          f'{option} takes {dim}_list only: the _start/_stop/_step forms of '
          'the drop options are not supported')
    gone = (indexing.list_positions(self.labels_now(dim), sel) if by_label
            else self._listed(dim, sel))
    self.keep(dim, np.delete(np.arange(self.current(dim).size), gone))

  def increasing(self, dim: str) -> None:
    if dim not in self.labels:
      raise KeyError(dim)
    x = self.labels_now(dim)
    is_increasing = np.diff(x) > 0
    if np.all(is_increasing):
      return
    if not np.all(~is_increasing):
      raise ValueError(f'Cannot make non-monotonic dimension {dim} increasing')
    self.keep(dim, np.arange(x.size)[::-1])

  def touched(self) -> dict:
    """The dims whose axis is no longer the original one."""
    return {d: p for d, p in self.pos.items()
            if d in self.sizes and not (p.size == self.sizes[d]
                    and np.array_equal(p, np.arange(p.size)))}


def _axes(ds: xl.Dataset) -> tuple:
  """(sizes, labels) of every dim of `ds`: those of its variables and those
  that only a 1-D coordinate of the same name spans."""
  sizes = dict(ds.sizes)
  labels = {}
  for name, c in ds.coords.items():
    if isinstance(c, xl.DataArray):
      if c.dims == (name,):
        labels[name] = np.asarray(c.values)
        sizes.setdefault(name, labels[name].size)
      continue
    c = np.asarray(c)
    if c.ndim == 1:
      labels[name] = c
      sizes.setdefault(name, c.size)
  return sizes, labels


def _compose(ds: xl.Dataset, sel, sel_strings, isel, drop_sel,
             drop_sel_strings, drop_isel, increasing, drop=(), keep=()
             ) -> tuple:
  """(composer, `ds` with its variables dropped or kept) after every step."""
  comp = _Composer(*_axes(ds))
  for dim in _as_names(increasing):
    comp.increasing(dim)
  ds = _select_variables(ds, drop, keep)
  # (a dim or an index that went with the variables cannot be selected on)
  comp.sizes, comp.labels = _axes(ds)
  for selection in get_selections(_as_pairs(isel), force_string=False):
    for dim, s in selection.items():
      comp.isel(dim, s)
  for pairs, force in ((sel, False), (sel_strings, True)):
    for selection in get_selections(_as_pairs(pairs), force_string=force):
      for dim, s in selection.items():
        comp.sel(dim, s)
  for selection in get_selections(_as_pairs(drop_isel), force_string=False):
    for dim, s in selection.items():
      comp.drop(dim, s, False, 'drop_isel')
  for pairs, force, option in ((drop_sel, False, 'drop_sel'),
                               (drop_sel_strings, True, 'drop_sel_strings')):
    for selection in get_selections(_as_pairs(pairs), force_string=force):
      for dim, s in selection.items():
        comp.drop(dim, s, True, option)
  return comp, ds


def compose_positions(ds, *, sel: Selector = None, sel_strings: Selector = None,
                      isel: Selector = None, drop_sel: Selector = None,
                      drop_sel_strings: Selector = None,
                      drop_isel: Selector = None,
                      make_dims_increasing=()) -> dict:
  """{dim: int64 positions into the original axis} of every dim that
  `slice_dataset` with the same options changes: all steps composed, nothing
  moved."""
  return _compose(xl.as_dataset(ds), sel, sel_strings, isel, drop_sel,
                  drop_sel_strings, drop_isel,
                  make_dims_increasing)[0].touched()


def _affine(pos: np.ndarray) -> t.Optional[tuple]:
  """(first, step, count) of positions that form an affine run with a non-zero
  step; None for any other list."""
  n = int(pos.size)
  if n == 0:
    return (0, 1, 0)
  if n == 1:
    return (int(pos[0]), 1, 1)
  step = int(pos[1] - pos[0])
  if step != 0 and bool(np.all(np.diff(pos) == step)):
    return (int(pos[0]), step, n)
  return None


def _outer_reindex(dims, sizes, touched, n_inner: int
                   ) -> t.Optional[indexing.Reindex]:
  """The selection on the dims before the last `n_inner` as one `Reindex` in
  place: per kept position of the touched dims, the C-order position in their
  original grid.  None where no such dim is touched."""
  hit = tuple(d for d in dims[:len(dims) - n_inner] if d in touched)
  if not hit:
    return None
  table = np.zeros([1] * len(hit), dtype=np.int64)
  for ax, d in enumerate(hit):
    shape = [1] * len(hit)
    shape[ax] = touched[d].size
    table = table * sizes[d] + touched[d].reshape(shape)
  return indexing.Reindex(hit, hit, table)


def _plain(da: xl.DataArray, touched: dict):
  """One take per touched dim: host arrays in NumPy, device arrays in torch."""
  data = da.data
  if operands.on_device(data):
    if isinstance(data, (xl.SlabGather, xl.SlabConcat)):
      data = data.materialize()
    for ax, d in enumerate(da.dims):
      if d in touched:
        data = torch.index_select(
            data, ax, torch.as_tensor(touched[d], device=data.device))
    return data
  data = np.asarray(da.values)
  for ax, d in enumerate(da.dims):
    if d in touched:
      data = np.take(data, touched[d], axis=ax)
  return data


def _lazy_slabs(da: xl.DataArray, sizes: dict, re_: indexing.Reindex
                ) -> xl.SlabGather:
  table = indexing.slab_table(da.dims, sizes, da.dims, re_, 2)
  data = da.data
  if isinstance(data, xl.SlabGather):  # a gather of a gather
    return xl.SlabGather(data.base, indexing.compose(table,
                                                     data.index.ravel()))
  if isinstance(data, torch.Tensor):
    data = data.contiguous()  # (the input itself where it is contiguous)
  else:
    data = np.ascontiguousarray(data)
  return xl.SlabGather(data, table)


def _scatter_slabs(da: xl.DataArray, sizes: dict, re_: indexing.Reindex,
                   out_shape: tuple) -> torch.Tensor:
  """Whole slabs of a float32 / float64 device variable through K16, every
  source slab with its one destination."""
  k = indexing.common_tail(da.dims, da.dims, re_)
  if isinstance(da.data, xl.SlabGather):
    k = 2  # (a gather's base is addressed slab by slab)
  device = engine.require_gpu()
  dtype = operands.torch_dtype(da.dtype)
  table = indexing.slab_table(da.dims, sizes, da.dims, re_, k).reshape(-1)
  ten, physical = operands.operand(da, da.dims, device, dtype, k)
  if physical is not None:  # a view or a gather: where the slabs really lie
    table = indexing.compose(table, physical)
  n = table.size
  return engine.slab_scatter(
      ten, np.ascontiguousarray(table, dtype=np.int64),
      (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64)), n,
      n_point=math.prod(out_shape[len(out_shape) - k:]), checked=True)


def _box(da: xl.DataArray, sizes: dict, touched: dict) -> torch.Tensor:
  """A device variable of 4- or 8-byte elements through K17: one launch."""
  dims = da.dims
  device = engine.require_gpu()
  ten, physical = operands.operand(da, dims, device,
                                   operands.torch_dtype(da.dtype), 2)
  re_ = _outer_reindex(dims, sizes, touched, 2)
  table = None if re_ is None else indexing.slab_table(
      dims, sizes, dims, re_, 2).reshape(-1)
  if physical is not None:  # a view or a gather: where the slabs really lie
    table = physical if table is None else indexing.compose(table, physical)
  n_out_slab = math.prod(touched[d].size if d in touched else sizes[d]
                         for d in dims[:-2])
  cols = touched.get(dims[-1])
  return engine.box_gather(
      ten, sizes[dims[-2]], sizes[dims[-1]], src_slab=table,
      n_out_slab=n_out_slab, rows=touched.get(dims[-2]),
      cols=None if cols is None else (_affine(cols) or cols))


def _move(da: xl.DataArray, touched: dict, materialize: bool):
  """The data of `da` with every touched dim cut to its kept positions."""
  dims = da.dims
  if not any(d in touched for d in dims):
    return da.data
  sizes = dict(da.sizes)
  if isinstance(da.data, xl.SlabConcat):
    da = da.copy(da.data.materialize())
  out_shape = tuple(touched[d].size if d in touched else sizes[d]
                    for d in dims)
  device = operands.on_device(da.data)
  dtype = operands.torch_dtype(da.dtype) if device else None
  if not any(d in touched for d in dims[-2:]):  # whole slabs move
    re_ = _outer_reindex(dims, sizes, touched, 2)
    if not materialize:
      return _lazy_slabs(da, sizes, re_)
    if device and (dtype, dtype) in engine.SCATTER_PAIRS:
      if not math.prod(out_shape):
        return torch.empty(out_shape, dtype=dtype,
                           device=engine.require_gpu())
      return _scatter_slabs(da, sizes, re_, out_shape).reshape(out_shape)
    return _plain(da, touched)
  if not materialize:
    raise ValueError(
        f'materialize=False needs the last two dims of {da.name!r} to be a '
        f'slab that is not sliced: its dims are {dims}, '
        f'{tuple(d for d in dims if d in touched)} are sliced')
  if device and len(dims) >= 2 and dtype in engine.BOX_DTYPES:
    return _box(da, sizes, touched).reshape(out_shape)
  return _plain(da, touched)


def _slice_coords(coords: dict, touched: dict) -> dict:
  out = {}
  for name, c in coords.items():
    if isinstance(c, xl.DataArray):
      if any(d in touched for d in c.dims):
        c = xl.DataArray(_plain(c._host(), touched), c.dims, {}, name)
    elif name in touched and np.ndim(c) == 1:
      c = np.asarray(c)[touched[name]]
    out[name] = c
  return out


def _coord_dims(name: str, c) -> tuple:
  if isinstance(c, xl.DataArray):
    return c.dims
  return (name,) if np.ndim(c) == 1 else ()


def _select_variables(ds: xl.Dataset, drop, keep) -> xl.Dataset:
  """`ds.drop_vars(drop)` (data variables or coords) or `ds[keep]` (data
  variables, in the order given, with the coordinates that lie along their
  dims)."""
  if drop:
    missing = [n for n in drop if n not in ds.data_vars and n not in ds.coords]
    if missing:
      raise ValueError(f'These variables cannot be found in this dataset: '
                       f'{missing}')
    coords = {k: c for k, c in ds.coords.items() if k not in drop}
    names = [k for k in ds.data_vars if k not in drop]
  elif keep:
    for n in keep:
      if n not in ds.data_vars:
        raise KeyError(n)
    names = list(keep)
    have = {d for n in names for d in ds.data_vars[n].dims}
    coords = {k: c for k, c in ds.coords.items()
              if all(d in have for d in _coord_dims(k, c))}
  else:
    return ds
  out = xl.Dataset(coords=coords, attrs=ds.attrs)
  for n in names:
    v = ds.data_vars[n]
    out.data_vars[n] = xl.DataArray(v.data, v.dims, out.coords, n)
  return out


def slice_dataset(ds, *, sel: Selector = None, sel_strings: Selector = None,
                  isel: Selector = None, drop_sel: Selector = None,
                  drop_sel_strings: Selector = None,
                  drop_isel: Selector = None, drop_variables=None,
                  keep_variables=None, make_dims_increasing=(),
                  materialize: bool = True):
  """`main` of scripts/slice_dataset.py without IO.  Every selector is the
  flag's string ('time_start=2021-02-01,time_step=5,longitude_step=60') or the
  parsed dict, with keys `<dim>_start`, `<dim>_stop`, `<dim>_step` (a slice)
  or `<dim>_list` ('+'-delimited values); `sel_strings` / `drop_sel_strings`
  keep every value a string (years are sliced as '2000').  The order is the
  script's: make_dims_increasing, drop_variables (data variables or coords) or
  keep_variables (a list or a comma-delimited string each; giving both is a
  ValueError), isel, sel, sel_strings, drop_isel, drop_sel, drop_sel_strings.
  The three drop options take `_list` keys only: an absent label is a
  KeyError, a position out of range an IndexError, negative positions count
  from the end.

  With `materialize=False` nothing moves: a variable that is sliced along
  dims before its last two comes back as a `SlabGather` over the input (read
  in place by MSE and CRPS); slicing one of the last two dims is then a
  ValueError."""
  like = ds
  ds = xl.as_dataset(ds)
  drop, keep = _as_names(drop_variables), _as_names(keep_variables)
  if drop and keep:
    raise ValueError('keep_variables and drop_variables are mutually '
                     'exclusive')
  comp, ds = _compose(ds, sel, sel_strings, isel, drop_sel, drop_sel_strings,
                      drop_isel, make_dims_increasing, drop, keep)
  touched = comp.touched()
  out = xl.Dataset(coords=_slice_coords(ds.coords, touched), attrs=ds.attrs)
  for name, v in ds.data_vars.items():
    out.data_vars[name] = xl.DataArray(_move(v, touched, materialize), v.dims,
                                       out.coords, name)
  return xl.like_input(out, like)


def make_dims_increasing(ds, dims):
  """The script's `_maybe_make_some_dims_increasing`: every dim of `dims` that
  is decreasing is reversed; a dim that is neither is a ValueError."""
  return slice_dataset(ds, make_dims_increasing=dims)
