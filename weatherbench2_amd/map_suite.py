"""`deterministic_spatial` chunk by chunk: SpatialBias / SpatialMSE / SpatialMAE
of every variable of a chunk straight into the running temporal mean.

Reference: scripts/evaluate.py:431-435, 471-478 (the config: three map metrics,
no regions, Zarr output), weatherbench2/metrics.py:304-374 (the maps),
evaluation.py:583-599 + 735-744 (per chunk, then `xbeam.Mean` over init_time).
The reference materialises three full-size maps per chunk and variable and
hands them to the combiner.  The generic path of this package does the same on
the device (wb2_spatial_maps, the `metric` concat, wb2_time_accumulate_runs:
~150 B of HBM traffic per grid point).  Chunks of one evaluation share their
structure, so -- like program.py does for the scalar metrics -- the first chunk
of a structure goes through the generic path (it creates the accumulators and
fixes dims, coordinates and dtypes of the result) and every later one through
ONE launch of wb2_spatial_accumulate_addr: forecast and truth are read once
(8 B per point) and d, d^2, |d| are added to the three running sums where they
live (48 B per point), value by value in time order -- the bits of the generic
path.  Without skipna the step counts stay on the host until result().
"""
from __future__ import annotations

import typing as t

import numpy as np
import torch

from weatherbench2_amd import _lib, engine
from weatherbench2_amd import metrics as gm
from weatherbench2_amd import xarray_lite as xl

_KINDS = {gm.SpatialBias: 0, gm.SpatialMSE: 1, gm.SpatialMAE: 2}


def applies(eval_config) -> bool:
  """The `deterministic_spatial` config: the three map metrics (each at most
  once, at least one), optionally SpatialSEEPS entries (`--compute_seeps`:
  maps of their precipitation variable only), no regions, no derived
  variables, a temporal mean."""
  metrics = getattr(eval_config, 'metrics', None) or {}
  kinds = [_KINDS.get(type(m)) for m in metrics.values()]
  fused = [k for k in kinds if k is not None]
  others = [m for m, k in zip(metrics.values(), kinds) if k is None]
  return bool(fused) and len(set(fused)) == len(fused) and all(
      type(m) is gm.SpatialSEEPS for m in others) and (
          not getattr(eval_config, 'regions', None)) and (
              not getattr(eval_config, 'derived_variables', None)) and getattr(
                  eval_config, 'temporal_mean', True)


class MapSuite:
  """The replayable form of one chunk structure of a map-metric config."""

  def __init__(self, variables, kinds, time_dim, split_dim, skipna, device,
               extras=(), fills=None):
    self.variables = variables   # [(name, result dims, result shape)]
    # metric index -> 0 bias / 1 mse / 2 mae, None for the others
    self.kinds = kinds
    # [(variable, metric index, metric)]: map metrics of single variables
    # (SpatialSEEPS), computed by the metric itself and accumulated per slab
    self.extras = list(extras)
    # variable -> metric indices it has no values for (NaN in the merged
    # result, evaluation.py:424-437): their sums are NaN from the first step
    self.fills = dict(fills or {})
    self._nan_rows: dict = {}    # variable -> rows whose fills are NaN
    self.time_dim, self.split_dim = time_dim, split_dim
    self.skipna, self.device = bool(skipna), device
    self._lib = _lib.load()
    self._plan = None   # _Plan of the structure, after the first run
    self._keep = None
    self._const: dict = {}  # variable -> (offsets [metric][dst], lead, block)
    self._fast_extras: dict = {}  # (variable, metric index) -> _FastSeeps
    self._times_memo: dict = {}

  def reset(self):
    pass

  def _offsets(self, acc, dims, shape, order, rows) -> np.ndarray:
    """[metric][destination]: first accumulator element of the slab of
    (metric m, the chunk's non-time dims in `order`)."""
    block = int(np.prod(acc.rest_shape, dtype=np.int64))
    rest_dims = [d for d in acc.dims if d != acc.split]
    stride, step = {}, 1
    for d, n in zip(reversed(rest_dims), reversed(acc.rest_shape)):
      stride[d] = step
      step *= n
    lead_dims = ['metric'] + list(order)
    sizes = [shape[dims.index(d)] for d in lead_dims]
    off = np.zeros(sizes, dtype=np.int64)
    for ax, d in enumerate(lead_dims):
      where = [1] * len(lead_dims)
      where[ax] = sizes[ax]
      if acc.split is not None and d == acc.split:
        part = rows * block
      else:
        part = np.arange(sizes[ax], dtype=np.int64) * stride[d]
      off = off + part.reshape(where)
    return off.reshape(sizes[0], -1)

  def run(self, forecast: xl.Dataset, truth: xl.Dataset, mean) -> None:
    plan = self._plan
    if plan is not None and plan.matches(forecast, truth):
      groups = plan.tables(forecast, truth, mean, self)
    else:
      groups, self._plan = self._first(forecast, truth, mean)
    self._launch(groups)
    self._fill(mean)
    for name, m, metric in self.extras:
      self._extra(name, m, metric, forecast, truth, mean)

  def run_many(self, pairs, mean) -> None:
    """k chunks that carry the SAME lead labels, in chunk order, as ONE
    launch: the running sums of their destinations are loaded once, the k
    chunks' time steps added one after the other in chunk order, and stored --
    the additions of k runs of `run`, in the same order: the same bits, at
    (8 k + 48) / k instead of 56 bytes of HBM traffic per grid point and
    chunk (xbeam.Mean combines any number of chunks per key before it touches
    the output, evaluation.py:735-744)."""
    plan = self._plan
    if len(pairs) == 1 or plan is None or not all(
        plan.matches(f, t_) for f, t_ in pairs):
      for f, t_ in pairs:
        self.run(f, t_, mean)
      return
    per_chunk = [plan.tables(f, t_, mean, self) for f, t_ in pairs]
    groups = {}
    last = per_chunk[-1]   # (a row met by a later chunk may have grown the
    for key in last:       #  accumulators: the addresses of the last table)
      fa = np.concatenate([tab[key][0] for tab in per_chunk], axis=0)
      ta = np.concatenate([tab[key][1] for tab in per_chunk], axis=0)
      dtype, n_point, _ = key
      groups[(dtype, n_point, fa.shape[0])] = (fa, ta, last[key][2],
                                               last[key][3])
    self._launch(groups)
    self._fill(mean)
    for name, m, metric in self.extras:
      fast = self._fast_extras.get((name, m))
      if fast and all(fast.matches(f, t_) for f, t_ in pairs):
        fast.run_many(pairs, mean)   # one map launch + one accumulate
      else:
        for f, t_ in pairs:
          self._extra(name, m, metric, f, t_, mean)

  def _fill(self, mean):
    """Without skipna a metric that lacks the variable leaves NaN sums (NaN
    maps were added): rows this suite meets first get them here."""
    if self.skipna:
      return
    for name, ms in self.fills.items():
      acc = mean._acc[name]
      if acc.split is None:
        continue   # (the generic first chunk has written them)
      done = self._nan_rows.setdefault(name, set())
      for row in set(acc.row_of.values()) - done:
        for m in ms:
          acc.total[row, m] = float('nan')
        done.add(row)

  def _extra(self, name, m, metric, forecast, truth, mean):
    """A single-variable map metric (SpatialSEEPS): its own chunk map, added to
    the slabs of (metric m, variable) -- one destination entry per slab."""
    fast = self._fast_extras.get((name, m))
    if fast is None:
      # the generic way below once per structure, then what it did replayed
      # from the chunk's pointers and valid times (two C-ABI calls per chunk)
      self._fast_extras[(name, m)] = _FastSeeps.build(
          self, name, m, metric, forecast, truth) or False
    elif fast and fast.matches(forecast, truth):
      return fast.run(forecast, truth, mean)
    ds = metric.compute_chunk(forecast, truth)
    da = ds[name]
    const, lead, block, n_point = self._const[name]
    acc = mean._acc[name]
    rows = 0
    if acc.split is not None:
      rows = acc.rows(np.asarray(forecast.coords[acc.split]))[lead]
    dst = engine.upload_table(rows * block + const[m], self.device,
                              cache=False)
    engine.order_read(da.data)
    engine.time_accumulate(da.data, da.dims.index(self.time_dim), self.skipna,
                           acc.total, acc.count if self.skipna else None, dst,
                           n_point)

  def _first(self, forecast, truth, mean):
    """The address tables of one chunk from scratch (label work, views, slab
    tables) + what of them the next chunk of the structure can reuse."""
    device = self.device
    groups: dict = {}
    keep, parts, reusable = [], [], True
    for vi, (name, dims, shape) in enumerate(self.variables):
      fvar, tvar = forecast[name], truth[name]
      geo, prepared = gm._geometry(forecast, fvar, [tvar])
      order = tuple(d for d in geo.out_dims if d != self.time_dim)
      full = (self.time_dim,) + order
      sizes = tuple(geo.out_shape[geo.out_dims.index(d)] for d in full)
      if tuple(d for d in dims[1:-2] if d != self.time_dim) != order:
        raise ValueError(f'{name}: chunk layout changed')
      tables = [gm._slab_table(full, sizes, p[1], p[0].shape[:-2])
                for p in prepared]
      tensors, tables, dtype = gm._prepare_inputs(
          geo, [p[0] for p in prepared], tables, device)
      n_row, n_col = (len(geo.latitude), len(geo.longitude))
      if geo.layout != gm.plan_lib.LATLON:
        n_row, n_col = n_col, n_row
      n_outer = int(np.prod(sizes, dtype=np.int64))
      addr, rel = [], []
      for x, tb, src in zip(tensors, tables, (fvar.data, tvar.data)):
        a, alive = gm._slab_addresses(x, tb, n_row, n_col, n_outer)
        a = np.asarray(a, dtype=np.int64).reshape(sizes[0], -1)
        addr.append(a)
        keep.append(alive)
        # the next chunk's addresses are its base + the same offsets when the
        # slabs are read from the chunk's own (device) array
        inside = isinstance(src, torch.Tensor) and src.is_cuda and a.size and (
            _inside(src, int(a.min()), int(a.max())))
        reusable = reusable and bool(inside)
        rel.append(a - src.data_ptr() if inside else None)
      acc = mean._acc[name]
      rows = None
      if acc.split is not None:
        rows = acc.rows(np.asarray(forecast.coords[acc.split]))
      chunk_shape = tuple(
          sizes[full.index(d)] if d in full else n
          for d, n in zip(dims, shape))
      zero = None if rows is None else np.zeros_like(rows)
      const = self._offsets(acc, dims, chunk_shape, order, zero)
      block = int(np.prod(acc.rest_shape, dtype=np.int64))
      n_dst = const.shape[1]
      lead = np.zeros(n_dst, dtype=np.int64)
      if rows is not None:
        where = [1] * len(order)
        where[order.index(acc.split)] = len(rows)
        lead = np.broadcast_to(
            np.arange(len(rows), dtype=np.int64).reshape(where),
            [sizes[full.index(d)] for d in order]).ravel()
      by_kind = np.full((3, n_dst), -1, dtype=np.int64)
      for m, kind in enumerate(self.kinds):
        if kind is not None:
          by_kind[kind] = const[m]
      key = (dtype, n_row * n_col, sizes[0])
      parts.append((key, vi, name, rel, by_kind, lead, block, rows is not None,
                    _layout(fvar.data), _layout(tvar.data)))
      self._const[name] = (const, lead, block, n_row * n_col)
      g = groups.setdefault(key, [[], [], [], []])
      row_of_dst = 0 if rows is None else rows[lead]
      live = by_kind >= 0
      off = row_of_dst * block + by_kind
      g[0].append(addr[0])
      g[1].append(addr[1])
      g[2].append(np.where(live, acc.total.data_ptr() + 8 * off, 0))
      g[3].append(np.where(live, acc.count.data_ptr() + 8 * off, 0)
                  if self.skipna else np.zeros_like(off))
      self._count_steps(acc, rows, sizes[0])
    out = {k: tuple(np.concatenate(x, axis=1) for x in g)
           for k, g in groups.items()}
    self._keep = keep  # alive until the launches below are enqueued
    return out, (_Plan(parts) if reusable else None)

  def _count_steps(self, acc, rows, n_time: int):
    if not self.skipna:
      for row in ([None] if rows is None else rows.tolist()):
        acc.pending[row] = acc.pending.get(row, 0) + n_time

  def _launch(self, groups: dict):
    device = self.device
    stream = engine.current_stream_ptr(device)
    for (dtype, n_point, n_time), (fa, ta, sa, ca) in groups.items():
      n_dst = fa.shape[1]
      width = 16 // torch.empty((), dtype=dtype).element_size()
      aligned = n_point % width == 0 and not (
          (fa & 15).any() or (ta & 15).any())
      table = engine.upload_table(
          np.concatenate([fa.ravel(), ta.ravel(), sa.ravel(), ca.ravel()]),
          device, cache=False)
      n = n_time * n_dst
      base = table.data_ptr()
      engine.hooked_call(
          'spatial_accumulate', self._lib.wb2_spatial_accumulate_addr,
          'wb2_spatial_accumulate_addr', engine.dtype_code(dtype),
          int(self.skipna), int(aligned), base, base + 8 * n, n_time, n_dst,
          n_point, base + 16 * n,
          (base + 16 * n + 24 * n_dst) if self.skipna else None, stream)
    self._keep = None  # the launches are enqueued: the allocator orders reuse


class _FastSeeps:
  """One SpatialSEEPS entry of a map suite for the later chunks of a
  structure: metrics.SpatialSEEPS.compute_chunk + engine.time_accumulate as
  two C-ABI calls on recorded arguments (wb2_seeps_map into a buffer of its
  own, wb2_time_accumulate_runs into the running sums) -- the generic path's
  kernels on the generic path's arguments, so its bits.  Per chunk: the
  precipitation arrays' pointers, the wet-threshold slab of every valid time
  (metrics._climatology_gather), the accumulator rows of the lead labels."""

  @classmethod
  def build(cls, suite, name, m, metric, forecast, truth):
    try:
      return cls(suite, name, m, metric, forecast, truth)
    except (ValueError, KeyError, TypeError):
      return None

  def __init__(self, suite, name, m, metric, forecast, truth):
    if type(metric) is not gm.SpatialSEEPS or suite.time_dim is None:
      raise ValueError('not a SpatialSEEPS entry')
    f, t_ = gm._inputs(forecast, truth)
    geo, arrays, tables, aux = metric._prepare(f, t_)
    fdata, tdata, wdata = arrays
    if tables[0] is not None or tables[1] is not None:
      raise ValueError('forecast / truth are read through a slab table')
    for x in (fdata, tdata, wdata):
      if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous()):
        raise ValueError('an input is not a contiguous device tensor')
    if not (fdata.dtype == tdata.dtype == wdata.dtype):
      raise ValueError('inputs differ in dtype')
    self.code = engine.dtype_code(fdata.dtype)  # (TypeError: no such kernel)
    if fdata is not f[name].data or tdata is not t_[name].data:
      raise ValueError('the pass read a copy of the chunk')
    climatology = xl.as_dataset(metric.climatology)
    wvar = climatology[f'{name}_seeps_threshold']
    wrest = tuple(d for d in wvar.dims if d not in gm._SPATIAL)
    self.gather = gm._climatology_gather(climatology, wvar, f, geo, wrest)
    self.suite, self.name, self.m = suite, name, m
    self.layouts = (_layout(fdata), _layout(tdata))
    self.n_outer = geo.n_outer
    self.n_point = int(fdata.shape[-2]) * int(fdata.shape[-1])
    self.slab_bytes = self.n_point * fdata.element_size()
    self.wet = wdata
    self.aux = gm._resident_aux(aux, suite.device).reshape(-1)
    self.scalar = float(metric.dry_threshold_mm / 1000.0)
    self.out = torch.empty((self.n_outer, self.n_point), dtype=torch.float64,
                           device=suite.device)
    self._outs: dict = {}   # chunks per launch -> map buffer (run_many)
    # the map as the metric hands it over: out_dims + the two spatial dims
    axis = geo.out_dims.index(suite.time_dim)
    shape = tuple(geo.out_shape)
    self.n_lead = int(np.prod(shape[:axis], dtype=np.int64))
    self.n_time = int(shape[axis])
    self.n_tail = int(np.prod(shape[axis + 1:], dtype=np.int64)) * self.n_point
    self._lib = _lib.load()

  def matches(self, forecast, truth) -> bool:
    return (_layout(forecast[self.name].data) == self.layouts[0] and
            _layout(truth[self.name].data) == self.layouts[1])

  def run(self, forecast, truth, mean) -> None:
    import ctypes
    suite, lib = self.suite, self._lib
    dev = suite.device
    stream = engine.current_stream_ptr(dev)
    g = self.gather
    memo = suite._times_memo   # (the chunk's valid times: once per chunk for
    if memo.get('of') is not forecast:   # all SpatialSEEPS entries)
      memo.clear()
      memo['of'] = forecast
    table = g['values'](forecast, memo)[g['cell']] + g['base']
    wet_ptr, wet_tab = self.wet.data_ptr(), None
    if self.n_outer == 1:   # one slab: its address, no table to upload
      wet_ptr += int(table[0]) * self.slab_bytes
    else:
      wet_tab = engine.upload_table(table, dev)
    ins = (ctypes.c_void_p * 3)(forecast[self.name].data.data_ptr(),
                                truth[self.name].data.data_ptr(), wet_ptr)
    tabs = (ctypes.c_void_p * 3)(None, None, _lib.ptr(wet_tab) or None)
    status = lib.wb2_seeps_map(self.code, ins, tabs, self.n_outer,
                               self.n_point, self.aux.data_ptr(), self.scalar,
                               self.out.data_ptr(), stream)
    if status != 0:
      _lib.check(status, 'wb2_seeps_map')
    const, lead, block, n_point = suite._const[self.name]
    acc = mean._acc[self.name]
    rows = 0
    if acc.split is not None:
      rows = acc.rows(np.asarray(forecast.coords[acc.split]))[lead]
    dst = engine.upload_table(rows * block + const[self.m], dev)
    status = lib.wb2_time_accumulate_runs(
        _lib.WB2_F64, self.out.data_ptr(), self.n_lead, self.n_time,
        self.n_tail, int(suite.skipna), dst.data_ptr(), n_point,
        acc.total.data_ptr(),
        acc.count.data_ptr() if suite.skipna else None, stream)
    if status != 0:
      _lib.check(status, 'wb2_time_accumulate_runs')


  def run_many(self, pairs, mean) -> None:
    """The k chunks of a window that carry the same lead labels: ONE
    wb2_seeps_map_addr launch over the slabs of all of them (by address) and
    ONE wb2_time_accumulate_runs that adds the k chunks' time steps in chunk
    order -- the additions of k calls of `run`, in the same order."""
    import ctypes
    suite, lib = self.suite, self._lib
    dev = suite.device
    stream = engine.current_stream_ptr(dev)
    k, n = len(pairs), self.n_outer
    g = self.gather
    memo = suite._times_memo
    addr = np.empty((3, k, n), dtype=np.int64)
    own = np.arange(n, dtype=np.int64) * self.slab_bytes
    for c, (forecast, truth) in enumerate(pairs):
      if memo.get('of') is not forecast:
        memo.clear()
        memo['of'] = forecast
      table = g['values'](forecast, memo)[g['cell']] + g['base']
      addr[0, c] = forecast[self.name].data.data_ptr() + own
      addr[1, c] = truth[self.name].data.data_ptr() + own
      addr[2, c] = self.wet.data_ptr() + table * self.slab_bytes
    # a chunk's slabs run (lead part, time, tail); the launch writes them as
    # (lead part, chunk, time, tail): k chunks = k x n_time steps of one run
    tail = self.n_tail // self.n_point
    addr = addr.reshape(3, k, self.n_lead, self.n_time, tail).transpose(
        0, 2, 1, 3, 4)
    tab = engine.upload_table(np.ascontiguousarray(addr).ravel(), dev)
    out = self._outs.get(k)
    if out is None:
      out = self._outs[k] = torch.empty((k * n, self.n_point),
                                        dtype=torch.float64, device=dev)
    base = tab.data_ptr()
    tabs = (ctypes.c_void_p * 3)(base, base + 8 * k * n, base + 16 * k * n)
    status = lib.wb2_seeps_map_addr(self.code, tabs, k * n, self.n_point,
                                    self.aux.data_ptr(), self.scalar,
                                    out.data_ptr(), stream)
    if status != 0:
      _lib.check(status, 'wb2_seeps_map_addr')
    forecast = pairs[-1][0]
    const, lead, block, n_point = suite._const[self.name]
    acc = mean._acc[self.name]
    rows = 0
    if acc.split is not None:
      rows = acc.rows(np.asarray(forecast.coords[acc.split]))[lead]
    dst = engine.upload_table(rows * block + const[self.m], dev)
    status = lib.wb2_time_accumulate_runs(
        _lib.WB2_F64, out.data_ptr(), self.n_lead, k * self.n_time,
        self.n_tail, int(suite.skipna), dst.data_ptr(), n_point,
        acc.total.data_ptr(),
        acc.count.data_ptr() if suite.skipna else None, stream)
    if status != 0:
      _lib.check(status, 'wb2_time_accumulate_runs')


def _inside(x: torch.Tensor, lo: int, hi: int) -> bool:
  store = x.untyped_storage()
  return store.data_ptr() <= lo and hi < store.data_ptr() + store.nbytes()


def _layout(x) -> tuple:
  if isinstance(x, torch.Tensor):
    return (tuple(x.shape), tuple(x.stride()), x.dtype, x.device)
  return (type(x).__name__,)


class _Plan:
  """What the chunks of one structure share: every slab's offset from its
  array's base, every destination's offset inside its accumulator row."""

  def __init__(self, parts):
    self.parts = parts
    self.names = [p[2] for p in parts]
    self.layouts = [(p[8], p[9]) for p in parts]
    self.groups = {}
    for key, vi, name, rel, by_kind, lead, block, split, _, _ in parts:
      g = self.groups.setdefault(key, {'vi': [], 'rel_f': [], 'rel_t': [],
                                       'kind': [], 'lead': [], 'block': []})
      n_dst = by_kind.shape[1]
      g['vi'].append(np.full(n_dst, vi, dtype=np.int64))
      g['rel_f'].append(rel[0])
      g['rel_t'].append(rel[1])
      g['kind'].append(by_kind)
      g['lead'].append(lead)
      g['block'].append(np.full(n_dst, block, dtype=np.int64))
    for g in self.groups.values():
      g['vi'] = np.concatenate(g['vi'])
      g['rel_f'] = np.concatenate(g['rel_f'], axis=1)
      g['rel_t'] = np.concatenate(g['rel_t'], axis=1)
      g['kind'] = np.concatenate(g['kind'], axis=1)
      g['live'] = g['kind'] >= 0
      g['lead'] = np.concatenate(g['lead'])
      g['block'] = np.concatenate(g['block'])

  def matches(self, forecast, truth) -> bool:
    for name, (lf, lt) in zip(self.names, self.layouts):
      if _layout(forecast[name].data) != lf or _layout(truth[name].data) != lt:
        return False
    return True

  def tables(self, forecast, truth, mean, suite) -> dict:
    n_var = len(self.parts)
    base_f = np.empty(n_var, dtype=np.int64)
    base_t = np.empty(n_var, dtype=np.int64)
    total = np.empty(n_var, dtype=np.int64)
    count = np.empty(n_var, dtype=np.int64)
    rows_of = [None] * n_var
    n_lead = 1
    for key, vi, name, _, _, _, _, split, _, _ in self.parts:
      acc = mean._acc[name]
      base_f[vi] = forecast[name].data.data_ptr()
      base_t[vi] = truth[name].data.data_ptr()
      if split:
        rows_of[vi] = acc.rows(np.asarray(forecast.coords[acc.split]))
        n_lead = max(n_lead, len(rows_of[vi]))
      total[vi] = acc.total.data_ptr()   # (after rows(): it may have grown)
      count[vi] = acc.count.data_ptr() if suite.skipna else 0
      suite._count_steps(acc, rows_of[vi], key[2])
    rows = np.zeros((n_var, n_lead), dtype=np.int64)
    for vi, r in enumerate(rows_of):
      if r is not None:
        rows[vi, :len(r)] = r
    out = {}
    for key, g in self.groups.items():
      vi = g['vi']
      off = rows[vi, g['lead']] * g['block'] + g['kind']
      out[key] = (base_f[vi] + g['rel_f'], base_t[vi] + g['rel_t'],
                  np.where(g['live'], total[vi] + 8 * off, 0),
                  np.where(g['live'], count[vi] + 8 * off, 0))
    return out


def build(eval_config, forecast: xl.Dataset, truth: xl.Dataset, result,
          mean, skipna) -> t.Optional[MapSuite]:
  """The map suite of the structure of (forecast, truth), after the generic
  pass over it (`result`, already added to `mean`); None when the config or
  the result layout is not the one described in the module docstring (why:
  program.REASONS)."""
  from weatherbench2_amd.program import _no
  if not applies(eval_config) or getattr(mean, 'keeps_time', False):
    return _no('map suite: not a map-metric config with a temporal mean')
  result = xl.as_dataset(result)
  labels = result.coords.get('metric')
  # (the merge of the per-metric results sorts the labels: map by name)
  if labels is None or sorted(labels) != sorted(eval_config.metrics):
    return _no(f'map suite: metric labels {labels}')
  labels = [str(k) for k in labels]
  kinds = [_KINDS.get(type(eval_config.metrics[k])) for k in labels]
  variables, extras, fills = [], [], {}
  device = None
  for name, da in result.data_vars.items():
    acc = mean._acc.get(name)
    dims = tuple(da.dims)
    if acc is None or name not in forecast or name not in truth:
      return _no(f'map suite: {name} has no accumulator / input')
    if (len(dims) < 4 or dims[0] != 'metric' or mean.dim not in dims[1:-2]
        or set(dims[-2:]) != set(gm._SPATIAL)):
      return _no(f'map suite: {name} dims {dims}')
    if acc.dims != tuple(d for d in dims if d != mean.dim) or (
        acc.split not in (None, mean.split_dim)):
      return _no(f'map suite: {name} accumulator {acc.dims} split {acc.split}')
    if not isinstance(da.data, torch.Tensor) or not da.data.is_cuda:
      return _no(f'map suite: {name} is {type(da.data).__name__}')
    device = da.data.device
    variables.append((name, dims, tuple(da.shape)))
    for m, (label, kind) in enumerate(zip(labels, kinds)):
      if kind is not None:
        continue
      metric = eval_config.metrics[label]
      if metric.precip_name == name:
        extras.append((name, m, metric))
      elif bool(torch.isnan(da.data[m]).all().item()):
        fills.setdefault(name, []).append(m)
      else:
        return _no(f'map suite: {label} has values for {name}')
  if not variables or set(result.data_vars) != set(
      gm._common_vars(forecast, truth)):
    return _no('map suite: result variables differ from the common variables')
  suite = MapSuite(variables, kinds, mean.dim, mean.split_dim, skipna, device,
                   extras, fills)
  # every accumulator row that exists was written by the generic path
  for name in fills:
    suite._nan_rows[name] = set(mean._acc[name].row_of.values())
  return suite
