"""Launch layer: torch tensors (device memory, streams) -> C-ABI kernels.

PyTorch is plumbing here: it owns HBM allocations and the current HIP stream;
every FLOP of the hot path runs in libwb2hip.so.
"""
from __future__ import annotations

import ctypes
import math
import operator
import os
import threading
import typing as t

import numpy as np
import torch

from weatherbench2_amd import _lib
from weatherbench2_amd.plan import ReductionPlan

_DTYPES = {torch.float32: _lib.WB2_F32, torch.float64: _lib.WB2_F64}
_FIELD_F32_MODES = (_lib.MODE_DET, _lib.MODE_DET_ACC, _lib.MODE_WIND)

_STAGED_UPLOAD_MIN_BYTES = 1 << 20

# Profiling hook (bench.py, tools/): called as hook('begin' | 'end', kernel) on
# the launch stream around the dominant kernel of a pass.  None in production.
_LAUNCH_HOOK = None


def set_launch_hook(hook):
  """Installs (or clears, with None) the profiling hook; returns the old one."""
  global _LAUNCH_HOOK
  old, _LAUNCH_HOOK = _LAUNCH_HOOK, hook
  return old


def hooked_call(kernel: str, fn, what: str, *args) -> None:
  """THE hook bracket: the bound library function `fn` called between the
  hook's 'begin' and 'end' of `kernel`; a nonzero return raises in the name of
  `what` and sends no 'end' (a failed launch leaves the bracket open)."""
  hook = _LAUNCH_HOOK
  if hook is not None:
    hook('begin', kernel)
  status = fn(*args)
  if status != 0:
    _lib.check(status, what)
  if hook is not None:
    hook('end', kernel)


def _launch(kernel: str, c_name: str, *args) -> None:
  """`hooked_call` of the entry point named `c_name`."""
  hooked_call(kernel, getattr(_lib.load(), c_name), c_name, *args)


def dtype_code(dtype: torch.dtype) -> int:
  """The C ABI's code (WB2_F32 / WB2_F64) of one of the kernels' dtypes."""
  try:
    return _DTYPES[dtype]
  except KeyError:
    raise TypeError(f'unsupported dtype {dtype}') from None


def _require_float(*tensors) -> None:
  """The tensors (None: absent) share one of the kernels' two dtypes."""
  first = tensors[0]
  if first.dtype not in _DTYPES or any(
      x is not None and x.dtype != first.dtype for x in tensors):
    raise TypeError('the input must be float32 or float64' if len(tensors) == 1
                    else 'inputs must share a float32/float64 dtype')


def _check_slab(slab, n: int, what: str) -> None:
  """A slab table is None or `n` int64; `what` spells n in the message."""
  if slab is not None and (slab.dtype != torch.int64 or slab.numel() != n):
    raise ValueError(f'the slab table must hold {what} int64')


def _check_contiguous(device, where: str, *tensors, view=None) -> None:
  """The tensors are contiguous on `device` (`where` names it in the message);
  `view` only has to live there: a strided tensor whose intact slabs the
  caller addresses one by one."""
  ok = view is None or view.device == device
  for x in tensors:
    ok = ok and x.device == device and x.is_contiguous()
  if not ok:
    raise ValueError(f'inputs must be contiguous on {where}')


_I32 = ctypes.c_int32


def _geometry(c_name: str, ins, outs) -> dict:
  """{name: value} of the out-parameters `outs` = [(name, ctypes type)], in
  order, of the geometry entry point `c_name` called with the integers `ins`
  (a pointer has no value and is returned as it is)."""
  vals = [ctype() for _, ctype in outs]
  _lib.check(getattr(_lib.load(), c_name)(
      *ins, *[ctypes.byref(v) for v in vals]), c_name)
  return {name: getattr(v, 'value', v) for (name, _), v in zip(outs, vals)}


def current_stream_ptr(device) -> int:
  return torch.cuda.current_stream(device).cuda_stream


class _ThreadStreams(threading.local):

  def __init__(self):
    self.streams: dict = {}
    self.disabled = False


_THREAD_STREAMS = _ThreadStreams()


def disable_thread_stream() -> None:
  """The calling thread keeps the default / caller's stream for good (IO helper
  threads -- evaluation._prefetched -- whose uploads the main thread consumes:
  a private stream there would order nothing with the consumer)."""
  _THREAD_STREAMS.disabled = True


def _own_stream(device: torch.device):
  return _THREAD_STREAMS.streams.get((device.type, device.index))


def _adopt_thread_stream(device: torch.device) -> None:
  """Worker threads (Beam's DirectRunner calls compute_chunk from several,
  evaluation.py:583-599; ctypes releases the GIL) get a HIP stream of their own
  as their torch *current* stream the first time they reach the GPU path:
  everything such a thread launches, allocates and reads back is then ordered
  on its stream, and the passes of different threads overlap on the device
  instead of queueing on the shared default stream.

  Hand-offs between threads are ordered through the default stream:
    * every ENTRY to the GPU path (`require_gpu`) makes the own stream wait for
      what the default stream has queued -- inputs the main thread produced or
      made resident at any time before, and whatever other workers published;
    * `publish_thread_stream` (the exit of the outermost chunk scope, i.e. the
      moment results leave the pass) makes the default stream wait for the own
      stream, so a result read on the main thread, or on another worker (whose
      reads wait for the default stream, `order_read`), sees finished kernels.
  The main thread keeps the caller's stream.  WB2HIP_THREAD_STREAMS=0 disables."""
  if threading.current_thread() is threading.main_thread():
    return
  st = _THREAD_STREAMS
  key = (device.type, device.index)
  if key not in st.streams:
    if st.disabled or os.environ.get('WB2HIP_THREAD_STREAMS', '1') == '0':
      st.streams[key] = None
    else:
      own = torch.cuda.Stream(device=device)
      torch.cuda.set_stream(own)
      st.streams[key] = own
  own = st.streams[key]
  if own is not None:
    own.wait_stream(torch.cuda.default_stream(device))


def publish_thread_stream() -> None:
  """Results of this (worker) thread's stream become visible to the default
  stream: called when the outermost chunk scope of a pass exits."""
  for (kind, index), own in _THREAD_STREAMS.streams.items():
    if own is not None:
      torch.cuda.default_stream(torch.device(kind, index)).wait_stream(own)


def order_read(tensor: torch.Tensor) -> None:
  """Before a device result is read (`.values`, RunningMean.add): a reader on a
  private stream waits for what has been published on the default stream, and
  the read is recorded with the allocator (cross-stream block reuse)."""
  if not tensor.is_cuda:
    return
  dev = tensor.device
  cur = torch.cuda.current_stream(dev)
  default = torch.cuda.default_stream(dev)
  if cur != default:
    cur.wait_stream(default)
  # The reader's stream is (in general) not the stream the result was
  # allocated on -- a worker's private stream -- and `wait_stream` orders
  # visibility only: the caching allocator hands a freed block back to its
  # OWN stream at once, where the worker's next pass could overwrite it while
  # this read is still queued here.  Recording the use makes the allocator
  # wait for this stream before it reuses the block (a no-op when the streams
  # are the same).
  tensor.record_stream(cur)


def require_gpu() -> torch.device:
  if not torch.cuda.is_available():
    raise _lib.Wb2HipError(
        'no HIP device visible: the MI355X path has no CPU fallback')
  device = torch.device('cuda', torch.cuda.current_device())
  _adopt_thread_stream(device)
  return device


def as_device_tensor(x, device, dtype=None) -> torch.Tensor:
  """numpy / torch / DLPack-capable array -> contiguous tensor on `device`."""
  if isinstance(x, torch.Tensor):
    ten = x
  elif isinstance(x, np.ndarray):
    if not x.dtype.isnative:
      x = x.astype(x.dtype.newbyteorder('='))
    if (device.type == 'cuda' and x.nbytes >= _STAGED_UPLOAD_MIN_BYTES
        and (dtype is None or torch.from_numpy(np.empty(0, x.dtype)).dtype
             == dtype)):
      # big host chunks cross PCIe through the pinned staging ring on the copy
      # stream (feeder.py) instead of a pageable, synchronous cudaMemcpy
      from weatherbench2_amd import feeder
      return feeder.upload(x, device)
    ten = torch.from_numpy(np.ascontiguousarray(x))
  elif hasattr(x, '__dlpack__'):
    ten = torch.from_dlpack(x)
  else:
    ten = torch.as_tensor(np.asarray(x))
  if dtype is not None and ten.dtype != dtype:
    ten = ten.to(dtype)
  if ten.device != device:
    ten = ten.to(device, non_blocking=True)
  return ten.contiguous()


def digest(buf: np.ndarray) -> bytes:
  """Content digest of a contiguous numeric array (xxh3 when importable --
  GB/s --, blake2b otherwise)."""
  buf = np.ascontiguousarray(buf)
  if buf.size == 0:  # memoryview cannot cast shapes with zeros
    return b'empty:' + repr((buf.shape, buf.dtype.str)).encode()
  raw = memoryview(buf.reshape(-1)).cast('B')
  try:
    import xxhash
    return xxhash.xxh3_128_digest(raw)
  except ImportError:
    import hashlib
    return hashlib.blake2b(raw, digest_size=16).digest()


class _TableUploads(threading.local):
  """Per-thread, per-device: content cache of uploaded int64 tables + a small
  pinned ring for the misses."""

  def __init__(self):
    self.cache: dict = {}   # (device, shape, digest) -> (device tensor, event)
    self.ring: dict = {}    # device -> [pinned slots, events, next]


_TABLES = _TableUploads()
_TABLE_SLOT_BYTES = 1 << 18
# A slot is reused when the copy out of it has run: with 8 slots the host was
# held at 8 tables ahead of the device -- a window of the map suite uploads 20
_TABLE_SLOTS = int(os.environ.get('WB2HIP_TABLE_SLOTS', 32))


def upload_table(table: np.ndarray, device, cache: bool = True) -> torch.Tensor:
  """int64 slab table -> device tensor WITHOUT stalling the queue.

  `torch.from_numpy(t).to(device)` is a synchronous pageable copy: with kernels
  queued ahead the host blocks until the GPU has drained, once per table and
  call.  Tables recur (same chunk geometry, same valid times), so they are
  cached by a digest of their content; a miss goes through a pinned slot with
  an asynchronous copy on the current stream of `device`, and the event of that
  copy stays with the cache entry: a hit under a different current stream
  (`torch.cuda.stream(...)`) waits for it before the table is read."""
  table = np.ascontiguousarray(table, dtype=np.int64)
  device = torch.device(device)
  st = _TABLES
  key = None
  if cache:  # (cache=False: a table that will not come again -- addresses)
    key = (str(device), table.shape, digest(table))
    hit = st.cache.get(key)
    if hit is not None:
      dev, ev = hit
      if ev is not None:
        torch.cuda.current_stream(device).wait_event(ev)
      return dev
  nbytes = table.nbytes
  ev = None
  if nbytes > _TABLE_SLOT_BYTES or nbytes == 0 or device.type != 'cuda':
    dev = torch.from_numpy(table).to(device)  # synchronous: complete on return
  else:
    ring = st.ring.get(str(device))
    if ring is None:
      ring = st.ring[str(device)] = [
          [torch.empty(_TABLE_SLOT_BYTES // 8, dtype=torch.int64).pin_memory()
           for _ in range(_TABLE_SLOTS)], [None] * _TABLE_SLOTS, 0]
    slots, events, nxt = ring
    ring[2] = (nxt + 1) % len(slots)
    if events[nxt] is not None:
      events[nxt].synchronize()
    slot = slots[nxt][:table.size]
    slot.numpy()[...] = table.reshape(-1)
    # (the current stream of `device`: allocation and copy are queued on it)
    dev = torch.empty(table.shape, dtype=torch.int64, device=device)
    dev.view(-1).copy_(slot, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    events[nxt] = ev
  if key is not None:
    if len(st.cache) >= 512:
      st.cache.clear()
    st.cache[key] = (dev, ev)
  return dev


def _slabs_intact(x: torch.Tensor) -> bool:
  """Contiguous, or a strided view whose 2-D slabs are contiguous and whose
  outer strides are whole slabs (addressed through a slab table)."""
  if x.is_contiguous():
    return True
  if x.dim() < 2:
    return False
  st = x.stride()
  se = x.shape[-1] * x.shape[-2]
  return st[-1] == 1 and st[-2] == x.shape[-1] and all(
      s >= 0 and s % se == 0 for s in st[:-2])


def stream_reduce(plan: ReductionPlan, mode: int,
                  inputs: t.Sequence[torch.Tensor],
                  slabs: t.Sequence[t.Optional[torch.Tensor]], n_outer: int,
                  skipna: bool, want_sums: bool = False,
                  aux: t.Optional[torch.Tensor] = None, scalar: float = 0.0):
  """Runs K1 + K2.  `inputs[i]` is [n_slab_i, n_row, n_col] on the plan's device.

  Returns (metrics[NMETRIC, n_region, n_outer], sums[n_outer, n_region, K] or
  None) as float64 device tensors; the call is asynchronous on the current
  stream.
  """
  dev = plan.device
  dtype = inputs[0].dtype
  dtype_code(dtype)  # (TypeError: not one of the kernels' dtypes)
  for x in inputs:
    if x.dtype != dtype or x.device != dev or not _slabs_intact(x):
      raise ValueError('inputs must share dtype/device and keep every '
                       '(n_row, n_col) slab contiguous')
    if tuple(x.shape[-2:]) != (plan.n_row, plan.n_col):
      raise ValueError(f'slab shape {tuple(x.shape[-2:])} != plan '
                       f'({plan.n_row}, {plan.n_col})')
  for s, x in zip(slabs, inputs):
    if s is None and (not x.is_contiguous() or
                      x.numel() != n_outer * plan.n_row * plan.n_col):
      raise ValueError('an input without a slab table must be n_outer '
                       'contiguous slabs')
    _check_slab(s, n_outer, 'n_outer')
  aligned = all(x.data_ptr() % 16 == 0 for x in inputs)
  return _stream_launch(plan, mode, dtype, n_outer, skipna, want_sums, aux,
                        scalar, aligned, inputs=inputs, slabs=slabs)


def _check_address_tables(plan, addr, n_outer):
  for a in addr:
    if (a.dtype != torch.int64 or a.device != plan.device or
        a.numel() != n_outer or not a.is_contiguous()):
      raise ValueError('address tables are contiguous int64[n_outer] on the '
                       'plan device')


def stream_reduce_addr(plan: ReductionPlan, mode: int, dtype: torch.dtype,
                       addr: t.Sequence[torch.Tensor], aligned16: bool,
                       n_outer: int, skipna: bool, want_sums: bool = False,
                       aux: t.Optional[torch.Tensor] = None,
                       scalar: float = 0.0):
  """K1 + K2 over slabs that live in different allocations (the variables of
  a chunk, several consecutive chunks): `addr[i]` is an int64[n_outer] device
  tensor holding the byte address of input i's slab for every outer slab
  (wb2_stream_partials_addr).  The caller keeps the memory behind the
  addresses alive until the launch has been enqueued on the current stream
  (torch's allocator is stream-ordered).  Same return value as stream_reduce."""
  dtype_code(dtype)  # (TypeError: not one of the kernels' dtypes)
  _check_address_tables(plan, addr, n_outer)
  return _stream_launch(plan, mode, dtype, n_outer, skipna, want_sums, aux,
                        scalar, bool(aligned16), addr=addr)


class PreparedLaunch:
  """What every launch of a reduction over `plan` at the column-tile width
  `tile` is made of, worked out ONCE: the segment-entry table (`seg_eoff`,
  `n_ts`), `n_ctile` and, with a slot count `k`, the `partials` tensor
  [n_outer, n_chunk, nwf, n_ts, k].  `values` holds every field of
  `wb2_plan_tables` by name (and `nwf`, which C reads off `wfield`).  The
  struct (`tables`: what `plan_tables` returns) and the plan's part of the
  long argument lists are both read from it, so the two forms of one launch
  cannot drift.  It keeps alive what they point at."""

  _REST = ('chunk_row0', 'chunk_nrow', 'n_chunk', 'n_ctile', 'seg_col0',
           'seg_eoff', 'n_seg', 'n_ts')
  _STREAM = operator.itemgetter('n_row', 'n_col', 'w_row', 'w_col', 'wfield',
                                'wfield_dtype', 'aux', 'scalar', *_REST)
  _ENS = operator.itemgetter('n_row', 'n_col', 'w_row', 'w_col', 'wfield',
                             *_REST)
  _FOLD = operator.itemgetter('n_chunk', 'nwf', 'n_seg', 'seg_eoff', 'n_ts',
                              'band_chunk0', 'n_band', 'coef_band', 'coef_seg',
                              'region_wf', 'region_wsum', 'n_region')

  def __init__(self, plan: ReductionPlan, tile: int, k: int = 0,
               n_outer: int = 0, field=None, field_code: int = _lib.WB2_F64,
               aux=None, scalar: float = 0.0):
    self.plan, self.k, self.n_outer = plan, k, n_outer
    self.seg_eoff, self.n_ts = plan.seg_entries(tile)
    self.n_ctile = -(-plan.n_col // tile)
    self.keep = (field, aux)
    ptr = _lib.ptr
    self.values = {
        'n_row': plan.n_row, 'n_col': plan.n_col, 'n_chunk': plan.n_chunk,
        'n_ctile': self.n_ctile, 'n_seg': plan.n_seg, 'n_ts': self.n_ts,
        'n_band': plan.n_band, 'n_region': plan.n_region, 'nwf': plan.nwf,
        'w_row': ptr(plan.w_row), 'w_col': ptr(plan.w_col),
        'wfield': ptr(field), 'wfield_dtype': field_code, 'reserved': 0,
        'aux': ptr(aux), 'scalar': float(scalar),
        # (tables every plan has: no None to map to NULL)
        'chunk_row0': plan.chunk_row0.data_ptr(),
        'chunk_nrow': plan.chunk_nrow.data_ptr(),
        'seg_col0': plan.seg_col0.data_ptr(),
        'seg_eoff': self.seg_eoff.data_ptr(),
        'band_chunk0': plan.band_chunk0.data_ptr(),
        'coef_band': plan.coef_band.data_ptr(),
        'coef_seg': plan.coef_seg.data_ptr(),
        'region_wf': plan.region_wf.data_ptr(),
        'region_wsum': plan.region_wsum.data_ptr()}
    self._tables = None
    self.partials = self.new_partials(n_outer, k) if k else None

  @property
  def tables(self) -> _lib.PlanTables:
    if self._tables is None:
      self._tables = _lib.PlanTables(
          **{name: self.values[name] for name, _ in _lib.PlanTables._fields_})
    return self._tables

  def new_partials(self, n_outer: int, k: int) -> torch.Tensor:
    v = self.values
    return torch.empty((n_outer, v['n_chunk'], v['nwf'], self.n_ts, k),
                       dtype=torch.float64, device=self.plan.device)

  def stream_args(self) -> tuple:
    """The plan's arguments of wb2_stream_partials_ex / _addr, between
    `n_outer` and `partials`."""
    return self._STREAM(self.values)

  def ens_args(self) -> tuple:
    """The plan's arguments of the ensemble partials entry points, between
    `n_outer` and `partials`."""
    return self._ENS(self.values)

  def fold_args(self) -> tuple:
    """The plan's arguments of wb2_det_combine / wb2_ens_combine, between
    `n_outer` and `sums`."""
    return self._FOLD(self.values)

  def fold(self, c_name: str, head: tuple, n_metric: int, want_sums: bool,
           stream: int):
    """The region fold `c_name` (whose arguments begin with `head`) of the
    partials: (metrics[n_metric, n_region, n_outer], sums[n_outer, n_region,
    k] or None)."""
    n_region, dev = self.values['n_region'], self.plan.device
    metrics = torch.empty((n_metric, n_region, self.n_outer),
                          dtype=torch.float64, device=dev)
    sums = (torch.empty((self.n_outer, n_region, self.k), dtype=torch.float64,
                        device=dev) if want_sums else None)
    _lib.check(getattr(_lib.load(), c_name)(
        *head, _lib.ptr(self.partials), self.n_outer, *self.fold_args(),
        _lib.ptr(sums), _lib.ptr(metrics), stream), c_name)
    return metrics, sums


def plan_tables(plan: ReductionPlan, tile_cols: int, field=None,
                field_code: int = _lib.WB2_F64, aux=None, scalar: float = 0.0):
  """(`wb2_plan_tables` struct of `plan` for a column-tile width, what it
  points at -- keep both alive until the call has been enqueued)."""
  prep = PreparedLaunch(plan, tile_cols, 0, 0, field, field_code, aux, scalar)
  return prep.tables, (field, aux, prep.seg_eoff, prep.n_ts)


def _field_and_tile(plan, dtype, mode, skipna, aligned=True):
  """(weight field, its dtype code, column-tile width) of a deterministic
  launch.  The field is float32 where its values are float32 numbers and the
  launch has the instantiation (same bits, half the field bytes per point).
  `aligned` is the caller's flag, passed on as it is: the width does not
  depend on it (vec_width in csrc/stream_reduce.hip), and the launch tests the
  field's address itself."""
  field, field_code = plan.wfield, _lib.WB2_F64
  if (dtype == torch.float32 and mode in _FIELD_F32_MODES and
      getattr(plan, 'wfield32', None) is not None and
      os.environ.get('WB2HIP_FIELD_F32', '1') != '0'):
    field, field_code = plan.wfield32, _lib.WB2_F32
  tile = _lib.load().wb2_tile_cols_ex(
      mode, _DTYPES[dtype], int(skipna), int(plan.wfield is not None),
      plan.n_col, int(aligned))
  return field, field_code, tile


def _stream_launch(plan, mode, dtype, n_outer, skipna, want_sums, aux, scalar,
                   aligned, inputs=None, slabs=None, addr=None):
  lib = _lib.load()
  code = _DTYPES[dtype]
  field, field_code, tile = _field_and_tile(plan, dtype, mode, skipna, aligned)
  prep = PreparedLaunch(plan, tile, lib.wb2_num_slots(mode, int(skipna)),
                        n_outer, field, field_code, aux, scalar)
  stream = current_stream_ptr(plan.device)
  tail = (n_outer, *prep.stream_args(), _lib.ptr(prep.partials), stream)
  if addr is not None:
    hooked_call('stream_partials', lib.wb2_stream_partials_addr,
                'wb2_stream_partials_addr', mode, code, int(skipna),
                _lib.ptr_array(addr), int(aligned), *tail)
  else:
    hooked_call('stream_partials', lib.wb2_stream_partials_ex,
                'wb2_stream_partials', mode, code, int(skipna),
                _lib.ptr_array(inputs), _lib.ptr_array(slabs), *tail)
  return prep.fold('wb2_det_combine', (mode, int(skipna)),
                   _lib.GENERIC_KQ.get(mode, _lib.NMETRIC), want_sums, stream)


def pairs_supported(plan: ReductionPlan, mode: int, dtype: torch.dtype,
                    skipna: bool, aligned: bool = True) -> bool:
  """Whether a launch of `mode` over `plan` can answer wind-vector pairs from
  its own read (wb2_pairs_supported; WB2HIP_WIND_PAIRS=0 switches the pair
  kernel off for A/B runs: the pairs then take a WB2_MODE_WIND launch)."""
  if os.environ.get('WB2HIP_WIND_PAIRS', '1') == '0' or dtype not in _DTYPES:
    return False
  return bool(_lib.load().wb2_pairs_supported(
      mode, _DTYPES[dtype], int(skipna), int(plan.wfield is not None),
      plan.n_col, int(aligned)))


def stream_reduce_pairs(plan: ReductionPlan, mode: int, dtype: torch.dtype,
                        addr: t.Sequence[torch.Tensor], aligned16: bool,
                        n_outer: int, n_pair: int, skipna: bool):
  """K1 + K1p + K2 over slabs given by address, the last 2 * n_pair of them the
  u slabs then the v slabs of n_pair wind-vector pairs: returns
  (metrics[NMETRIC, n_region, n_outer], wind[NMETRIC, n_region, n_pair]) --
  the bits of stream_reduce_addr over the slabs plus a MODE_WIND pass over the
  pairs, from one read (wb2_det_wind_suite_step)."""
  _check_address_tables(plan, addr, n_outer)
  step = PairSuiteStep(plan, mode, dtype, skipna, n_outer, n_pair,
                       aligned=bool(aligned16))
  return step.run(None, list(addr))


class PairSuiteStep:
  """The deterministic suite over a launch whose last 2 * n_pair slabs are the
  u slabs, then the v slabs, of n_pair wind-vector pairs: per-variable metrics
  of all n_outer slabs AND the wind-vector metrics of the pairs from ONE read
  (wb2_det_wind_suite_step; metrics.py:283-301 calling :194-201 derive both
  from the same `diff`).  Bit-identical to a DET / DET_ACC launch over the
  slabs plus a WIND launch over the pairs.

  Prepared once per (plan, mode, dtype, skipna, n_outer, n_pair); `run` takes
  inputs + slab-number tables, or inputs=None + address tables, and returns
  (metrics[NMETRIC, n_region, n_outer], wind[NMETRIC, n_region, n_pair])."""

  def __init__(self, plan: ReductionPlan, mode: int, dtype: torch.dtype,
               skipna: bool, n_outer: int, n_pair: int, aligned: bool = True):
    lib = _lib.load()
    code = dtype_code(dtype)
    if mode not in (_lib.MODE_DET, _lib.MODE_DET_ACC):
      raise ValueError('wind-vector pairs ride on MODE_DET / MODE_DET_ACC')
    if not 0 <= 2 * n_pair <= n_outer:
      raise ValueError(f'{n_pair=} does not fit {n_outer=}')
    self.lib, self.plan, self.mode, self.skipna = lib, plan, mode, bool(skipna)
    self.code, self.n_outer, self.n_pair = code, int(n_outer), int(n_pair)
    self.aligned = bool(aligned)
    field, field_code, tile = _field_and_tile(plan, dtype, mode, skipna,
                                              aligned)
    self._prep = prep = PreparedLaunch(
        plan, tile, lib.wb2_num_slots(mode, int(skipna)), n_outer, field,
        field_code)
    self.tables, self.partials = prep.tables, prep.partials
    self.wind_partials = prep.new_partials(
        max(n_pair, 1), lib.wb2_num_slots(_lib.MODE_WIND, int(skipna)))
    self._tables_ref = ctypes.byref(self.tables)
    self._fn = lib.wb2_det_wind_suite_step
    self.n_metric = _lib.NMETRIC
    self.n_values = _lib.NMETRIC * plan.n_region * (self.n_outer + self.n_pair)

  def run(self, inputs, tables, out: t.Optional[torch.Tensor] = None,
          stream_ptr: t.Optional[int] = None):
    """`out` (optional): flat float64[n_values] that receives the per-variable
    block followed by the wind block."""
    dev = self.plan.device
    if out is None:
      out = torch.empty((self.n_values,), dtype=torch.float64, device=dev)
    n_det = _lib.NMETRIC * self.plan.n_region * self.n_outer
    hooked_call(
        'stream_partials', self._fn, 'wb2_det_wind_suite_step',
        self._tables_ref, self.mode, self.code, int(self.skipna),
        None if inputs is None else _lib.ptr_array(inputs),
        _lib.ptr_array(tables), int(self.aligned), self.n_outer, self.n_pair,
        self.partials.data_ptr(), self.wind_partials.data_ptr(),
        out.data_ptr(), out.data_ptr() + 8 * n_det,
        current_stream_ptr(dev) if stream_ptr is None else stream_ptr)
    flat = out.view(-1)
    return (flat[:n_det].view(_lib.NMETRIC, self.plan.n_region, self.n_outer),
            flat[n_det:n_det + _lib.NMETRIC * self.plan.n_region * self.n_pair]
            .view(_lib.NMETRIC, self.plan.n_region, self.n_pair))


class SuiteStep:
  """One chunk of the deterministic suite per call: K1 -> K2 -> the running
  temporal mean through wb2_det_suite_step -- ONE C-ABI call per chunk instead
  of three calls with ~25 marshalled arguments each (the kernels and their
  bits are those of stream_reduce + time_accumulate).

  Prepared once per (plan, mode, dtype, skipna, n_outer): the plan's tables go
  into a `wb2_plan_tables` struct, the partials / metrics scratch is allocated
  here and reused by every call (calls are stream-ordered).  `run` takes the
  chunk's inputs and, optionally, the accumulators.

    step = SuiteStep(plan, MODE_DET_ACC, torch.float32, False, n_outer)
    step.accumulate_into(total, count, (n_lead, n_time, n_tail))
    step.run([f, t, c], [f_tab, t_tab, c_tab])     # per chunk
  """

  def __init__(self, plan: ReductionPlan, mode: int, dtype: torch.dtype,
               skipna: bool, n_outer: int, aligned: bool = True,
               aux: t.Optional[torch.Tensor] = None, scalar: float = 0.0,
               by_address: bool = False):
    lib = _lib.load()
    self.code, self.n_outer = dtype_code(dtype), int(n_outer)
    self.lib, self.plan, self.mode, self.skipna = lib, plan, mode, bool(skipna)
    self.by_address, self.aligned = bool(by_address), bool(aligned)
    field, field_code, tile = _field_and_tile(plan, dtype, mode, skipna,
                                              aligned)
    self._prep = prep = PreparedLaunch(
        plan, tile, lib.wb2_num_slots(mode, int(skipna)), n_outer, field,
        field_code, aux, scalar)
    self.tables, self.partials = prep.tables, prep.partials
    self.n_metric = _lib.GENERIC_KQ.get(mode, _lib.NMETRIC)
    self.metrics = torch.empty((self.n_metric, plan.n_region, n_outer),
                               dtype=torch.float64, device=plan.device)
    self._tables_ref = ctypes.byref(self.tables)
    self._acc = (0, 0, 0, 0, None, None, None)
    self._acc_keep = None
    self._fn = lib.wb2_det_suite_step

  def accumulate_into(self, total: t.Optional[torch.Tensor],
                      count: t.Optional[torch.Tensor] = None,
                      view: t.Optional[tuple] = None, skipna: bool = False,
                      dst: t.Optional[torch.Tensor] = None) -> None:
    """Every later run() adds its metrics, read as [lead][time][tail] = `view`,
    to total / count over `time` (None: no accumulation)."""
    if total is None:
      self._acc, self._acc_keep = (0, 0, 0, 0, None, None, None), None
      return
    n_lead, n_time, n_tail = (int(v) for v in view)
    if n_lead * n_time * n_tail != self.metrics.numel():
      raise ValueError(f'view {view} does not cover the metrics '
                       f'{tuple(self.metrics.shape)}')
    for x in (total, count):
      if x.dtype != torch.float64 or not x.is_contiguous():
        raise ValueError('accumulators are contiguous float64 tensors')
    if dst is None and total.numel() != n_lead * n_tail:
      raise ValueError('accumulator shape mismatch')
    if dst is not None and (dst.dtype != torch.int64 or
                            dst.numel() != n_lead * n_tail):
      raise ValueError('dst is int64 with one entry per result element')
    self._acc = (n_lead, n_time, n_tail, int(skipna), _lib.ptr(dst) or None,
                 total.data_ptr(), count.data_ptr())
    self._acc_keep = (total, count, dst)

  def run(self, inputs: t.Optional[t.Sequence[torch.Tensor]],
          tables: t.Sequence[t.Optional[torch.Tensor]],
          metrics: t.Optional[torch.Tensor] = None,
          stream_ptr: t.Optional[int] = None) -> torch.Tensor:
    """Enqueues the step on the current stream.  `inputs` + slab-number
    `tables` (None entries = identity), or inputs=None + address tables
    (by_address).  Returns the metrics tensor [n_metric, n_region, n_outer]
    (the step's own scratch unless `metrics` is given: valid until the next
    run)."""
    out = self.metrics if metrics is None else metrics
    if self.by_address != (inputs is None):
      raise ValueError('by_address steps take inputs=None and address tables')
    hooked_call(  # (brackets K1 + K2 [+ the accumulation] here)
        'stream_partials', self._fn, 'wb2_det_suite_step',
        self._tables_ref, self.mode, self.code, int(self.skipna),
        None if inputs is None else _lib.ptr_array(inputs),
        _lib.ptr_array(tables), int(self.aligned), self.n_outer,
        self.partials.data_ptr(), out.data_ptr(), *self._acc,
        current_stream_ptr(self.plan.device) if stream_ptr is None
        else stream_ptr)
    return out

  def bind(self, inputs, tables, stream_ptr: t.Optional[int] = None):
    """The call for one fixed (inputs, tables) pair with its arguments
    marshalled ONCE (the pointer arrays are built here, not per call): a
    zero-argument callable for loops that come back to the same chunk buffers
    (a ring of staging slots, a benchmark's table sets).  The accumulators are
    the ones set when bind() is called; the stream is `stream_ptr` or the
    current stream at bind time."""
    if self.by_address != (inputs is None):
      raise ValueError('by_address steps take inputs=None and address tables')
    fn = self._fn
    keep = (inputs, tables, self._acc_keep)
    args = (self._tables_ref, self.mode, self.code, int(self.skipna),
            None if inputs is None else _lib.ptr_array(inputs),
            _lib.ptr_array(tables), int(self.aligned), self.n_outer,
            self.partials.data_ptr(), self.metrics.data_ptr()) + self._acc + (
                current_stream_ptr(self.plan.device) if stream_ptr is None
                else stream_ptr,)

    def call(_keep=keep):
      if fn(*args) != 0:
        _lib.check(-1, 'wb2_det_suite_step')
    return call


GATHER_MAX_MEMBERS = {torch.float32: 128, torch.float64: 64}  # register sort
_NAN_SLABS: dict = {}
_NAN_SLABS_LOCK = threading.Lock()


def nan_slab(device: torch.device, dtype: torch.dtype, n_elems: int):
  """One resident slab of NaNs per (device, dtype, size): what the holes of a
  gathered ensemble point at."""
  key = (str(device), dtype, int(n_elems))
  slab = _NAN_SLABS.get(key)
  if slab is None:
    with _NAN_SLABS_LOCK:
      slab = _NAN_SLABS.get(key)
      if slab is None:
        slab = torch.full((int(n_elems),), float('nan'), dtype=dtype,
                          device=device)
        # filled before any other thread's stream can read it (once per size)
        if torch.device(device).type == 'cuda':
          torch.cuda.current_stream(device).synchronize()
        _NAN_SLABS[key] = slab
  return slab


def gather_pointers(base: torch.Tensor, index: np.ndarray, slab_elems: int):
  """Device addresses of the slabs `index` (any shape, -1 = hole) of the
  contiguous device tensor `base` ([..., slab]): int64 array of index.shape
  (host).  Holes point at the resident NaN slab."""
  index = np.asarray(index, dtype=np.int64)
  ptrs = base.data_ptr() + index * (slab_elems * base.element_size())
  if (index < 0).any():
    hole = nan_slab(base.device, base.dtype, slab_elems).data_ptr()
    ptrs = np.where(index < 0, np.int64(hole), ptrs)
  return ptrs


def ensemble_reduce(plan: ReductionPlan, ens: torch.Tensor,
                    member_stride: int, n_member: int,
                    ens_slab: t.Optional[torch.Tensor], truth: torch.Tensor,
                    truth_slab: t.Optional[torch.Tensor], n_outer: int,
                    skipna: bool, want_sums: bool = False,
                    maps: t.Optional[torch.Tensor] = None,
                    member_ptrs: t.Optional[torch.Tensor] = None,
                    addresses: t.Optional[torch.Tensor] = None):
  """Runs K3 + the region fold.  `ens` holds the members member-major with
  `member_stride` elements between members; `truth` is [n_slab, n_row, n_col].
  With `member_ptrs` (int64[n_outer, n_member] device ADDRESSES of the member
  slabs, `gather_pointers`) the ensemble is read in place from wherever its
  slabs live: `ens` is then only the tensor those addresses point into (kept
  alive, dtype), `member_stride` and `ens_slab` are ignored.
  With `addresses` (int64[2, n_outer] on the device: the byte address of member
  0's slab and of the truth slab of every outer index; member m follows
  `member_stride` elements behind member 0 -- wb2_ens_partials_addr) `ens` and
  `truth` are tensors of the right dtype that stay alive, nothing more: the
  chunks of a window are read where they lie (xarray_lite.SlabConcat).

  Returns (metrics[NMETRIC_ENS, n_region, n_outer], sums or None).
  """
  lib = _lib.load()
  dev = plan.device
  _require_float(ens, truth)
  code = _DTYPES[ens.dtype]
  if addresses is not None:
    if (addresses.dtype != torch.int64 or addresses.device != dev or
        not addresses.is_contiguous() or addresses.numel() != 2 * n_outer or
        maps is not None or member_ptrs is not None):
      raise ValueError('addresses is a contiguous int64[2, n_outer] on the '
                       'plan device (no maps, no member_ptrs)')
  else:
    # (a non-contiguous `ens` is a view with intact slabs that the caller
    # addresses through member_stride + ens_slab: metrics._ens_layout)
    addressed = ens_slab is not None or member_ptrs is not None
    _check_contiguous(dev, 'the plan device', truth,
                      *([] if addressed else [ens]), view=ens)
  for s in (ens_slab, truth_slab):
    _check_slab(s, n_outer, 'n_outer')
  if member_ptrs is not None and (
      member_ptrs.dtype != torch.int64 or member_ptrs.device != dev or
      not member_ptrs.is_contiguous() or
      member_ptrs.numel() != n_outer * n_member):
    raise ValueError('member_ptrs is a contiguous int64[n_outer, n_member] '
                     'on the plan device')
  if maps is not None and (maps.dtype != torch.float64 or maps.numel() !=
                           6 * n_outer * plan.n_row * plan.n_col):
    raise ValueError('maps must be float64[6, n_outer, n_row * n_col]')
  prep = PreparedLaunch(plan, lib.wb2_ens_tile_cols(plan.n_col),
                        lib.wb2_ens_num_slots(int(skipna)), n_outer,
                        plan.wfield)
  stream = current_stream_ptr(dev)
  tail = (n_outer, *prep.ens_args(), _lib.ptr(prep.partials))
  if addresses is not None:
    base = addresses.data_ptr()
    hooked_call('ens_partials', lib.wb2_ens_partials_addr,
                'wb2_ens_partials_addr', code, int(skipna), base,
                base + 8 * n_outer, n_member, member_stride, *tail, stream)
  elif member_ptrs is not None:
    hooked_call('ens_partials', lib.wb2_ens_partials_gather,
                'wb2_ens_partials_gather', code, int(skipna),
                _lib.ptr(member_ptrs), _lib.ptr(truth), _lib.ptr(truth_slab),
                n_member, *tail, _lib.ptr(maps), stream)
  else:
    hooked_call('ens_partials', lib.wb2_ens_partials_maps,
                'wb2_ens_partials_maps', code, int(skipna), _lib.ptr(ens),
                _lib.ptr(ens_slab), _lib.ptr(truth), _lib.ptr(truth_slab),
                n_member, member_stride, *tail, _lib.ptr(maps), stream)
  return prep.fold('wb2_ens_combine', (int(skipna),), _lib.NMETRIC_ENS,
                   want_sums, stream)


def energy_score(plan: ReductionPlan, ens: torch.Tensor, member_stride: int,
                 n_member: int, ens_slab: t.Optional[torch.Tensor],
                 truth: torch.Tensor, truth_slab: t.Optional[torch.Tensor],
                 n_outer: int, skipna: bool) -> torch.Tensor:
  """wb2_energy_score: (score, spread, skill)[3, n_region, n_outer] float64 of
  a member-major ensemble (`member_stride` elements between members) in one
  read of the members.  Asynchronous on the current stream."""
  dev = plan.device
  _require_float(ens, truth)
  # (a non-contiguous `ens` is a view with intact slabs that the caller
  # addresses through member_stride + ens_slab: metrics._ens_layout)
  _check_contiguous(dev, 'the plan device', truth,
                    *([ens] if ens_slab is None else []), view=ens)
  for s in (ens_slab, truth_slab):
    _check_slab(s, n_outer, 'n_outer')
  g = _geometry('wb2_energy_layout',
                (n_member, int(skipna), int(plan.wfield is not None)),
                [('block', _I32), ('n_block', _I32), ('k', _I32)])
  n_virtual = n_outer * g['n_block']
  prep = PreparedLaunch(plan, _lib.load().wb2_ens_tile_cols(plan.n_col),
                        g['k'], n_virtual, plan.wfield)
  means = torch.empty((2 * g['block'], plan.n_region, n_virtual),
                      dtype=torch.float64, device=dev)
  out = torch.empty((3, plan.n_region, n_outer), dtype=torch.float64,
                    device=dev)
  _launch('energy_score', 'wb2_energy_score', _DTYPES[ens.dtype], int(skipna),
          _lib.ptr(ens), _lib.ptr(ens_slab), _lib.ptr(truth),
          _lib.ptr(truth_slab), n_member, member_stride, n_outer,
          ctypes.byref(prep.tables), _lib.ptr(prep.partials), _lib.ptr(means),
          _lib.ptr(out), current_stream_ptr(dev))
  return out


def time_accumulate(values: torch.Tensor, time_axis: int, skipna: bool,
                    total: torch.Tensor, count: torch.Tensor,
                    dst: t.Optional[torch.Tensor] = None, run: int = 1):
  """total/count += sum/notnull-count of `values` (float32 or float64) over
  `time_axis` (device); the sums continue from the accumulators value by value.  `dst` (int64 device
  tensor, one entry per RUN of `run` consecutive elements of `values` without
  its time axis): where in `total` / `count` the run goes (identity without
  it)."""
  lib = _lib.load()
  if values.dtype not in _DTYPES:
    values = values.to(torch.float64)
  values = values.contiguous()
  shape = tuple(values.shape)
  n_lead = int(np.prod(shape[:time_axis], dtype=np.int64))
  n_time = shape[time_axis]
  n_tail = int(np.prod(shape[time_axis + 1:], dtype=np.int64))
  if count is None and skipna:
    raise ValueError('skipna needs the count accumulator')
  if dst is None:
    if total.numel() != n_lead * n_tail or (
        count is not None and count.numel() != n_lead * n_tail):
      raise ValueError('accumulator shape mismatch')
  elif (dst.dtype != torch.int64 or run < 1 or (n_lead * n_tail) % run
        or dst.numel() != n_lead * n_tail // run
        or (count is not None and total.numel() != count.numel())):
    raise ValueError('dst is int64 with one entry per run of result elements')
  # (the entries of `dst` must be distinct and < total.numel(): the kernel
  # reads, adds and writes each destination without atomics.  RunningMean
  # builds them on the host -- _Accumulator.destinations -- and checks there.)
  _lib.check(lib.wb2_time_accumulate_runs(
      _DTYPES[values.dtype], _lib.ptr(values), n_lead, n_time, n_tail,
      int(skipna), _lib.ptr(dst), int(run),
      _lib.ptr(total), _lib.ptr(count), current_stream_ptr(values.device)),
             'wb2_time_accumulate')


class _SpectrumPlans(threading.local):
  """hipFFT plans are expensive (rocFFT compiles kernels): cache by shape.  One
  cache per thread: a plan's hipFFT handle is bound to a stream while it runs,
  and a thread only ever evicts plans of its own."""

  def __init__(self):
    self.plans = {}

  def get(self, dtype_code: int, n_lon: int, n_rows: int):
    key = (dtype_code, n_lon, n_rows, torch.cuda.current_device())
    hit = self.plans.get(key)
    if hit is None:
      lib = _lib.load()
      handle = ctypes.c_void_p()
      _lib.check(lib.wb2_spectrum_plan_create(dtype_code, n_lon, n_rows,
                                              ctypes.byref(handle)),
                 'wb2_spectrum_plan_create')
      nbytes = lib.wb2_spectrum_plan_workspace(handle)
      if nbytes < 0:
        _lib.check(-1, 'wb2_spectrum_plan_workspace')
      if len(self.plans) >= 8:  # bounded: drop the oldest plan
        old_key = next(iter(self.plans))
        lib.wb2_spectrum_plan_destroy(self.plans.pop(old_key)[0])
      hit = (handle, int(nbytes))
      self.plans[key] = hit
    return hit


_SPECTRUM_PLANS = _SpectrumPlans()


def zonal_spectrum(x: torch.Tensor, circumference: torch.Tensor, n_lat: int,
                   n_time: int = 0, skipna: bool = True) -> torch.Tensor:
  """x: [..., n_lat, n_lon] contiguous device tensor (rows = everything but lon).

  Returns float64 [..., n_lat, n_lon//2+1], or with n_time > 0 (x's LEADING
  dim is time) the time mean [rest..., n_lat, n_lon//2+1].
  """
  lib = _lib.load()
  if x.dtype not in _DTYPES or not x.is_contiguous():
    raise ValueError('x must be a contiguous float32/float64 tensor')
  n_lon = x.shape[-1]
  n_rows = x.numel() // n_lon
  n_bins = n_lon // 2 + 1
  if n_time > 0:
    if x.shape[0] != n_time:
      raise ValueError('time must be the leading dim for the fused time mean')
    out_shape = tuple(x.shape[1:-1]) + (n_bins,)
  else:
    out_shape = tuple(x.shape[:-1]) + (n_bins,)
  out = torch.empty(out_shape, dtype=torch.float64, device=x.device)
  if n_rows == 0:  # an empty chunk: nothing to transform (a plan needs rows)
    return out
  handle, nbytes = _SPECTRUM_PLANS.get(_DTYPES[x.dtype], n_lon, n_rows)
  work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
  _lib.check(lib.wb2_zonal_spectrum(
      handle, _lib.ptr(x), _lib.ptr(circumference), n_lat, n_time, int(skipna),
      _lib.ptr(out), _lib.ptr(work), current_stream_ptr(x.device)),
             'wb2_zonal_spectrum')
  return out


def zonal_spectrum_lat_mean(x: torch.Tensor, circumference: torch.Tensor,
                            lat_weights: torch.Tensor, n_lat: int,
                            weight_sum: t.Optional[float] = None,
                            row_weight: t.Optional[torch.Tensor] = None
                            ) -> torch.Tensor:
  """Area-weighted latitude mean of the zonal energy spectrum (BASELINE
  configs[3]) of x: [..., n_lat, n_lon] -> float64 [..., n_lon//2+1]
  = sum_lat w[lat] S[..., lat, :] / sum_lat w[lat].

  One fused kernel when the plan has the LDS FFT (float32 rows of an
  instantiated length): the per-latitude spectra are never written.  Otherwise
  the spectrum is materialised and reduced with the axis kernel.  `weight_sum`
  (= float(sum(w)), known on the host) and `row_weight` (= w * circumference,
  float64 on the device) may be passed by callers that evaluate many chunks on
  one grid: the call is then exactly two kernel launches."""
  lib = _lib.load()
  if x.dtype not in _DTYPES or not x.is_contiguous():
    raise ValueError('x must be a contiguous float32/float64 tensor')
  n_lon = x.shape[-1]
  if x.shape[-2] != n_lat:
    raise ValueError('latitude must be the second-to-last dim')
  n_rows = x.numel() // n_lon
  n_field = n_rows // n_lat
  n_bins = n_lon // 2 + 1
  if n_rows == 0:
    return torch.empty(tuple(x.shape[:-2]) + (n_bins,), dtype=torch.float64,
                       device=x.device)
  handle, nbytes = _SPECTRUM_PLANS.get(_DTYPES[x.dtype], n_lon, n_rows)
  w = lat_weights.to(torch.float64)
  n_seg = lib.wb2_zonal_spectrum_latmean_segments(handle, n_lat)
  if n_seg < 0:
    _lib.check(n_seg, 'wb2_zonal_spectrum_latmean_segments')
  out_shape = tuple(x.shape[:-2]) + (n_bins,)
  if n_seg == 0 or x.data_ptr() % 16:
    spec = zonal_spectrum(x, circumference, n_lat)
    total, _, _ = axis_moments(spec.reshape(n_field, n_lat, n_bins), n_field,
                               n_lat, n_bins, w, False)
    # the count of axis_moments is n_lat: divide by the weights' sum instead
    if weight_sum is not None:
      return (total / float(weight_sum)).reshape(out_shape)
    return (total / w.sum()).reshape(out_shape)
  if row_weight is None:
    row_weight = (w * circumference.to(torch.float64)).contiguous()
  # without a host-side sum the normalisation stays on the device (no sync):
  # scale = 1 in the kernel, one division afterwards
  scale = 1.0 if weight_sum is None else 1.0 / float(weight_sum)
  partial = torch.empty((n_field, n_seg, n_bins), dtype=torch.float64,
                        device=x.device)
  out = torch.empty((n_field, n_bins), dtype=torch.float64, device=x.device)
  _lib.check(lib.wb2_zonal_spectrum_latmean(
      handle, _lib.ptr(x), _lib.ptr(row_weight), n_lat, n_seg, scale,
      _lib.ptr(partial), _lib.ptr(out), current_stream_ptr(x.device)),
             'wb2_zonal_spectrum_latmean')
  if weight_sum is None:
    out = out / w.sum()
  return out.reshape(out_shape)


def spatial_maps(forecast: torch.Tensor, f_slab, truth: torch.Tensor, t_slab,
                 n_outer: int, n_point: int, want=('bias', 'mse', 'mae')):
  """K5 per-time maps: returns {name: tensor[n_outer, n_point]} (input dtype)."""
  lib = _lib.load()
  dev = forecast.device
  _require_float(forecast, truth)
  outs = {k: torch.empty((n_outer, n_point), dtype=forecast.dtype, device=dev)
          for k in want}
  _lib.check(lib.wb2_spatial_maps(
      _DTYPES[forecast.dtype], _lib.ptr(forecast), _lib.ptr(f_slab),
      _lib.ptr(truth), _lib.ptr(t_slab), n_outer, n_point,
      _lib.ptr(outs.get('bias')), _lib.ptr(outs.get('mse')),
      _lib.ptr(outs.get('mae')), current_stream_ptr(dev)), 'wb2_spatial_maps')
  return outs


def spatial_accumulate(forecast: torch.Tensor, f_slab, truth: torch.Tensor,
                       t_slab, n_time: int, n_rest: int, n_point: int,
                       skipna: bool, total: torch.Tensor,
                       count: t.Optional[torch.Tensor]):
  """K5 temporal accumulation into total/count [3, n_rest, n_point] (fp64)."""
  lib = _lib.load()
  _require_float(forecast, truth)
  _lib.check(lib.wb2_spatial_accumulate(
      _DTYPES[forecast.dtype], int(skipna), _lib.ptr(forecast),
      _lib.ptr(f_slab), _lib.ptr(truth), _lib.ptr(t_slab), n_time, n_rest,
      n_point, _lib.ptr(total), _lib.ptr(count),
      current_stream_ptr(forecast.device)), 'wb2_spatial_accumulate')


POINT_MODES = {'wind_speed': 0, 'relative_humidity': 1}
STENCIL_MODES = {'divergence': 0, 'vorticity': 1, 'geostrophic_u': 2,
                 'geostrophic_v': 3, 'geostrophic_speed': 4,
                 'ageostrophic_u': 5, 'ageostrophic_v': 6,
                 'ageostrophic_speed': 7}


def upload_f64_table(table: np.ndarray, device) -> torch.Tensor:
  """float64 coefficient table -> device tensor through `upload_table` (content
  cache, pinned ring: no stall of the queue)."""
  table = np.ascontiguousarray(table, dtype=np.float64)
  return upload_table(table.view(np.int64), device).view(torch.float64)


def derived_pointwise(mode: str, a: torch.Tensor, a_slab, b: torch.Tensor,
                      b_slab, n_slab: int, n_point: int,
                      out_dtype: t.Optional[torch.dtype] = None,
                      slab_scalar: t.Optional[torch.Tensor] = None):
  """K8 pointwise maps: [n_slab, n_point] of `out_dtype` (the input dtype when
  None).  Slab o of `a` / `b` starts `table[o] * n_point` elements after the
  tensor's first element (identity when the table is None)."""
  dev = a.device
  _require_float(a, b)
  out_dtype = a.dtype if out_dtype is None else out_dtype
  out = torch.empty((n_slab, n_point), dtype=out_dtype, device=dev)
  if slab_scalar is not None and (slab_scalar.dtype != out_dtype
                                  or slab_scalar.numel() != n_slab):
    raise ValueError('slab_scalar must hold n_slab values of out_dtype')
  _launch('derived_pointwise', 'wb2_derived_pointwise', POINT_MODES[mode],
          _DTYPES[a.dtype], _DTYPES[out_dtype], _lib.ptr(a), _lib.ptr(a_slab),
          _lib.ptr(b), _lib.ptr(b_slab), _lib.ptr(slab_scalar), n_slab,
          n_point, _lib.ptr(out), current_stream_ptr(dev))
  return out


def stencil_geometry(dtype: torch.dtype, wide: bool) -> tuple:
  """(columns per workgroup tile, rows per row chunk) of the stencil kernel."""
  return tuple(_geometry('wb2_derived_stencil_geometry',
                         (_DTYPES[dtype], int(wide)),
                         [('tile', _I32), ('rows', _I32)]).values())


def derived_stencil(mode: str, inputs: t.Sequence[t.Optional[torch.Tensor]],
                    slabs: t.Sequence, n_slab: int, n_row: int, n_col: int,
                    lat_rows: bool, row_coef: torch.Tensor, row_uniform: bool,
                    col_coef: torch.Tensor, col_uniform: bool,
                    lat_tables: torch.Tensor, m_per_deg: float):
  """K8 horizontal stencil: float64 [n_slab, n_row, n_col].  `inputs` = (the
  field differentiated along longitude, along latitude, u, v -- the last two
  for the ageostrophic modes only), each with an optional slab table;
  `row_coef` / `col_coef` are plan.gradient_tables of the two axes,
  `lat_tables` plan.latitude_tables, all float64 on the device."""
  first = inputs[0]
  dev = first.device
  _require_float(*inputs)
  n_lat = n_row if lat_rows else n_col
  if (tuple(row_coef.shape) != (4, n_row) or tuple(col_coef.shape) != (4, n_col)
      or tuple(lat_tables.shape) != (2, n_lat)):
    raise ValueError('coefficient tables do not match the slab shape')
  inputs = list(inputs) + [None] * (4 - len(inputs))
  slabs = list(slabs) + [None] * (4 - len(slabs))
  out = torch.empty((n_slab, n_row, n_col), dtype=torch.float64, device=dev)
  _launch('derived_stencil', 'wb2_derived_stencil', STENCIL_MODES[mode],
          _DTYPES[first.dtype], int(lat_rows), _lib.ptr_array(inputs),
          _lib.ptr_array(slabs), n_slab, n_row, n_col, _lib.ptr(row_coef),
          int(row_uniform), _lib.ptr(col_coef), int(col_uniform),
          _lib.ptr(lat_tables[0]), _lib.ptr(lat_tables[1]), float(m_per_deg),
          _lib.ptr(out), current_stream_ptr(dev))
  return out


COLUMN_MODES = {'integral': 0, 'transport': 1, 'gradient_ratio': 2,
                'cumulative': 3, 'eddy': 4}


def column_geometry(dtype: torch.dtype, wide: bool) -> tuple:
  """(points per workgroup tile, levels in flight per thread) of the column
  kernel."""
  return tuple(_geometry('wb2_derived_column_geometry',
                         (_DTYPES[dtype], int(wide)),
                         [('tile', _I32), ('ahead', _I32)]).values())


def zonal_mean(x: torch.Tensor, slab, n_slab: int, n_row: int, n_col: int,
               lat_rows: bool) -> torch.Tensor:
  """[n_slab, n_lat] NaN-skipping means over longitude of (n_row, n_col) slabs
  of `x` (slab o at `slab[o]` slabs after its first element; identity when
  None), in the dtype of `x`."""
  out = torch.empty((n_slab, n_row if lat_rows else n_col), dtype=x.dtype,
                    device=x.device)
  _launch('derived_zonal_mean', 'wb2_derived_zonal_mean', _DTYPES[x.dtype],
          int(lat_rows), _lib.ptr(x), _lib.ptr(slab), n_slab, n_row, n_col,
          _lib.ptr(out), current_stream_ptr(x.device))
  return out


def derived_column(mode: str, inputs: t.Sequence[torch.Tensor],
                   slabs: t.Sequence[torch.Tensor], n_column: int, n_level: int,
                   n_point: int, *, out_dtype: t.Optional[torch.dtype] = None,
                   levels: t.Optional[tuple] = None,
                   spacing: t.Optional[torch.Tensor] = None,
                   level_coef: t.Optional[torch.Tensor] = None,
                   level_uniform: bool = False,
                   means: t.Sequence[torch.Tensor] = (), mean_div: int = 1,
                   scale: float = 1.0,
                   out: t.Optional[torch.Tensor] = None) -> torch.Tensor:
  """K9 column kernel.  `slabs[k]` is the int64 device table [n_column,
  n_level] of input k (level l of column slab c starts `table * n_point`
  elements after the tensor's first element).

    integral / transport / eddy  -> [n_column, n_point] of `out_dtype`, over the
      levels `levels` = (begin, end); `spacing` = float64 [n_level - 1];
      `means` = the two zonal-mean tables [n_column * n_level, n_mean] (eddy)
    gradient_ratio               -> [n_column, n_level, n_point] of the input
      dtype; `level_coef` / `level_uniform` = plan.gradient_tables(level)
    cumulative                   -> `out` itself (float64), integrated in place
      through slabs[0]
  """
  inputs = list(inputs)
  first = out if mode == 'cumulative' else inputs[0]
  dev = first.device
  if first.dtype not in _DTYPES or any(x.dtype != first.dtype
                                       for x in inputs + list(means)):
    raise TypeError('inputs must share a float32/float64 dtype')
  for tab in slabs:
    if tab.dtype != torch.int64 or tab.numel() != n_column * n_level:
      raise ValueError('a slab table must hold n_column * n_level int64')
  if spacing is not None and spacing.numel() != n_level - 1:
    raise ValueError('spacing must hold n_level - 1 values')
  if level_coef is not None and tuple(level_coef.shape) != (4, n_level):
    raise ValueError('the coefficient table does not match the level count')
  n_mean = 0
  if mode == 'eddy':
    n_mean = means[0].shape[-1]
    if any(m.numel() != n_column * n_level * n_mean for m in means):
      raise ValueError('a zonal-mean table must be [n_column * n_level, n_mean]')
  out_dtype = first.dtype if out_dtype is None else out_dtype
  if mode == 'gradient_ratio':
    out = torch.empty((n_column, n_level, n_point), dtype=out_dtype, device=dev)
  elif mode != 'cumulative':
    out = torch.empty((n_column, n_point), dtype=out_dtype, device=dev)
  begin, end = (0, n_level) if levels is None else levels
  _launch('derived_column', 'wb2_derived_column', COLUMN_MODES[mode],
          _DTYPES[first.dtype], _DTYPES[out_dtype],
          _lib.ptr_array((inputs + list(means) + [None] * 4)[:4]),
          _lib.ptr_array((list(slabs) + [None] * 3)[:3]), n_column, n_level,
          n_point, begin, end, _lib.ptr(spacing),
          _lib.ptr(level_coef), int(level_uniform), mean_div, n_mean,
          float(scale), _lib.ptr(out), current_stream_ptr(dev))
  return out


LEAD_MODES = {'diff_sum': 0, 'sum': 1}


def lead_geometry(dtype: torch.dtype, wide: bool) -> tuple:
  """(points per workgroup tile, leads in flight per thread, the window counts
  that keep their terms in registers) of the lead-window kernel."""
  g = _geometry('wb2_derived_lead_geometry', (_DTYPES[dtype], int(wide)),
                [('tile', _I32), ('ahead', _I32),
                 ('windows', ctypes.POINTER(_I32)), ('n', _I32)])
  return g['tile'], g['ahead'], tuple(g['windows'][k] for k in range(g['n']))


def derived_lead_window(mode: str, x: torch.Tensor,
                        slab: t.Optional[torch.Tensor], n_outer: int,
                        n_lead: int, n_point: int, window: int,
                        clamp_negative: bool = False) -> torch.Tensor:
  """K10 lead-window kernel: [n_outer, n_lead, n_point] of the dtype of `x`.
  `slab` is the int64 device table [n_outer, n_lead] (lead l of outer index o
  starts `table * n_point` elements after the first element of `x`), None for
  a contiguous `x`.

    diff_sum  the rolling sum over `window` leads of x[l] - x[l - 1], NaN at
              the first `window` leads; sums below zero become 0.0 when
              `clamp_negative`
    sum       the rolling sum over `window` leads of x, NaN at the first
              `window - 1` leads
  """
  _require_float(x)
  _check_slab(slab, n_outer * n_lead, 'n_outer * n_lead')
  if window < 1:
    raise ValueError(f'window={window} must be at least one lead')
  out = torch.empty((n_outer, n_lead, n_point), dtype=x.dtype, device=x.device)
  _launch('derived_lead_window', 'wb2_derived_lead_window', LEAD_MODES[mode],
          _DTYPES[x.dtype], _lib.ptr(x), _lib.ptr(slab), n_outer, n_lead,
          n_point, min(int(window), 2**31 - 1), int(clamp_negative),
          _lib.ptr(out), current_stream_ptr(x.device))
  return out


REGRID_MODES = {'nanmean': 0, 'linear': 1}


def regrid_geometry(dtype: torch.dtype, lat_rows: bool, wide: bool) -> dict:
  """Tile extents of the K11 regridding kernels: `tile` contiguous-axis
  elements per workgroup pass, `run` target rows (columns) per workgroup,
  `band` band entries a thread requests before it combines any, `max_contig`
  the longest contiguous axis the workgroup kernels hold (longer ones take the
  one-thread-per-cell kernel), `grid_slabs` slabs per grid row."""
  return _geometry('wb2_regrid_geometry',
                   (_DTYPES[dtype], int(lat_rows), int(wide)),
                   [(name, _I32) for name in
                    ('tile', 'run', 'band', 'max_contig', 'grid_slabs')])


def regrid_separable(mode: str, x: torch.Tensor,
                     slab: t.Optional[torch.Tensor], n_slab: int,
                     lat_rows: bool, source_shape: tuple, target_shape: tuple,
                     tables: t.Sequence[torch.Tensor]) -> torch.Tensor:
  """K11 separable regridding: [n_slab, target slab] of the dtype of `x`, in
  the layout of the input ((lat, lon) slabs when `lat_rows`, else (lon, lat)).
  Shapes are (n_lon, n_lat); `tables` = (ptr, idx, w, nan) of the longitude
  axis, then of the latitude axis, on the device of `x`; `slab` the int64
  device table of the slabs (None: contiguous)."""
  _require_float(x)
  _check_slab(slab, n_slab, 'n_slab')
  (s_lon, s_lat), (t_lon, t_lat) = source_shape, target_shape
  ptr_lon, idx_lon, w_lon, nan_lon, ptr_lat, idx_lat, w_lat, nan_lat = tables
  for ptr, n in ((ptr_lon, t_lon), (ptr_lat, t_lat)):
    if ptr.dtype != torch.int32 or ptr.numel() != n + 1:
      raise ValueError('an axis table must hold n_target + 1 int32 offsets')
  out = torch.empty((n_slab, t_lat * t_lon), dtype=x.dtype, device=x.device)
  _launch('regrid_separable', 'wb2_regrid_separable', REGRID_MODES[mode],
          _DTYPES[x.dtype], int(lat_rows), _lib.ptr(x), _lib.ptr(slab), n_slab,
          s_lon, s_lat, t_lon, t_lat, _lib.ptr(ptr_lon), _lib.ptr(idx_lon),
          _lib.ptr(w_lon), _lib.ptr(nan_lon), _lib.ptr(ptr_lat),
          _lib.ptr(idx_lat), _lib.ptr(w_lat), _lib.ptr(nan_lat), _lib.ptr(out),
          current_stream_ptr(x.device))
  return out


def regrid_gather(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                  n_slab: int, n_src: int, index: torch.Tensor) -> torch.Tensor:
  """K11 gather: out[o][j] = slab o of `x` at index[j] (int32 device table),
  for elements of 1, 2, 4 or 8 bytes, [n_slab, len(index)] of the dtype of
  `x`."""
  if index.dtype != torch.int32:
    raise ValueError('the index table must be int32')
  _check_slab(slab, n_slab, 'n_slab')
  out = torch.empty((n_slab, index.numel()), dtype=x.dtype, device=x.device)
  _launch('regrid_gather', 'wb2_regrid_gather', x.element_size(), _lib.ptr(x),
          _lib.ptr(slab), n_slab, n_src, _lib.ptr(index), index.numel(),
          _lib.ptr(out), current_stream_ptr(x.device))
  return out


def quantile_geometry(dtype: torch.dtype, wide: bool = False) -> dict:
  """Extents of the K12 quantile kernels: `tile_points` adjacent points per
  workgroup, `max_resident` the longest series selected out of LDS (longer
  ones stream), `targets_per_pass` quantiles that share a streaming pass,
  `key_bits_per_pass` key bits settled per counting pass."""
  return _geometry('wb2_quantile_geometry', (_DTYPES[dtype], int(wide)),
                   [('tile_points', _I32), ('max_resident', ctypes.c_int64),
                    ('targets_per_pass', _I32),
                    ('key_bits_per_pass', _I32)])


def quantile_select(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                    n_outer: int, n_red: int, n_inner: int, q,
                    skipna: bool) -> torch.Tensor:
  """K12 exact quantiles: float64 [len(q), n_outer, n_inner] of the series
  x[o, :, i] (NumPy's quantile, or nanquantile with `skipna`, method 'linear').
  `slab` is the int64 device table [n_outer, n_red] (sample r of outer index o
  starts `table * n_inner` elements after the first element of `x`), None for
  a contiguous `x`; `q` a sequence of numbers in [0, 1]."""
  _require_float(x)
  _check_slab(slab, n_outer * n_red, 'n_outer * n_red')
  qs = [float(v) for v in q]
  q_host = (ctypes.c_double * len(qs))(*qs)
  out = torch.empty((len(qs), n_outer, n_inner), dtype=torch.float64,
                    device=x.device)
  _launch('quantile_select', 'wb2_quantile_select', _DTYPES[x.dtype],
          int(bool(skipna)), _lib.ptr(x), _lib.ptr(slab), n_outer, n_red,
          n_inner, q_host, len(qs), _lib.ptr(out),
          current_stream_ptr(x.device))
  return out


TIME_STATS = ('sum', 'mean', 'min', 'max')  # bit s of the K13 mask, in order


def time_window_geometry(dtype: torch.dtype, wide: bool = False) -> dict:
  """Extents of the K13 kernel: `tile_points` adjacent points per workgroup,
  `steps_ahead` time steps a thread requests before it combines any,
  `max_grid_outer` outer indices per grid row."""
  return _geometry('wb2_time_window_geometry', (_DTYPES[dtype], int(wide)),
                   [('tile_points', _I32), ('steps_ahead', _I32),
                    ('max_grid_outer', _I32)])


def time_bin_stats(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                   n_outer: int, n_time: int, n_point: int,
                   bin_range: torch.Tensor, statistics: t.Sequence[str],
                   skipna: bool, bins_per_group: int = 1) -> dict:
  """K13 statistics of time bins: {statistic: [n_outer, n_bin, n_point] of
  the dtype of `x`} for the names in `statistics` (of TIME_STATS), all from
  ONE launch and one read of `x`.  Bin b is the time steps [bin_range[b, 0],
  bin_range[b, 1]) of the series x[o, :, i] (`bin_range` an int32 device
  tensor [n_bin, 2]; an empty or incomplete range gives NaN).  `slab` is the
  int64 device table [n_outer, n_time] (time step t of outer index o starts
  `table * n_point` elements after the first element of `x`), None for a
  contiguous `x`."""
  _require_float(x)
  _check_slab(slab, n_outer * n_time, 'n_outer * n_time')
  if (bin_range.dtype != torch.int32 or bin_range.dim() != 2
      or bin_range.shape[1] != 2 or not bin_range.is_contiguous()
      or bin_range.device != x.device):
    raise ValueError('bin_range must be a contiguous int32 [n_bin, 2] on the '
                     'device of the input')
  names = list(dict.fromkeys(statistics))
  unknown = [s for s in names if s not in TIME_STATS]
  if unknown or not names:
    raise ValueError(f'statistics must be some of {TIME_STATS}: {statistics}')
  n_bin = int(bin_range.shape[0])
  outs = {s: torch.empty((n_outer, n_bin, n_point), dtype=x.dtype,
                         device=x.device) for s in names}
  mask = sum(1 << TIME_STATS.index(s) for s in names)
  out_ptrs = _lib.ptr_array([outs.get(s) for s in TIME_STATS])
  _launch('time_bin_stats', 'wb2_time_bin_stats', mask, _DTYPES[x.dtype],
          int(bool(skipna)), _lib.ptr(x), _lib.ptr(slab), n_outer, n_time,
          n_point, _lib.ptr(bin_range), n_bin, int(bins_per_group), out_ptrs,
          current_stream_ptr(x.device))
  return outs


SMOOTH_MODES = ('explicit', 'fast')  # WB2_SMOOTH_*, in order


def climatology_geometry(dtype: torch.dtype, wide: bool = False) -> dict:
  """Extents of the K14 moments kernel: `tile_points` adjacent points per
  workgroup, `members_ahead` members a thread requests before it combines
  any, `max_grid_outer` outer indices per grid row."""
  return _geometry('wb2_climatology_geometry', (_DTYPES[dtype], int(wide)),
                   [('tile_points', _I32), ('members_ahead', _I32),
                    ('max_grid_outer', _I32)])


def _check_series(x, slab, n_outer, n_time, lists):
  _require_float(x)
  _check_slab(slab, n_outer * n_time, 'n_outer * n_time')
  for name, a in lists.items():
    if a is not None and (a.dtype != torch.int32 or a.dim() != 1
                          or not a.is_contiguous() or a.device != x.device):
      raise ValueError(f'{name} must be a contiguous 1-D int32 tensor on the '
                       'device of the input')


def group_moments(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                  n_outer: int, n_time: int, n_point: int, group_begin,
                  member: torch.Tensor, fill: t.Optional[torch.Tensor] = None,
                  pivot: t.Optional[torch.Tensor] = None) -> tuple:
  """K14 moments: float64 (count, sum, sumsq), each [n_outer, n_group,
  n_point], of the groups of time steps of the series x[o, :, i], about
  `pivot` (float64 [n_outer, n_point], None = 0), from ONE launch and one
  read of `x`.  `group_begin` is a HOST sequence of n_group + 1 offsets into
  `member` (int32 device tensor of time steps, in time order; a step outside
  [0, n_time) is an absent sample); `fill` (int32 device tensor like `member`,
  or None) names the step read in the place of a NaN, negative for none.
  `slab` as for `time_bin_stats`."""
  _check_series(x, slab, n_outer, n_time, {'member': member, 'fill': fill})
  begin = np.ascontiguousarray(group_begin, dtype=np.int32)
  if begin.ndim != 1 or begin.size < 1:
    raise ValueError('group_begin must hold n_group + 1 offsets')
  n_group, n_member = begin.size - 1, int(member.numel())
  if fill is not None and fill.numel() != n_member:
    raise ValueError('fill must have one entry per member')
  if pivot is not None and (pivot.dtype != torch.float64
                            or pivot.numel() != n_outer * n_point
                            or not pivot.is_contiguous()
                            or pivot.device != x.device):
    raise ValueError('pivot must be a contiguous float64 [n_outer, n_point] '
                     'on the device of the input')
  begin_dev = torch.from_numpy(begin).to(x.device)
  outs = tuple(torch.empty((n_outer, n_group, n_point), dtype=torch.float64,
                           device=x.device) for _ in range(3))
  _launch('group_moments', 'wb2_group_moments', _DTYPES[x.dtype], _lib.ptr(x),
          _lib.ptr(slab), n_outer, n_time, n_point, _lib.ptr(begin_dev),
          begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_group,
          _lib.ptr(member), _lib.ptr(fill), n_member, _lib.ptr(pivot),
          _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
          current_stream_ptr(x.device))
  return outs


def first_finite(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                 n_outer: int, n_time: int, n_point: int,
                 member: torch.Tensor) -> torch.Tensor:
  """K14 pivot plane: float64 [n_outer, n_point], the first sample of every
  point, in the order of `member`, that is neither NaN nor +-inf; 0.0 if there
  is none."""
  _check_series(x, slab, n_outer, n_time, {'member': member})
  pivot = torch.empty((n_outer, n_point), dtype=torch.float64, device=x.device)
  _launch('first_finite', 'wb2_first_finite', _DTYPES[x.dtype], _lib.ptr(x),
          _lib.ptr(slab), n_outer, n_time, n_point, _lib.ptr(member),
          int(member.numel()), _lib.ptr(pivot), current_stream_ptr(x.device))
  return pivot


def cycle_smooth(mode: str, moments, pivot: t.Optional[torch.Tensor],
                 n_cycle: int, n_pos: int, weights: torch.Tensor,
                 want: t.Sequence[str] = ('mean', 'std')) -> dict:
  """K14 smoothing: {'mean' / 'std': float64 [n_outer, n_cycle * n_pos,
  n_point]} from the moments (count, sum, sumsq) of `group_moments`, whose
  groups are n_cycle cycles of n_pos positions, with the float64 device
  `weights` of an odd window; `mode` is 'explicit' or 'fast' (see
  include/wb2hip.h)."""
  if mode not in SMOOTH_MODES:
    raise ValueError(f'mode must be one of {SMOOTH_MODES}: {mode!r}')
  names = list(dict.fromkeys(want))
  if not names or any(s not in ('mean', 'std') for s in names):
    raise ValueError(f"want must be some of ('mean', 'std'): {want}")
  count, total, sumsq = moments
  n_outer, n_group, n_point = count.shape
  for a in (count, total, sumsq):
    if (a.dtype != torch.float64 or not a.is_contiguous()
        or a.shape != count.shape):
      raise ValueError('the moments must be contiguous float64 planes of one '
                       'shape')
  if n_group != n_cycle * n_pos:
    raise ValueError(f'{n_group} groups are not {n_cycle} cycles of {n_pos}')
  if (weights.dtype != torch.float64 or weights.dim() != 1
      or not weights.is_contiguous() or weights.device != count.device):
    raise ValueError('weights must be a contiguous float64 vector on the '
                     'device of the moments')
  if pivot is not None and (pivot.dtype != torch.float64
                            or pivot.numel() != n_outer * n_point
                            or not pivot.is_contiguous()):
    raise ValueError('pivot must be a contiguous float64 [n_outer, n_point]')
  outs = {s: torch.empty_like(count) for s in names}
  _launch('cycle_smooth', 'wb2_cycle_smooth', SMOOTH_MODES.index(mode),
          _lib.ptr(count), _lib.ptr(total), _lib.ptr(sumsq), _lib.ptr(pivot),
          n_outer, n_cycle, n_pos, n_point, _lib.ptr(weights),
          int(weights.numel()), _lib.ptr(outs.get('mean')),
          _lib.ptr(outs.get('std')), current_stream_ptr(count.device))
  return outs


def window_quantile_geometry(dtype: torch.dtype, n_year: int,
                             n_w: int) -> dict:
  """What the K15 launch chooses for groups of at most `n_year` members and a
  window of `n_w` weights: `tile_points` adjacent points and `positions`
  consecutive positions per workgroup, its `lds_bytes`, and the key bits
  settled per counting pass.  Raises where no tile fits the LDS."""
  return _geometry('wb2_window_quantile_geometry',
                   (_DTYPES[dtype], int(n_year), int(n_w)),
                   [('tile_points', _I32), ('positions', _I32),
                    ('lds_bytes', ctypes.c_int64),
                    ('key_bits_per_pass', _I32)])


def window_quantile(x: torch.Tensor, slab: t.Optional[torch.Tensor],
                    n_outer: int, n_time: int, n_point: int, group_begin,
                    n_cycle: int, n_pos: int, member: torch.Tensor,
                    fill: t.Optional[torch.Tensor], weights, quantiles,
                    dry_threshold: t.Optional[float] = None,
                    denominator: t.Optional[int] = None) -> tuple:
  """K15: (quantile, dry_fraction) of the rolling window over K14's groups g =
  c * n_pos + a, from ONE launch.  `weights` is a HOST sequence of an odd
  number of non-negative integers (the window, proportional to H - |k|),
  `quantiles` a HOST sequence in [0, 1].  quantile is float64 [n_q, n_outer,
  n_cycle * n_pos, n_point]: the weighted quantiles (include/wb2hip.h) of the
  samples X[y, (a + k) mod n_pos] that are not NaN and, with `dry_threshold`,
  not below it.  With `denominator` as well, dry_fraction is float64 [n_outer,
  n_cycle * n_pos, n_point]: the samples below the threshold / denominator;
  otherwise None.  `group_begin`, `member`, `fill`, `slab` as for
  `group_moments`."""
  _check_series(x, slab, n_outer, n_time, {'member': member, 'fill': fill})
  begin = np.ascontiguousarray(group_begin, dtype=np.int32)
  n_group = int(n_cycle) * int(n_pos)
  if begin.ndim != 1 or begin.size != n_group + 1:
    raise ValueError('group_begin must hold n_cycle * n_pos + 1 offsets')
  n_member = int(member.numel())
  if fill is not None and fill.numel() != n_member:
    raise ValueError('fill must have one entry per member')
  w = np.ascontiguousarray(weights, dtype=np.int32)
  q = np.ascontiguousarray(quantiles, dtype=np.float64)
  if w.ndim != 1 or q.ndim != 1:
    raise ValueError('weights and quantiles must be vectors')
  if denominator is not None and dry_threshold is None:
    raise ValueError('the dry fraction needs a dry threshold')
  begin_dev = torch.from_numpy(begin).to(x.device)
  quant = torch.empty((q.size, n_outer, n_group, n_point),
                      dtype=torch.float64, device=x.device)
  dry = None if denominator is None else torch.empty(
      (n_outer, n_group, n_point), dtype=torch.float64, device=x.device)
  _launch('window_quantile', 'wb2_window_quantile', _DTYPES[x.dtype],
          _lib.ptr(x), _lib.ptr(slab), n_outer, n_time, n_point,
          _lib.ptr(begin_dev),
          begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n_cycle),
          int(n_pos), _lib.ptr(member), _lib.ptr(fill), n_member,
          w.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(w.size),
          int(dry_threshold is not None),
          0.0 if dry_threshold is None else float(dry_threshold),
          int(denominator or 0),
          q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(q.size),
          _lib.ptr(quant), _lib.ptr(dry), current_stream_ptr(x.device))
  return quant, dry


# (input dtype, output dtype) pairs of K16; every other pair is refused
SCATTER_PAIRS = ((torch.float32, torch.float32), (torch.float64, torch.float64),
                 (torch.float64, torch.float32))


def slab_scatter_geometry(in_dtype: torch.dtype,
                          out_dtype: t.Optional[torch.dtype] = None,
                          wide: bool = False) -> dict:
  """Extents of the K16 kernel: `tile_points` adjacent points per workgroup,
  `max_grid_outer` sources per grid row."""
  out_dtype = in_dtype if out_dtype is None else out_dtype
  return _geometry('wb2_slab_scatter_geometry',
                   (dtype_code(in_dtype), dtype_code(out_dtype), int(wide)),
                   [('tile_points', _I32), ('max_grid_outer', _I32)])


def scatter_csr(src, dst, n_in_slab: int, n_out_slab: int) -> tuple:
  """(src_slab, dst_begin, dst_slab) as contiguous int64 HOST arrays, checked:
  `src` one input slab per entry (-1: a NaN source; an entry may repeat a
  slab), `dst` either a LIST of one sequence of output slabs per entry or the
  CSR pair as a TUPLE (dst_begin, dst_slab).  Every output slab of
  [0, n_out_slab) must be written exactly once and every source lie in
  [-1, n_in_slab): the kernel trusts the tables."""
  src = np.ascontiguousarray(src, dtype=np.int64).reshape(-1)
  if isinstance(dst, tuple):
    if len(dst) != 2 or np.ndim(dst[0]) != 1 or len(dst[0]) != src.size + 1:
      raise ValueError('the CSR form is (dst_begin[n_source + 1], dst_slab)')
    begin = np.ascontiguousarray(dst[0], dtype=np.int64)
    slabs = np.ascontiguousarray(dst[1], dtype=np.int64).reshape(-1)
  else:
    lists = [np.asarray(d, dtype=np.int64).reshape(-1) for d in dst]
    if len(lists) != src.size:
      raise ValueError('one destination list per source entry is needed: '
                       f'{len(lists)} lists, {src.size} sources')
    begin = np.zeros(src.size + 1, dtype=np.int64)
    np.cumsum([d.size for d in lists], out=begin[1:])
    slabs = (np.concatenate(lists) if lists else np.zeros(0, np.int64))
    slabs = np.ascontiguousarray(slabs, dtype=np.int64)
  if begin[0] != 0 or np.any(np.diff(begin) < 0) or begin[-1] != slabs.size:
    raise ValueError('dst_begin must ascend from 0 to the number of '
                     'destinations')
  if src.size and (src.min() < -1 or src.max() >= n_in_slab):
    raise IndexError(f'source slab out of range [-1, {n_in_slab})')
  if slabs.size and (slabs.min() < 0 or slabs.max() >= n_out_slab):
    raise IndexError(f'destination slab out of range [0, {n_out_slab})')
  written = np.bincount(slabs, minlength=n_out_slab)
  if np.any(written != 1):
    twice = np.flatnonzero(written > 1)
    never = np.flatnonzero(written == 0)
    raise ValueError(
        'every output slab must be written exactly once: '
        f'{twice.size} written more than once (first: {twice[:4].tolist()}), '
        f'{never.size} never (first: {never[:4].tolist()})')
  return src, begin, slabs


def slab_scatter(x: torch.Tensor, src, dst, n_out_slab: int, *,
                 n_point: t.Optional[int] = None,
                 out_dtype: t.Optional[torch.dtype] = None,
                 dests_per_group: int = 4,
                 out: t.Optional[torch.Tensor] = None,
                 checked: bool = False) -> torch.Tensor:
  """K16: [n_out_slab, n_point] of `out_dtype` (default: that of `x`) in which
  every slab listed for source entry s is the input slab `src[s]` cast to
  `out_dtype`, and NaN where `src[s]` is -1; each input slab is read once
  however many destinations it has.  Input slab k is the `n_point` elements
  (default: everything behind the first dim of `x`) that start `k * n_point`
  elements after the first element of `x`, so `x` is a contiguous tensor or a
  view whose table addresses intact slabs of its storage.  `src` and `dst` are
  HOST tables (`scatter_csr` checks them); `out`, if given, is the contiguous
  result to fill.  `checked` says that `src` and `dst` are what `scatter_csr`
  returned for this `n_out_slab` (a planner's CSR, perhaps shared by several
  variables): only the sources are then held against the storage of `x`.
  `dests_per_group` changes no result."""
  out_dtype = x.dtype if out_dtype is None else out_dtype
  if (x.dtype, out_dtype) not in SCATTER_PAIRS:
    raise TypeError(f'unsupported dtype pair {x.dtype} -> {out_dtype}')
  if n_point is None:
    n_point = int(np.prod(x.shape[1:], dtype=np.int64)) if x.dim() else 1
  n_point, n_out_slab = int(n_point), int(n_out_slab)
  if n_point < 0 or n_out_slab < 0 or int(dests_per_group) < 1:
    raise ValueError('bad sizes')
  # the elements of the storage from the first element of `x` on
  store = x.untyped_storage()
  reach = (store.nbytes() - (x.data_ptr() - store.data_ptr())
           ) // x.element_size() if x.numel() else 0
  n_in_slab = reach // max(n_point, 1)
  if checked:
    src, (begin, slabs) = src, dst
    if src.size and src.max() >= n_in_slab:
      raise IndexError(f'source slab out of range [-1, {n_in_slab})')
  else:
    src, begin, slabs = scatter_csr(src, dst, n_in_slab, n_out_slab)
  if out is None:
    out = torch.empty((n_out_slab, n_point), dtype=out_dtype, device=x.device)
  elif (out.dtype != out_dtype or out.numel() != n_out_slab * n_point
        or not out.is_contiguous() or out.device != x.device):
    raise ValueError('out must be a contiguous [n_out_slab, n_point] tensor of '
                     'the output dtype on the device of the input')
  if src.size == 0 or n_point == 0:
    return out
  tables = [upload_table(a, x.device) for a in (src, begin, slabs)]
  # (an empty input has no address; every source is -1 then, nothing is read)
  _launch('slab_scatter', 'wb2_slab_scatter', _DTYPES[x.dtype],
          _DTYPES[out_dtype], _lib.ptr(x if x.numel() else out),
          *[_lib.ptr(a) for a in tables],
          int(src.size), n_point, int(dests_per_group), _lib.ptr(out),
          current_stream_ptr(x.device))
  return out


# K17 copies bits: every dtype of 4 or 8 bytes the slicing layer hands it
BOX_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
BOX_FORMS = ('run', 'reversed', 'scalar', 'list')  # WB2_BOX_*, in order


def box_gather_geometry(dtype: torch.dtype, form: str, n_col_out: int) -> dict:
  """Extents of the K17 kernel for an output row of `n_col_out` columns in the
  column form `form` (one of BOX_FORMS): a workgroup owns `tile_rows` x
  `tile_cols` points of one output slab, `max_grid_outer` slabs per grid
  row."""
  return _geometry('wb2_box_gather_geometry',
                   (_box_elem_size(dtype), BOX_FORMS.index(form),
                    int(n_col_out)),
                   [('tile_rows', _I32), ('tile_cols', _I32),
                    ('max_grid_outer', _I32)])


def _box_elem_size(dtype: torch.dtype) -> int:
  if dtype not in BOX_DTYPES:
    raise TypeError(f'unsupported dtype {dtype}: the box gather moves '
                    'float32, float64, int32 and int64')
  return 4 if dtype in (torch.float32, torch.int32) else 8


def _upload_i32(table: np.ndarray, device) -> torch.Tensor:
  """An int32 table on the device, through the int64 table cache (padded to
  an even count and reinterpreted; the padding is never read)."""
  padded = np.zeros(table.size + table.size % 2, dtype=np.int32)
  padded[:table.size] = table
  return upload_table(padded.view(np.int64), device).view(torch.int32)


def _box_table(values, n: int, what: str) -> t.Optional[np.ndarray]:
  """`values` (None: identity) as a checked contiguous int32 HOST table of
  positions in [0, n)."""
  if values is None:
    return None
  table = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
  if table.size and (table.min() < 0 or table.max() >= n):
    raise IndexError(f'{what} out of range [0, {n})')
  return table.astype(np.int32)


def box_gather_form(x: torch.Tensor, out: torch.Tensor, n_col_in: int, cols
                    ) -> str:
  """The column form (one of BOX_FORMS) a `box_gather` of `x` into `out` with
  the columns `cols` takes."""
  is_list = not isinstance(cols, tuple)
  col0, step, n = (0, 1, len(cols)) if is_list else cols
  form = _lib.load().wb2_box_gather_form(
      _box_elem_size(x.dtype), _lib.ptr(x) or None, _lib.ptr(out) or None,
      int(n_col_in), int(col0), int(step), int(is_list), int(n))
  if form < 0:
    _lib.check(form, 'wb2_box_gather_form')
  return BOX_FORMS[form]


def box_gather(x: torch.Tensor, n_row_in: int, n_col_in: int, *,
               src_slab=None, n_out_slab: t.Optional[int] = None, rows=None,
               cols=None, out: t.Optional[torch.Tensor] = None
               ) -> torch.Tensor:
  """K17: [n_out_slab, n_row_out, n_col_out] of the dtype of `x` with
  out[s, i, j] = slab src_slab[s], row rows[i], column cols[j] of the input,
  bit for bit, from ONE launch.  Input slab k is the `n_row_in * n_col_in`
  elements that start `k` slabs after the first element of `x`, so `x` is a
  contiguous tensor or a view whose table addresses intact slabs of its
  storage (K13's convention).  `src_slab` (None: the first `n_out_slab` slabs
  in order, by default as many as `x` holds) and `rows` (None: all rows in order) are HOST sequences of
  positions; `cols` is None (all columns), a HOST sequence, or the affine run
  as a TUPLE (col0, step, count) with any non-zero step.  Every table is
  checked here against the input's storage: the kernel trusts them.  `out`, if
  given, is the contiguous result to fill."""
  elem = _box_elem_size(x.dtype)
  n_row_in, n_col_in = int(n_row_in), int(n_col_in)
  if n_row_in < 0 or n_col_in < 0:
    raise ValueError('bad sizes')
  slab = n_row_in * n_col_in
  # the elements of the storage from the first element of `x` on
  store = x.untyped_storage()
  reach = (store.nbytes() - (x.data_ptr() - store.data_ptr())
           ) // x.element_size() if x.numel() else 0
  n_in_slab = reach // slab if slab else 0
  if src_slab is None:
    n_out_slab = (x.numel() // slab if slab else 0) if n_out_slab is None \
        else int(n_out_slab)
    if not 0 <= n_out_slab <= n_in_slab and n_out_slab:
      raise IndexError(f'{n_out_slab} slabs leave the input\'s {n_in_slab}')
    slabs = None
  else:
    slabs = np.ascontiguousarray(src_slab, dtype=np.int64).reshape(-1)
    if n_out_slab is not None and int(n_out_slab) != slabs.size:
      raise ValueError('n_out_slab differs from the length of src_slab')
    n_out_slab = slabs.size
    if slabs.size and (slabs.min() < 0 or slabs.max() >= n_in_slab):
      raise IndexError(f'source slab out of range [0, {n_in_slab})')
  row = _box_table(rows, n_row_in, 'row')
  n_row_out = n_row_in if row is None else row.size
  if cols is None:
    cols = (0, 1, n_col_in)
  if isinstance(cols, tuple):
    col0, step, n_col_out = (int(v) for v in cols)
    col = None
    if step == 0:
      raise ValueError('the column step is zero')
    if n_col_out < 0:
      raise ValueError('bad sizes')
    last = col0 + (n_col_out - 1) * step
    if n_col_out and not (0 <= col0 < n_col_in and 0 <= last < n_col_in):
      raise IndexError(f'the column run ({col0}, {step}, {n_col_out}) leaves '
                       f'[0, {n_col_in})')
  else:
    col = _box_table(cols, n_col_in, 'column')
    col0, step, n_col_out = 0, 1, col.size
  shape = (n_out_slab, n_row_out, n_col_out)
  if out is None:
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
  elif (out.dtype != x.dtype or out.numel() != math.prod(shape)
        or not out.is_contiguous() or out.device != x.device):
    raise ValueError('out must be a contiguous [n_out_slab, n_row_out, '
                     'n_col_out] tensor of the dtype and on the device of the '
                     'input')
  if out.numel() == 0:
    return out
  slab_dev = None if slabs is None else upload_table(slabs, x.device)
  row_dev = None if row is None else _upload_i32(row, x.device)
  col_dev = None if col is None else _upload_i32(col, x.device)
  _launch('box_gather', 'wb2_box_gather', elem, _lib.ptr(x),
          _lib.ptr(slab_dev), n_out_slab, n_row_in, n_col_in,
          _lib.ptr(row_dev), n_row_out, col0, step, _lib.ptr(col_dev),
          n_col_out, _lib.ptr(out), current_stream_ptr(x.device))
  return out


def event_counts_geometry(dtype: torch.dtype, n_member: int, n_class: int,
                          n_threshold: int, wide: bool = False) -> dict:
  """Extents of the K18 counting kernel: a workgroup owns `rows_per_group`
  rows of one outer index, `thresholds_per_launch` thresholds share one read of
  the members, the histogram takes `lds_bytes` of LDS, `max_grid_outer` outer
  indices per grid row."""
  return _geometry('wb2_event_counts_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    int(n_threshold), int(wide)),
                   [('rows_per_group', _I32), ('thresholds_per_launch', _I32),
                    ('lds_bytes', ctypes.c_int64), ('max_grid_outer', _I32)])


def _reach(x: torch.Tensor) -> int:
  """Elements of the storage of `x` from its first element on."""
  store = x.untyped_storage()
  return (store.nbytes() - (x.data_ptr() - store.data_ptr())
          ) // x.element_size() if x.numel() else 0


def _event_slabs(table, n_outer: int, x: torch.Tensor, slab: int, extra: int,
                 what: str) -> t.Optional[np.ndarray]:
  """The HOST slab table `table` (None: identity) of `n_outer` entries,
  checked against the storage of `x`: every slab, and `extra` elements past
  its start (the further members), lie inside."""
  if table is None:
    lo, hi = 0, n_outer - 1
  else:
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1)
    if table.size != n_outer:
      raise ValueError(f'the {what} slab table must hold {n_outer} entries')
    lo, hi = (int(table.min()), int(table.max())) if n_outer else (0, -1)
  if n_outer and (lo < 0 or hi * slab + extra + slab > _reach(x)):
    raise IndexError(f'the {what} slabs leave the storage of the operand')
  return table


def _member_front(ens, member_stride, n_member, ens_slab, truth, truth_slab,
                  n_outer, n_row, n_col, thresholds=(), thr_slabs=None):
  """The preparation of every front end that reads members against a truth
  (K18 - K21, K24): the operand checks, then the HOST slab tables, checked
  against the operands' storage (`_event_slabs`) and uploaded.  ((n_member,
  member_stride, n_outer, n_row, n_col) as ints; the C arguments (dtype, ens,
  ens_slab, truth, truth_slab) or, without a point, None; the device table of
  the thresholds' slabs or None)."""
  _require_float(ens, truth, *thresholds)
  # (`ens` may be a view whose whole slabs its table addresses)
  _check_contiguous(ens.device, 'the device of the members', truth,
                    *thresholds, view=ens)
  n_member, n_outer, n_row, n_col, member_stride = (
      int(v) for v in (n_member, n_outer, n_row, n_col, member_stride))
  if min(n_outer, n_row, n_col) < 0 or member_stride < 0:
    raise ValueError('bad sizes')
  thr_slabs = list(thr_slabs) if thr_slabs is not None else [None] * len(
      thresholds)
  if len(thr_slabs) != len(thresholds):
    raise ValueError('one slab table (or None) per threshold')
  slab = n_row * n_col
  es = _event_slabs(ens_slab, n_outer, ens, slab,
                    (max(n_member, 1) - 1) * member_stride, 'member')
  ts = _event_slabs(truth_slab, n_outer, truth, slab, 0, 'truth')
  hs = [_event_slabs(tb, n_outer, x, slab, 0, 'threshold')
        for tb, x in zip(thr_slabs, thresholds)]
  sizes = (n_member, member_stride, n_outer, n_row, n_col)
  if slab * n_outer == 0:
    return sizes, None, None
  dev = ens.device
  hs_dev = None
  if any(tb is not None for tb in hs):
    ident = np.arange(n_outer, dtype=np.int64)
    hs_dev = upload_table(np.stack([ident if tb is None else tb
                                    for tb in hs]), dev)
  return sizes, (dtype_code(ens.dtype),
                 _lib.ptr(ens), _lib.ptr(None if es is None else
                                         upload_table(es, dev)),
                 _lib.ptr(truth), _lib.ptr(None if ts is None else
                                           upload_table(ts, dev))), hs_dev


def _event_front(ens, member_stride, n_member, ens_slab, truth, truth_slab,
                 thresholds, thr_slabs, n_outer, n_row, n_col):
  """`_member_front` with thresholds (K18 counts, K19 codes, K21 sums):
  ((n_threshold, n_member, n_outer, n_row, n_col) as ints, the leading C
  arguments that wb2_event_counts, wb2_event_codes and wb2_twcrps_sums share
  -- None where there is no point: nothing to upload)."""
  thresholds = list(thresholds)
  if not thresholds:
    raise ValueError('no thresholds')
  (n_member, member_stride, n_outer, n_row, n_col), args, hs_dev = (
      _member_front(ens, member_stride, n_member, ens_slab, truth, truth_slab,
                    n_outer, n_row, n_col, thresholds, thr_slabs))
  sizes = (len(thresholds), n_member, n_outer, n_row, n_col)
  if args is None:
    return sizes, None
  return sizes, args + (_lib.ptr_array(thresholds), _lib.ptr(hs_dev),
                        len(thresholds), n_member, member_stride, n_outer,
                        n_row, n_col)


def _check_members(n_member, geo: dict, takes: str) -> None:
  """`n_member` against a geometry dict ('the CRPS bin sums take')."""
  if not geo['min_member'] <= int(n_member) <= geo['max_member']:
    raise ValueError(f'{int(n_member)} members: {takes} '
                     f"{geo['min_member']} to {geo['max_member']}")


def _column_classes(col_class, n_col: int, n_class: int) -> np.ndarray:
  """`col_class` as int64[n_col], every value in [0, n_class)."""
  cls = np.ascontiguousarray(col_class, dtype=np.int64).reshape(-1)
  if cls.size != n_col or (n_col and (cls.min() < 0 or cls.max() >= n_class)):
    raise IndexError(f'col_class must hold {n_col} classes in [0, {n_class})')
  return cls


def event_counts(ens: torch.Tensor, member_stride: int, n_member: int,
                 ens_slab, truth: torch.Tensor, truth_slab,
                 thresholds: t.Sequence[torch.Tensor], thr_slabs, n_outer: int,
                 n_row: int, n_col: int, col_class, n_class: int
                 ) -> torch.Tensor:
  """K18: int32 [n_threshold, n_outer, n_row, n_class, n_code] counts of the
  points of every (row, column class) by code = observed * (M + 1) + members
  exceeding (2 (M + 1): truth or a member is NaN), n_code = 2 (M + 1) + 1.
  Member m of outer index o is the slab of `n_row * n_col` elements that starts
  `ens_slab[o]` slabs and `m * member_stride` ELEMENTS after the first element
  of `ens`; `truth_slab` and `thr_slabs[t]` address the truth and threshold t
  likewise.  The slab tables and `col_class` (class of every column, in
  [0, n_class)) are HOST sequences, None = identity; all of them are checked
  here against the operands' storage: the kernel trusts them.  Up to 4
  thresholds share one read of the members; the C side splits the rest."""
  (n_thr, n_member, n_outer, n_row, n_col), args = _event_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, thresholds,
      thr_slabs, n_outer, n_row, n_col)
  dev = ens.device
  n_class = int(n_class)
  out = torch.empty((n_thr, n_outer, n_row, n_class, 2 * (n_member + 1) + 1),
                    dtype=torch.int32, device=dev)
  cls = _column_classes(col_class, n_col, n_class)
  if args is None:  # no points: nothing to count
    return out.zero_()
  _launch('event_counts', 'wb2_event_counts', *args,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class,
          _lib.ptr(out), current_stream_ptr(dev))
  return out


def _fold_weights(wrow, mult, n_row: int, n_class: int, class_cols=None
                  ) -> tuple:
  """The HOST operands of a fold as it takes them: `wrow` float64 [n_region,
  n_row], `mult` int32 [n_region, n_class] and, where given, `class_cols`
  int32 [n_class] (else None)."""
  wrow = np.ascontiguousarray(wrow, dtype=np.float64)
  mult = np.ascontiguousarray(mult, dtype=np.int32)
  n_region = wrow.shape[0] if wrow.ndim == 2 else -1
  if wrow.shape != (n_region, n_row) or mult.shape != (n_region, n_class):
    raise ValueError('wrow must be [n_region, n_row] and mult [n_region, '
                     'n_class]')
  if class_cols is None:
    return wrow, mult, None
  cols = np.ascontiguousarray(class_cols, dtype=np.int32).reshape(-1)
  if cols.size != n_class:
    raise ValueError(f'class_cols must hold {n_class} column counts')
  return wrow, mult, cols


def _class_fold(label: str, sums: torch.Tensor, n_cell: int, n_slot: int,
                table_shape: tuple, wrow: np.ndarray, mult: np.ndarray
                ) -> torch.Tensor:
  """One wb2_crps_bin_fold launch under the hook label `label`: float64
  `table_shape` (n_cell x n_region x n_slot) of the class sums `sums` ([n_cell,
  n_row, n_class, n_slot] in memory); `wrow`, `mult`: `_fold_weights`'s."""
  dev = sums.device
  table = torch.empty(table_shape, dtype=torch.float64, device=dev)
  if table.numel():
    _launch(label, 'wb2_crps_bin_fold', _lib.ptr(sums), n_cell, wrow.shape[1],
            mult.shape[1], n_slot,
            _lib.ptr(upload_f64_table(wrow, dev) if wrow.size else None),
            _lib.ptr(_upload_i32(mult.reshape(-1), dev)), wrow.shape[0],
            _lib.ptr(table), current_stream_ptr(dev))
  return table


def event_fold(cnt: torch.Tensor, wrow, mult) -> torch.Tensor:
  """wb2_event_fold: float64 [n_threshold, n_outer, n_region, n_code] =
  sum_i wrow[r, i] * float(sum_c mult[r, c] * cnt[.., i, c, code]), the inner
  sum in int64, the rows in increasing order: a fixed order.  `wrow` (float64
  [n_region, n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays."""
  if cnt.dtype != torch.int32 or cnt.dim() != 5 or not cnt.is_contiguous():
    raise ValueError('cnt must be a contiguous int32 [threshold, outer, row, '
                     'class, code] tensor')
  n_thr, n_outer, n_row, n_class, n_code = (int(n) for n in cnt.shape)
  wrow, mult, _ = _fold_weights(wrow, mult, n_row, n_class)
  n_region = wrow.shape[0]
  dev = cnt.device
  out = torch.empty((n_thr, n_outer, n_region, n_code), dtype=torch.float64,
                    device=dev)
  if out.numel() == 0:
    return out
  _launch('event_fold', 'wb2_event_fold', _lib.ptr(cnt), n_thr * n_outer,
          n_row, n_class, n_code,
          _lib.ptr(upload_f64_table(wrow, dev) if wrow.size else None),
          _lib.ptr(_upload_i32(mult.reshape(-1), dev)), n_region,
          _lib.ptr(out), current_stream_ptr(dev))
  return out


def event_codes(ens: torch.Tensor, member_stride: int, n_member: int, ens_slab,
                truth: torch.Tensor, truth_slab,
                thresholds: t.Sequence[torch.Tensor], thr_slabs, n_outer: int,
                n_row: int, n_col: int) -> torch.Tensor:
  """K19, wb2_event_codes: uint16 [n_threshold, n_outer, n_row, n_col] codes
  k | observed << 8 | invalid << 9 of every point (k = the members exceeding;
  k = observed = 0 where the truth or a member is NaN).  The operands, the
  slab tables and their checks are those of `event_counts`."""
  (n_thr, _, n_outer, n_row, n_col), args = _event_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, thresholds,
      thr_slabs, n_outer, n_row, n_col)
  dev = ens.device
  out = torch.empty((n_thr, n_outer, n_row, n_col), dtype=torch.uint16,
                    device=dev)
  if args is not None:  # (no points: no codes)
    _launch('event_codes', 'wb2_event_codes', *args, _lib.ptr(out),
            current_stream_ptr(dev))
  return out


def crps_bins_geometry(dtype: torch.dtype, n_member: int = 1,
                       n_class: int = 1) -> dict:
  """Extents of the K20 sums kernel: the member counts it takes
  (`min_member` .. `max_member`), the `tile_cols` columns a wave sorts at a
  time, `rows_per_group` = 1 (a row is one wave, a workgroup of its own), the
  `lds_bytes` of its tile, `max_grid_outer` outer indices per grid row."""
  return _geometry('wb2_crps_bins_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class)),
                   [('min_member', _I32), ('max_member', _I32),
                    ('tile_cols', _I32), ('rows_per_group', _I32),
                    ('lds_bytes', ctypes.c_int64), ('max_grid_outer', _I32)])


def crps_bin_sums(ens: torch.Tensor, member_stride: int, n_member: int,
                  ens_slab, truth: torch.Tensor, truth_slab, n_outer: int,
                  n_row: int, n_col: int, col_class, n_class: int) -> tuple:
  """K20, wb2_crps_bin_sums: (float64 [n_outer, n_row, n_class, 2, n_member +
  1] sums of alpha and beta, int32 [n_outer, n_row, n_class, 3] below / above /
  valid counts) of the points of every (row, column class).  The operands,
  the HOST slab tables and `col_class` are those of `event_counts`, checked
  here against the operands' storage in the same way: the kernel trusts
  them."""
  _require_float(ens, truth)
  _check_members(n_member, crps_bins_geometry(ens.dtype, 1, 1),
                 'the CRPS bin sums take')
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  n_class = int(n_class)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  sums = torch.empty((n_outer, n_row, n_class, 2, n_member + 1),
                     dtype=torch.float64, device=dev)
  cnt = torch.empty((n_outer, n_row, n_class, 3), dtype=torch.int32,
                    device=dev)
  if args is None:  # no points: nothing to add
    return sums.zero_(), cnt.zero_()
  _launch('crps_bin_sums', 'wb2_crps_bin_sums', *args, n_member,
          member_stride, n_outer, n_row, n_col,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class,
          _lib.ptr(sums), _lib.ptr(cnt), current_stream_ptr(dev))
  return sums, cnt


def crps_bin_fold(sums: torch.Tensor, cnt: torch.Tensor, class_cols, wrow,
                  mult) -> tuple:
  """(float64 [n_outer, n_region, 2, n_bin], float64 [n_outer, n_region, 4]):
  wb2_crps_bin_fold of the sums -- sum_i wrow[r, i] * (sum_c float(mult[r, c])
  * sums[o, i, c]), classes then rows in increasing order, plain float64 -- and
  wb2_event_fold of the counts (below, above, valid, invalid = `class_cols[c]`
  - valid).  `class_cols` (columns per class), `wrow` (float64 [n_region,
  n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays."""
  if (sums.dtype != torch.float64 or sums.dim() != 5 or sums.shape[3] != 2 or
      not sums.is_contiguous() or cnt.dtype != torch.int32 or
      tuple(cnt.shape) != tuple(sums.shape[:3]) + (3,) or
      not cnt.is_contiguous() or cnt.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [outer, row, class, '
                     '2, bin] tensor and cnt its int32 [outer, row, class, 3]')
  n_outer, n_row, n_class, _, n_bin = (int(n) for n in sums.shape)
  wrow, mult, cols = _fold_weights(wrow, mult, n_row, n_class, class_cols)
  table = _class_fold('crps_bin_fold', sums, n_outer, 2 * n_bin,
                      (n_outer, wrow.shape[0], 2, n_bin), wrow, mult)
  invalid = _upload_i32(cols, sums.device)[:n_class].reshape(
      1, 1, n_class) - cnt[..., 2]
  cnt4 = torch.cat([cnt, invalid[..., None].to(torch.int32)], dim=-1)
  return table, event_fold(cnt4[None].contiguous(), wrow, mult)[0]


def twcrps_geometry(dtype: torch.dtype, n_member: int = 1, n_class: int = 1,
                    n_threshold: int = 1) -> dict:
  """Extents of the K21 sums kernel: the member counts it takes (`min_member`
  .. `max_member`), the `thresholds_per_launch` that share one read and one
  sort of the members, the `tile_cols` columns a wave sorts at a time,
  `rows_per_group` = 1 (a row is one wave, a workgroup of its own), the
  `lds_bytes` of its tile, `max_grid_outer` outer indices per grid row."""
  return _geometry('wb2_twcrps_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    int(n_threshold)),
                   [('min_member', _I32), ('max_member', _I32),
                    ('thresholds_per_launch', _I32), ('tile_cols', _I32),
                    ('rows_per_group', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_grid_outer', _I32)])


def twcrps_sums(ens: torch.Tensor, member_stride: int, n_member: int,
                ens_slab, truth: torch.Tensor, truth_slab,
                thresholds: t.Sequence[torch.Tensor], thr_slabs, n_outer: int,
                n_row: int, n_col: int, col_class, n_class: int,
                lower: bool = False) -> tuple:
  """K21, wb2_twcrps_sums: (float64 [n_threshold, n_outer, n_row, n_class, 2]
  sums of A and B, int32 [n_threshold, n_outer, n_row, n_class, 1] valid
  counts) of the points of every (threshold, row, column class); `lower`
  picks the tail (v = min(z, t) instead of max(z, t)).  The operands, the HOST
  slab tables and `col_class` are those of `event_counts`, checked here against
  the operands' storage in the same way: the kernel trusts them.  Up to 4
  thresholds share one read and one sort of the members; the C side splits the
  rest."""
  n_class = int(n_class)
  thresholds = list(thresholds)
  _require_float(ens, truth, *thresholds)
  _check_members(n_member, twcrps_geometry(ens.dtype), 'the twCRPS sums take')
  (n_thr, n_member, n_outer, n_row, n_col), args = _event_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, thresholds,
      thr_slabs, n_outer, n_row, n_col)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  sums = torch.empty((n_thr, n_outer, n_row, n_class, 2), dtype=torch.float64,
                     device=dev)
  cnt = torch.empty((n_thr, n_outer, n_row, n_class, 1), dtype=torch.int32,
                    device=dev)
  if args is None:  # no points: nothing to add
    return sums.zero_(), cnt.zero_()
  _launch('twcrps_sums', 'wb2_twcrps_sums', *args,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class,
          int(bool(lower)), _lib.ptr(sums), _lib.ptr(cnt),
          current_stream_ptr(dev))
  return sums, cnt


def twcrps_fold(sums: torch.Tensor, cnt: torch.Tensor, class_cols, wrow,
                mult) -> tuple:
  """(float64 [n_threshold, n_outer, n_region, 2], float64 [n_threshold,
  n_outer, n_region, 2]): wb2_crps_bin_fold of the sums of A and B (n_cell =
  n_threshold * n_outer, n_slot = 2) -- sum_i wrow[r, i] * (sum_c float(mult[r,
  c]) * sums[t, o, i, c]), classes then rows in increasing order, plain
  float64 -- and wb2_event_fold of the counts (valid, invalid = `class_cols[c]`
  - valid).  `class_cols` (columns per class), `wrow` (float64 [n_region,
  n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays."""
  if (sums.dtype != torch.float64 or sums.dim() != 5 or sums.shape[4] != 2 or
      not sums.is_contiguous() or cnt.dtype != torch.int32 or
      tuple(cnt.shape) != tuple(sums.shape[:4]) + (1,) or
      not cnt.is_contiguous() or cnt.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [threshold, outer, '
                     'row, class, 2] tensor and cnt its int32 [threshold, '
                     'outer, row, class, 1]')
  n_thr, n_outer, n_row, n_class, _ = (int(n) for n in sums.shape)
  wrow, mult, cols = _fold_weights(wrow, mult, n_row, n_class, class_cols)
  table = _class_fold('twcrps_fold', sums, n_thr * n_outer, 2,
                      (n_thr, n_outer, wrow.shape[0], 2), wrow, mult)
  invalid = _upload_i32(cols, sums.device)[:n_class].reshape(
      1, 1, 1, n_class, 1) - cnt
  cnt2 = torch.cat([cnt, invalid.to(torch.int32)], dim=-1)
  return table, event_fold(cnt2.contiguous(), wrow, mult)


CONDITIONAL_MODES = {'spread': 0, 'forecast': 1, 'truth': 2}
CONDITIONAL_TERMS = 4  # mu, y, s2, se


def conditional_geometry(dtype: torch.dtype, n_member: int = 1,
                         n_class: int = 1, n_edge: int = 0) -> dict:
  """Extents of the K24 sums kernel: the member counts it takes (`min_member`
  .. `max_member`), the `max_edges` bin edges (one bin more), the `tile_cols`
  columns a wave bins at a time, `rows_per_group` = 1 (a row is one wave, a
  workgroup of its own), the `lds_bytes` of its tile, `max_grid_outer` outer
  indices per grid row."""
  return _geometry('wb2_conditional_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    int(n_edge)),
                   [('min_member', _I32), ('max_member', _I32),
                    ('max_edges', _I32), ('tile_cols', _I32),
                    ('rows_per_group', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_grid_outer', _I32)])


def conditional_edges(edges, max_edges: int = 63) -> np.ndarray:
  """`edges` as the float64 [n_edge] array the K24 kernel compares against:
  finite, strictly increasing, at most `max_edges` (ValueError otherwise)."""
  e = np.ascontiguousarray(edges, dtype=np.float64)
  if e.ndim != 1:
    raise ValueError('the bin edges must be a 1-D sequence')
  if e.size > max_edges:
    raise ValueError(f'{e.size} bin edges: the conditional sums take 0 to '
                     f'{max_edges}')
  if not np.isfinite(e).all():
    raise ValueError('the bin edges must be finite')
  if e.size > 1 and not (e[1:] > e[:-1]).all():
    raise ValueError('the bin edges must be strictly increasing')
  return e


def conditional_sums(ens: torch.Tensor, member_stride: int, n_member: int,
                     ens_slab, truth: torch.Tensor, truth_slab, n_outer: int,
                     n_row: int, n_col: int, col_class, n_class: int,
                     mode, edges) -> tuple:
  """K24, wb2_conditional_sums: (float64 [n_outer, n_row, n_class, n_bin, 4]
  sums of mu, y, s2 and se, int32 [n_outer, n_row, n_class, n_bin] counts) of
  the valid points of every (row, column class, bin).  `mode` is 'spread',
  'forecast' or 'truth' (or 0, 1, 2): what is binned; `edges` is a HOST
  sequence of n_bin - 1 finite, strictly increasing values in the units of
  that quantity (for 'spread': of the VARIANCE, that is, already squared).
  The operands, the HOST slab tables and `col_class` are those of
  `event_counts`; all of them and the edges are checked here: the kernel
  trusts them."""
  _require_float(ens, truth)
  mode = CONDITIONAL_MODES.get(mode, mode)
  if mode not in (0, 1, 2):
    raise ValueError(f'mode={mode!r}: the conditional sums take '
                     f'{", ".join(map(repr, CONDITIONAL_MODES))}')
  geo = conditional_geometry(ens.dtype)
  _check_members(n_member, geo, 'the conditional sums take')
  e = conditional_edges(edges, geo['max_edges'])
  n_bin = e.size + 1
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  n_class = int(n_class)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  sums = torch.empty((n_outer, n_row, n_class, n_bin, CONDITIONAL_TERMS),
                     dtype=torch.float64, device=dev)
  cnt = torch.empty((n_outer, n_row, n_class, n_bin), dtype=torch.int32,
                    device=dev)
  if args is None:  # no points: nothing to add
    return sums.zero_(), cnt.zero_()
  _launch('conditional_sums', 'wb2_conditional_sums', *args, n_member,
          member_stride, n_outer, n_row, n_col,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class, mode,
          _lib.ptr(upload_f64_table(e, dev) if e.size else None), e.size,
          _lib.ptr(sums), _lib.ptr(cnt), current_stream_ptr(dev))
  return sums, cnt


def conditional_fold(sums: torch.Tensor, cnt: torch.Tensor, class_cols, wrow,
                     mult) -> tuple:
  """(float64 [n_outer, n_region, n_bin, 4], float64 [n_outer, n_region,
  n_bin + 1]): wb2_crps_bin_fold of the sums (n_slot = 4 n_bin) -- sum_i
  wrow[r, i] * (sum_c float(mult[r, c]) * sums[o, i, c]), classes then rows in
  increasing order, plain float64 -- and wb2_event_fold of the counts (the
  bins, then invalid = `class_cols[c]` - the bins' total).  `class_cols`
  (columns per class), `wrow` (float64 [n_region, n_row]) and `mult` (int32
  [n_region, n_class]) are HOST arrays."""
  if (sums.dtype != torch.float64 or sums.dim() != 5 or
      sums.shape[4] != CONDITIONAL_TERMS or not sums.is_contiguous() or
      cnt.dtype != torch.int32 or tuple(cnt.shape) != tuple(sums.shape[:4]) or
      not cnt.is_contiguous() or cnt.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [outer, row, class, '
                     'bin, 4] tensor and cnt its int32 [outer, row, class, '
                     'bin]')
  n_outer, n_row, n_class, n_bin, _ = (int(n) for n in sums.shape)
  wrow, mult, cols = _fold_weights(wrow, mult, n_row, n_class, class_cols)
  table = _class_fold('conditional_fold', sums, n_outer,
                      CONDITIONAL_TERMS * n_bin,
                      (n_outer, wrow.shape[0], n_bin, CONDITIONAL_TERMS), wrow,
                      mult)
  invalid = _upload_i32(cols, sums.device)[:n_class].reshape(
      1, 1, n_class) - cnt.sum(dim=-1)
  codes = torch.cat([cnt, invalid[..., None].to(torch.int32)], dim=-1)
  return table, event_fold(codes[None].contiguous(), wrow, mult)[0]


JOINT_SIDES = {'right': 0, 'left': 1}


def joint_geometry(dtype: torch.dtype, n_member: int = 1, n_class: int = 1,
                   n_edge: int = 0, wide: bool = False) -> dict:
  """Extents of the K26 counting kernel: a workgroup owns `rows_per_group`
  rows of one outer index, the histogram takes `lds_bytes` of LDS, at most
  `max_edges` bin edges (one category more), `max_grid_outer` outer indices
  per grid row.  A histogram that does not fit is refused here as in
  `joint_counts`."""
  return _geometry('wb2_joint_counts_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    int(n_edge), int(wide)),
                   [('rows_per_group', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_edges', _I32), ('max_grid_outer', _I32)])


def joint_edges(edges) -> np.ndarray:
  """`edges` as the float64 [n_edge] array the K26 kernel compares against:
  finite, strictly increasing, at most the kernel's `max_edges` (ValueError
  otherwise)."""
  cap = joint_geometry(torch.float32)['max_edges']
  e = np.ascontiguousarray(edges, dtype=np.float64)
  if e.ndim == 1 and e.size > cap:
    raise ValueError(f'{e.size} bin edges: the joint counts take 0 to {cap}')
  return conditional_edges(e, cap)


def joint_counts(ens: torch.Tensor, member_stride: int, n_member: int,
                 ens_slab, truth: torch.Tensor, truth_slab, n_outer: int,
                 n_row: int, n_col: int, col_class, n_class: int, edges,
                 side='right') -> torch.Tensor:
  """K26, wb2_joint_counts: int32 [n_outer, n_row, n_class, B * B + 1] counts
  of every (row, column class): code = bin(truth) * B + bin(member) gets +1 per
  member of a valid point, code = B * B +1 per invalid point (truth or a member
  is NaN); B = len(edges) + 1.  `side` is 'right' (bin = #{k : edge_k <= v}) or
  'left' (#{k : edge_k < v}), or 0 / 1; `edges` is a HOST sequence of finite,
  strictly increasing values.  The operands, the HOST slab tables and
  `col_class` are those of `event_counts`; all of them and the edges are
  checked here: the kernel trusts them."""
  _require_float(ens, truth)
  side = JOINT_SIDES.get(side, side)
  if side not in (0, 1):
    raise ValueError(f'side={side!r}: the joint counts take '
                     f'{", ".join(map(repr, JOINT_SIDES))}')
  e = joint_edges(edges)
  n_class = int(n_class)
  if not 1 <= int(n_member) <= 128:  # (wb2_joint_counts' own limits)
    raise ValueError(f'{int(n_member)} members: the joint counts take 1 to 128')
  # (the classes and the LDS budget: refused here)
  joint_geometry(ens.dtype, n_member, n_class, e.size)
  n_code = (e.size + 1) ** 2 + 1
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  cnt = torch.empty((n_outer, n_row, n_class, n_code), dtype=torch.int32,
                    device=dev)
  if args is None:  # no points: nothing to count
    return cnt.zero_()
  _launch('joint_counts', 'wb2_joint_counts', *args, n_member, member_stride,
          n_outer, n_row, n_col,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class,
          _lib.ptr(upload_f64_table(e, dev) if e.size else None), e.size, side,
          _lib.ptr(cnt), current_stream_ptr(dev))
  return cnt


def joint_fold(cnt: torch.Tensor, wrow, mult) -> torch.Tensor:
  """float64 [n_outer, n_region, n_code]: wb2_event_fold of the joint counts
  (int32 [n_outer, n_row, n_class, n_code]).  `wrow` (float64 [n_region,
  n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays."""
  if cnt.dtype != torch.int32 or cnt.dim() != 4 or not cnt.is_contiguous():
    raise ValueError('cnt must be a contiguous int32 [outer, row, class, code] '
                     'tensor')
  return event_fold(cnt[None], wrow, mult)[0]


VARIOGRAM_ORDERS = {0.5: 0, 1.0: 1, 2.0: 2}  # order -> wb2_variogram_sums' code
VARIOGRAM_TERMS = 3  # gy, gf, sc


def variogram_order(order) -> int:
  """The order code (0, 1, 2) of the order 0.5, 1 or 2 (ValueError
  otherwise)."""
  try:
    return VARIOGRAM_ORDERS[float(order)]
  except (KeyError, TypeError, ValueError):
    raise ValueError(f'order={order!r}: the variogram sums take 0.5, 1 and '
                     '2') from None


def variogram_lags(lags) -> np.ndarray:
  """`lags` as the HOST int32 [n_lag, 2] array of (row offset a >= 0, column
  offset b) pairs that wb2_variogram_sums takes: whole numbers, no (0, 0), no
  pair twice (ValueError otherwise; the kernel's own limits are its to
  check)."""
  try:
    given = np.asarray(lags)
    arr = np.ascontiguousarray(given, dtype=np.int64)
    ok = (arr.ndim == 2 and arr.shape[1] == 2 and arr.shape[0] >= 1 and
          given.dtype != bool and
          bool(np.all(np.asarray(given, dtype=np.float64) == arr)))
  except (TypeError, ValueError, OverflowError):
    ok = False
  if not ok:
    raise ValueError('the lags must be a non-empty sequence of (row offset, '
                     'column offset) pairs of whole numbers')
  if (arr[:, 0] < 0).any():
    raise ValueError('a lag\'s row offset must be >= 0 (take the opposite '
                     'lag: it pairs the same points)')
  if ((arr[:, 0] == 0) & (arr[:, 1] == 0)).any():
    raise ValueError('the lag (0, 0) pairs a point with itself')
  if len({tuple(p) for p in arr.tolist()}) != arr.shape[0]:
    raise ValueError('the lags must differ: a lag is given twice')
  if np.abs(arr).max() >= 2 ** 31:
    raise ValueError('the lags are out of range')
  return np.ascontiguousarray(arr, dtype=np.int32)


def variogram_geometry(dtype: torch.dtype, n_member: int = 1,
                       n_class: int = 1, order=0.5, lags=((0, 1),)) -> dict:
  """Extents of the K27 sums kernel: the member counts it takes (`min_member`
  .. `max_member`), `max_lags`, the largest row offset `max_row_offset` and
  column offset `max_col_offset` of a lag, the `tile_cols` columns a wave
  walks at a time, `rows_per_group` = 1 (a row is one wave, a workgroup of its
  own), the `lds_bytes` of the strips and the tile of THESE lags,
  `max_grid_outer` outer indices per grid row.  Lags past the limits or over
  the LDS budget are refused here as in `variogram_sums`."""
  lg = variogram_lags(lags)
  return _geometry('wb2_variogram_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    variogram_order(order), lg.ctypes.data, lg.shape[0]),
                   [('min_member', _I32), ('max_member', _I32),
                    ('max_lags', _I32), ('max_row_offset', _I32),
                    ('max_col_offset', _I32), ('tile_cols', _I32),
                    ('rows_per_group', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_grid_outer', _I32)])


def variogram_sums(ens: torch.Tensor, member_stride: int, n_member: int,
                   ens_slab, truth: torch.Tensor, truth_slab, n_outer: int,
                   n_row: int, n_col: int, col_class, n_class: int, order,
                   lags) -> tuple:
  """K27, wb2_variogram_sums: (float64 [n_outer, n_row, n_class, n_lag, 3] sums
  of gy, gf and sc over the valid pairs, int32 [n_outer, n_row, n_class,
  n_lag, 2] counts of the valid and the invalid pairs) of every (anchor row,
  anchor's column class, lag).  `order` is 0.5, 1 or 2; `lags` is a HOST
  sequence of (a, b) pairs in grid points, a >= 0, longitude cyclic.  The
  operands, the HOST slab tables and `col_class` are those of `event_counts`;
  all of them and the lags are checked here: the kernel trusts the tables."""
  _require_float(ens, truth)
  code = variogram_order(order)
  lg = variogram_lags(lags)
  n_lag = lg.shape[0]
  n_class = int(n_class)
  geo = variogram_geometry(ens.dtype)
  _check_members(n_member, geo, 'the variogram sums take')
  if n_lag > geo['max_lags']:
    raise ValueError(f'{n_lag} lags: the variogram sums take 1 to '
                     f"{geo['max_lags']}")
  if lg[:, 0].max() > geo['max_row_offset']:
    raise ValueError(f'row offset {int(lg[:, 0].max())}: the variogram sums '
                     f"take 0 to {geo['max_row_offset']}")
  reach = int(np.abs(lg[:, 1]).max())
  if reach > geo['max_col_offset'] or (int(n_col) > 0 and reach >= int(n_col)):
    raise ValueError(f'column offset of size {reach}: the variogram sums take '
                     f"up to {geo['max_col_offset']}, below n_col={int(n_col)}")
  # (the classes and the LDS budget of these lags: refused here)
  variogram_geometry(ens.dtype, n_member, n_class, order, lg)
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  sums = torch.empty((n_outer, n_row, n_class, n_lag, VARIOGRAM_TERMS),
                     dtype=torch.float64, device=dev)
  cnt = torch.empty((n_outer, n_row, n_class, n_lag, 2), dtype=torch.int32,
                    device=dev)
  if args is None:  # no points: no pairs
    return sums.zero_(), cnt.zero_()
  _launch('variogram_sums', 'wb2_variogram_sums', *args, n_member,
          member_stride, n_outer, n_row, n_col,
          _lib.ptr(_upload_i32(cls.astype(np.int32), dev)), n_class, code,
          lg.ctypes.data, n_lag, _lib.ptr(sums), _lib.ptr(cnt),
          current_stream_ptr(dev))
  return sums, cnt


def variogram_fold(sums: torch.Tensor, cnt: torch.Tensor, class_cols, wrow,
                   mult) -> tuple:
  """(float64 [n_outer, n_region, n_lag, 3], float64 [n_outer, n_region, n_lag,
  2]): wb2_crps_bin_fold of the sums (n_slot = 3 n_lag) -- sum_i wrow[r, i] *
  (sum_c float(mult[r, c]) * sums[o, i, c]), classes then rows in increasing
  order, plain float64 -- and wb2_event_fold of the counts (n_code = 2 n_lag:
  per lag the valid and the invalid pairs).  `wrow` (float64 [n_region,
  n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays; `class_cols`
  is not needed (absent pairs are no invalid ones) and only checked."""
  if (sums.dtype != torch.float64 or sums.dim() != 5 or
      sums.shape[4] != VARIOGRAM_TERMS or not sums.is_contiguous() or
      cnt.dtype != torch.int32 or
      tuple(cnt.shape) != tuple(sums.shape[:4]) + (2,) or
      not cnt.is_contiguous() or cnt.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [outer, row, class, '
                     'lag, 3] tensor and cnt its int32 [outer, row, class, '
                     'lag, 2]')
  n_outer, n_row, n_class, n_lag, _ = (int(n) for n in sums.shape)
  wrow, mult, _ = _fold_weights(wrow, mult, n_row, n_class, class_cols)
  table = _class_fold('crps_bin_fold', sums, n_outer, VARIOGRAM_TERMS * n_lag,
                      (n_outer, wrow.shape[0], n_lag, VARIOGRAM_TERMS), wrow,
                      mult)
  codes = cnt.reshape(1, n_outer, n_row, n_class, 2 * n_lag)
  return table, event_fold(codes, wrow, mult)[0].reshape(
      n_outer, wrow.shape[0], n_lag, 2)


QUANTILE_SCORE_METHODS = ('linear', 'hazen', 'weibull')
QUANTILE_SCORE_TERMS = 2  # pinball, q
# those of wb2_quantile_score_geometry, and the levels of a table
QUANTILE_SCORE_MAX_MEMBER = 64
QUANTILE_SCORE_LAUNCH_LEVELS = 16
QUANTILE_SCORE_MAX_LEVELS = 64


def quantile_score_levels(levels, n_member: int, method: str = 'linear',
                          direct: bool = False) -> tuple:
  """The HOST tables of wb2_quantile_score_sums for `levels` and `n_member`
  sorted members: (int32 lo, int32 hi, float64 t, float64 tau, float64 1 -
  tau), each [n_level].  The 0-based position of level tau is v = tau (M - 1)
  ('linear'), M tau - 1/2 ('hazen') or (M + 1) tau - 1 ('weibull'), clamped to
  [0, M - 1], all in float64; lo = floor(v), t = v - lo, hi = min(lo + 1, M -
  1).  `direct`: the members ARE the quantile forecasts of the levels, in
  their order: lo = hi = the level's index, t = 0, and `method` is not asked.
  Checked (ValueError): the method, 1 to 64 members, levels that are a
  non-empty 1-D sequence of finite numbers in [0, 1], strictly increasing, at
  most 64 (direct: at most 16, and as many as members).  Needs no GPU."""
  if not direct and method not in QUANTILE_SCORE_METHODS:
    raise ValueError(f'method={method!r}: the quantile score takes '
                     f'{", ".join(map(repr, QUANTILE_SCORE_METHODS))}')
  try:
    tau = np.ascontiguousarray(levels, dtype=np.float64)
  except (TypeError, ValueError):
    raise ValueError('the levels must be numbers') from None
  if tau.ndim != 1 or tau.size == 0:
    raise ValueError('the levels must be a non-empty 1-D sequence')
  if not np.isfinite(tau).all():
    raise ValueError('the levels must be finite')
  if tau.min() < 0.0 or tau.max() > 1.0:
    raise ValueError('the levels must lie within [0, 1]')
  if tau.size > 1 and not (tau[1:] > tau[:-1]).all():
    raise ValueError('the levels must be strictly increasing')
  most = QUANTILE_SCORE_LAUNCH_LEVELS if direct else QUANTILE_SCORE_MAX_LEVELS
  if tau.size > most:
    raise ValueError(f'{tau.size} levels: the quantile score takes 1 to {most}'
                     + (' quantile forecasts' if direct else ''))
  n_member = int(n_member)
  if not 1 <= n_member <= QUANTILE_SCORE_MAX_MEMBER:
    raise ValueError(f'{n_member} members: the quantile score takes 1 to '
                     f'{QUANTILE_SCORE_MAX_MEMBER}')
  if direct:
    if tau.size != n_member:
      raise ValueError(f'{tau.size} levels for {n_member} quantile forecasts')
    lo = np.arange(n_member, dtype=np.int32)
    return lo, lo.copy(), np.zeros(n_member), tau, 1.0 - tau
  m = float(n_member)
  if method == 'linear':
    v = tau * (m - 1.0)
  elif method == 'hazen':
    v = m * tau - 0.5
  else:
    v = (m + 1.0) * tau - 1.0
  v = np.minimum(np.maximum(v, 0.0), m - 1.0)
  lo = np.floor(v)
  t = v - lo
  lo = lo.astype(np.int32)
  hi = np.minimum(lo + 1, n_member - 1).astype(np.int32)
  return lo, hi, t, tau, 1.0 - tau


def _quantile_score_tables(tables, n_member: int, direct: bool) -> tuple:
  """`tables` (those of `quantile_score_levels`) as the contiguous arrays the
  kernel reads, checked against `n_member`: it trusts them."""
  try:
    lo, hi, t, tau, omt = tables
  except (TypeError, ValueError):
    raise ValueError('the level tables must be (lo, hi, t, tau, 1 - tau)'
                     ) from None
  lo = np.ascontiguousarray(lo, dtype=np.int32)
  hi = np.ascontiguousarray(hi, dtype=np.int32)
  t, tau, omt = (np.ascontiguousarray(a, dtype=np.float64)
                 for a in (t, tau, omt))
  n_level = lo.size
  if n_level < 1 or any(a.shape != (n_level,) for a in (lo, hi, t, tau, omt)):
    raise ValueError('the level tables must be non-empty 1-D arrays of one '
                     'length')
  if (lo < 0).any() or (lo > hi).any() or (hi >= int(n_member)).any():
    raise ValueError('the level tables need 0 <= lo <= hi < n_member='
                     f'{int(n_member)}')
  if direct and (lo != hi).any():
    raise ValueError('direct quantiles need lo == hi')
  if not (np.isfinite(t).all() and (t >= 0).all() and (t < 1).all()):
    raise ValueError('the level tables need 0 <= t < 1')
  return lo, hi, t, tau, omt


def quantile_score_geometry(dtype: torch.dtype, n_member: int = 1,
                            n_class: int = 1, n_level: int = 1,
                            direct: bool = False) -> dict:
  """Extents of the K28 sums kernel: the member counts it takes (`min_member`
  .. `max_member`), the `max_levels` of one launch, the `tile_cols` columns a
  wave walks at a time, `rows_per_group` = 1 (a row is one wave, a workgroup
  of its own), the `lds_bytes` of the tile of THESE members and levels,
  `max_grid_outer` outer indices per grid row.  Sizes past the limits or over
  the LDS budget are refused here as in `quantile_score_sums`."""
  return _geometry('wb2_quantile_score_geometry',
                   (dtype_code(dtype), int(n_member), int(n_class),
                    int(bool(direct)), int(n_level)),
                   [('min_member', _I32), ('max_member', _I32),
                    ('max_levels', _I32), ('tile_cols', _I32),
                    ('rows_per_group', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_grid_outer', _I32)])


def quantile_score_sums(ens: torch.Tensor, member_stride: int, n_member: int,
                        ens_slab, truth: torch.Tensor, truth_slab,
                        n_outer: int, n_row: int, n_col: int, col_class,
                        n_class: int, tables, direct: bool = False) -> tuple:
  """K28, wb2_quantile_score_sums: (float64 [n_outer, n_row, n_class, n_level,
  2] sums of pinball and q, int32 [n_outer, n_row, n_class, n_level, 2] counts
  of `below` and `tie`, int32 [n_outer, n_row, n_class, 2] counts of the valid
  and the invalid points) of every (row, column class, level).  `tables` are
  the HOST tables of `quantile_score_levels`; `direct`: the members are the
  quantile forecasts themselves (at most 16).  More than 16 levels become
  further launches of up to 16, each with its own read and sort of the
  members.  The operands, the HOST slab tables and `col_class` are those of
  `event_counts`; all of them and the tables are checked here: the kernel
  trusts them."""
  _require_float(ens, truth)
  direct = bool(direct)
  geo = quantile_score_geometry(ens.dtype)
  _check_members(n_member, geo, 'the quantile score sums take')
  lo, hi, t, tau, omt = _quantile_score_tables(tables, n_member, direct)
  n_level = lo.size
  per = geo['max_levels']
  if n_level > (per if direct else QUANTILE_SCORE_MAX_LEVELS):
    raise ValueError(f'{n_level} levels: the quantile score sums take 1 to '
                     f'{per if direct else QUANTILE_SCORE_MAX_LEVELS}')
  n_class = int(n_class)
  # (the classes and the LDS budget: refused here)
  quantile_score_geometry(ens.dtype, n_member, n_class, min(n_level, per),
                          direct)
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  cls = _column_classes(col_class, n_col, n_class)
  dev = ens.device
  shape = (n_outer, n_row, n_class)
  valid = torch.empty(shape + (2,), dtype=torch.int32, device=dev)
  if args is None:  # no points: nothing to add
    return (torch.zeros(shape + (n_level, QUANTILE_SCORE_TERMS),
                        dtype=torch.float64, device=dev),
            torch.zeros(shape + (n_level, 2), dtype=torch.int32, device=dev),
            valid.zero_())
  cls_dev = _upload_i32(cls.astype(np.int32), dev)
  parts = []
  for l0 in range(0, n_level, per):
    nl = min(per, n_level - l0)
    sums = torch.empty(shape + (nl, QUANTILE_SCORE_TERMS), dtype=torch.float64,
                       device=dev)
    cnt = torch.empty(shape + (nl, 2), dtype=torch.int32, device=dev)
    part = [np.ascontiguousarray(a[l0:l0 + nl]) for a in (lo, hi, t, tau, omt)]
    _launch('quantile_score_sums', 'wb2_quantile_score_sums', *args, n_member,
            member_stride, n_outer, n_row, n_col, _lib.ptr(cls_dev), n_class,
            int(direct), nl, *[a.ctypes.data for a in part], _lib.ptr(sums),
            _lib.ptr(cnt), _lib.ptr(valid), current_stream_ptr(dev))
    parts.append((sums, cnt))
  if len(parts) == 1:
    return parts[0][0], parts[0][1], valid
  return (torch.cat([s for s, _ in parts], dim=3),
          torch.cat([c for _, c in parts], dim=3), valid)


def quantile_score_fold(sums: torch.Tensor, cnt: torch.Tensor,
                        valid: torch.Tensor, class_cols, wrow, mult) -> tuple:
  """(float64 [n_outer, n_region, n_level, 2], float64 [n_outer, n_region, 2
  n_level + 2]): wb2_crps_bin_fold of the sums (n_slot = 2 n_level) -- sum_i
  wrow[r, i] * (sum_c float(mult[r, c]) * sums[o, i, c]), classes then rows in
  increasing order, plain float64 -- and wb2_event_fold of the counts (per
  level below, tie; then valid, invalid).  `wrow` (float64 [n_region, n_row])
  and `mult` (int32 [n_region, n_class]) are HOST arrays; `class_cols` is not
  needed (the kernel counts the invalid points itself) and only checked."""
  if (sums.dtype != torch.float64 or sums.dim() != 5 or
      sums.shape[4] != QUANTILE_SCORE_TERMS or not sums.is_contiguous() or
      cnt.dtype != torch.int32 or
      tuple(cnt.shape) != tuple(sums.shape[:4]) + (2,) or
      not cnt.is_contiguous() or cnt.device != sums.device or
      valid.dtype != torch.int32 or
      tuple(valid.shape) != tuple(sums.shape[:3]) + (2,) or
      not valid.is_contiguous() or valid.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [outer, row, class, '
                     'level, 2] tensor, cnt its int32 [outer, row, class, '
                     'level, 2] and valid its int32 [outer, row, class, 2]')
  n_outer, n_row, n_class, n_level, _ = (int(n) for n in sums.shape)
  wrow, mult, _ = _fold_weights(wrow, mult, n_row, n_class, class_cols)
  table = _class_fold('crps_bin_fold', sums, n_outer,
                      QUANTILE_SCORE_TERMS * n_level,
                      (n_outer, wrow.shape[0], n_level, QUANTILE_SCORE_TERMS),
                      wrow, mult)
  codes = torch.cat([cnt.reshape(n_outer, n_row, n_class, 2 * n_level), valid],
                    dim=-1)
  return table, event_fold(codes[None].contiguous(), wrow, mult)[0]


CROSS_TERMS = 4  # power_forecast, power_truth, cospectrum, quadrature


def cross_spectrum_geometry(dtype: torch.dtype, n_col: int,
                            n_member: int = 1) -> dict:
  """Extents of the K25 rows kernel for rows of `n_col` points: `supported`
  (1: the length is instantiated), the `waves_per_group` (= rows in flight per
  workgroup), the `lds_bytes` of a workgroup (the twq table and two slabs per
  wave) and `max_grid_outer`, the most workgroups of a launch (waves stride
  over the rows beyond)."""
  return _geometry('wb2_cross_spectrum_geometry',
                   (dtype_code(dtype), int(n_col), int(n_member)),
                   [('supported', _I32), ('waves_per_group', _I32),
                    ('lds_bytes', ctypes.c_int64), ('max_grid_outer', _I32)])


def _aligned_members(ens, member_stride, n_member, ens_slab, n_outer, slab):
  """(ens, member_stride, ens_slab) with every row on the 2-element boundary
  the pass-0 loads of K25 need: the operands themselves where they are, else
  the addressed slabs gathered into one contiguous [n_outer, n_member, slab]
  copy (identity addressing of that copy)."""
  if ens.data_ptr() % (2 * ens.element_size()) == 0 and member_stride % 2 == 0:
    return ens, member_stride, ens_slab
  table = _event_slabs(ens_slab, n_outer, ens, slab,
                       (max(n_member, 1) - 1) * member_stride, 'member')
  first = np.arange(n_outer, dtype=np.int64) if table is None else table
  start = (first * slab)[:, None] + np.arange(
      n_member, dtype=np.int64)[None] * member_stride
  dev = ens.device
  index = torch.as_tensor(start, device=dev)[..., None] + torch.arange(
      slab, dtype=torch.int64, device=dev)
  dense = ens.as_strided((_reach(ens),), (1,))[index]
  return dense, slab, (np.arange(n_outer, dtype=np.int64) * n_member
                       if n_member != 1 else None)


def cross_spectrum_rows(ens: torch.Tensor, member_stride: int, n_member: int,
                        ens_slab, truth: torch.Tensor, truth_slab,
                        n_outer: int, n_row: int, n_col: int, circumference
                        ) -> tuple:
  """K25, wb2_cross_spectrum_rows: (float64 [n_outer, n_row, 4, n_col // 2 +
  1] row terms -- power_forecast, power_truth, cospectrum, quadrature, the
  three forecast terms summed over the members in storage order --, int32
  [n_outer, n_row, 2] valid / invalid flags) of every row.  The operands and
  the HOST slab tables are those of `event_counts`, checked here against the
  operands' storage in the same way: the kernel trusts them.  `circumference`
  is a HOST float64 [n_row].  A row length that is not instantiated is a
  ValueError (there is no other path); operands whose rows miss the alignment
  of the kernel's loads are copied once."""
  _require_float(ens, truth)
  n_member, n_outer, n_row, n_col, member_stride = (
      int(v) for v in (n_member, n_outer, n_row, n_col, member_stride))
  geo = cross_spectrum_geometry(ens.dtype, n_col, max(1, min(n_member, 128)))
  if not geo['supported']:
    raise ValueError(f'n_col={n_col}: the cross-spectrum has no kernel for '
                     'this row length')
  if not 1 <= n_member <= 128:
    raise ValueError(f'{n_member} members: the cross-spectrum takes 1 to 128')
  circ = np.ascontiguousarray(circumference, dtype=np.float64).reshape(-1)
  if circ.size != n_row:
    raise ValueError(f'circumference must hold {n_row} values')
  if min(n_outer, n_row) >= 0 and member_stride >= 0 and n_outer * n_row:
    ens, member_stride, ens_slab = _aligned_members(
        ens, member_stride, n_member, ens_slab, n_outer, n_row * n_col)
    if truth.data_ptr() % (2 * truth.element_size()):
      truth = truth.clone()
  (n_member, member_stride, n_outer, n_row, n_col), args, _ = _member_front(
      ens, member_stride, n_member, ens_slab, truth, truth_slab, n_outer,
      n_row, n_col)
  dev = ens.device
  n_bin = n_col // 2 + 1
  sums = torch.empty((n_outer, n_row, CROSS_TERMS, n_bin),
                     dtype=torch.float64, device=dev)
  cnt = torch.empty((n_outer, n_row, 2), dtype=torch.int32, device=dev)
  if args is None:  # no rows: nothing to transform
    return sums.zero_(), cnt.zero_()
  handle, _ = _SPECTRUM_PLANS.get(args[0], n_col, 1)
  _launch('cross_spectrum_rows', 'wb2_cross_spectrum_rows', handle, *args,
          n_member, member_stride, n_outer, n_row, n_col,
          _lib.ptr(upload_f64_table(circ, dev)), _lib.ptr(sums), _lib.ptr(cnt),
          current_stream_ptr(dev))
  return sums, cnt


def cross_spectrum_fold(sums: torch.Tensor, cnt: torch.Tensor, wrow) -> tuple:
  """(float64 [n_outer, n_region, 4, n_bin], float64 [n_outer, n_region, 2]):
  wb2_crps_bin_fold of the row terms (one class of multiplicity 1, n_slot = 4
  n_bin: acc = acc + wrow[r, i] * sums[o, i] over the rows in increasing order,
  plain float64) and wb2_event_fold of the valid / invalid flags.  `wrow`
  (float64 [n_region, n_row]) is a HOST array."""
  if (sums.dtype != torch.float64 or sums.dim() != 4 or
      sums.shape[2] != CROSS_TERMS or not sums.is_contiguous() or
      cnt.dtype != torch.int32 or tuple(cnt.shape) != tuple(sums.shape[:2]) +
      (2,) or not cnt.is_contiguous() or cnt.device != sums.device):
    raise ValueError('sums must be a contiguous float64 [outer, row, 4, bin] '
                     'tensor and cnt its int32 [outer, row, 2]')
  n_outer, n_row, _, n_bin = (int(n) for n in sums.shape)
  wrow = np.ascontiguousarray(wrow, dtype=np.float64)
  ones = np.ones((wrow.shape[0] if wrow.ndim == 2 else 0, 1), dtype=np.int32)
  wrow, mult, _ = _fold_weights(wrow, ones, n_row, 1)
  table = _class_fold('cross_spectrum_fold', sums, n_outer,
                      CROSS_TERMS * n_bin,
                      (n_outer, wrow.shape[0], CROSS_TERMS, n_bin), wrow, mult)
  counts = event_fold(cnt.reshape(1, n_outer, n_row, 1, 2), wrow, mult)[0]
  return table, counts


POOL_KINDS = {'mean': 0, 'max': 1}  # WB2_POOL_MEAN, WB2_POOL_MAX


def pool_geometry(dtype: torch.dtype, n_col: int = 1, windows=(1,)) -> dict:
  """Extents of the K22 pooling kernel for a call with `windows` on rows of
  `n_col`: a workgroup owns a tile of `tile_rows` x `tile_cols` outputs of one
  field, `windows_per_launch` windows share one staging of `lds_bytes` (that
  of the call's largest window), `max_window` is the largest window whose
  halo fits the LDS at the smallest tile, `max_grid_outer` fields per grid
  row.  `windows` is a HOST sequence."""
  windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
  return _geometry('wb2_pool_geometry',
                   (dtype_code(dtype), int(n_col),
                    windows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                    windows.size),
                   [('windows_per_launch', _I32), ('tile_rows', _I32),
                    ('tile_cols', _I32), ('lds_bytes', ctypes.c_int64),
                    ('max_window', _I32), ('max_grid_outer', _I32)])


def pool_fields(x: torch.Tensor, member_stride: int, n_member: int, slabs,
                n_outer: int, n_row: int, n_col: int, windows,
                kind: str = 'mean') -> torch.Tensor:
  """K22, wb2_pool_fields: [n_window, n_outer, n_member, n_row, n_col] in the
  dtype of `x`, the `kind` ('mean' or 'max') of every point's window -- odd
  sizes in grid points, rows clipped, columns cyclic; the two fixed orders are
  stated in wb2hip.h.  Field (o, m) is the slab of `n_row * n_col` elements
  that starts `slabs[o]` slabs and `m * member_stride` ELEMENTS after the
  first element of `x` (a field without members: n_member = 1).  `slabs`
  (None = identity) and `windows` are HOST sequences; the table is checked here
  against the storage of `x` -- the kernel trusts it --, the windows by the
  entry point."""
  if kind not in POOL_KINDS:
    raise ValueError(f'kind={kind!r}: the pooling takes '
                     f'{" or ".join(map(repr, POOL_KINDS))}')
  _require_float(x)
  n_member, n_outer, n_row, n_col, member_stride = (
      int(v) for v in (n_member, n_outer, n_row, n_col, member_stride))
  if min(n_outer, n_row, n_col) < 0 or member_stride < 0:
    raise ValueError('bad sizes')
  windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
  if windows.size == 0:
    raise ValueError('no windows')
  slab = n_row * n_col
  table = _event_slabs(slabs, n_outer, x, slab,
                       (max(n_member, 1) - 1) * member_stride, 'field')
  dev = x.device
  out = torch.empty((windows.size, n_outer, max(n_member, 0), n_row, n_col),
                    dtype=x.dtype, device=dev)
  # (no points: nothing to upload or launch; the entry point still checks)
  if table is not None and out.numel():
    table = upload_table(table, dev)
  _launch('pool_fields', 'wb2_pool_fields', dtype_code(x.dtype), _lib.ptr(x),
          _lib.ptr(table if out.numel() else None), n_member, member_stride,
          n_outer, n_row, n_col,
          windows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
          windows.size, POOL_KINDS[kind], _lib.ptr(out),
          current_stream_ptr(dev))
  return out


def resampled_means_geometry(dtype: torch.dtype, wide: bool = False) -> dict:
  """Extents of the K23 kernel: `tile_points` adjacent points per workgroup,
  `replicates_per_group` replicates whose chains a thread keeps in registers,
  `steps_ahead` time steps it requests before it combines any,
  `max_grid_outer` outer indices per grid row."""
  return _geometry('wb2_resampled_means_geometry',
                   (dtype_code(dtype), int(wide)),
                   [('tile_points', _I32), ('replicates_per_group', _I32),
                    ('steps_ahead', _I32), ('max_grid_outer', _I32)])


def checked_counts(counts, n_time: int) -> np.ndarray:
  """`counts` as a HOST int64 [n_replicate, n_time], refused (ValueError) when
  it is not an integer array of that shape with entries >= 0 and row sums below
  2^31."""
  counts = np.asarray(counts)
  if counts.dtype.kind not in 'iu' or counts.ndim != 2:
    raise ValueError('counts must be an integer array [n_replicate, n_time], '
                     f'not {counts.dtype} {counts.shape}')
  if counts.shape[0] < 1 or counts.shape[1] != n_time or n_time < 1:
    raise ValueError(f'counts {counts.shape} do not match n_time={n_time} '
                     '(at least one replicate and one time)')
  if counts.dtype.kind == 'u' and counts.size and counts.max() >= 2 ** 31:
    raise ValueError('counts: a row sum reaches 2^31')
  counts = counts.astype(np.int64)
  if counts.min() < 0:
    raise ValueError('counts hold a negative entry')
  if counts.sum(axis=1).max() >= 2 ** 31:
    raise ValueError('counts: a row sum reaches 2^31')
  return counts


def resampled_means_tables(counts: np.ndarray, dtype: torch.dtype) -> tuple:
  """The two HOST tables wb2_resampled_means reads, of checked counts
  [n_replicate, n_time]: the counts widened to float64 as [n_group, n_time
  padded to a multiple of steps_ahead, replicates_per_group] (the padding is
  zero) and their row sums, float64 [n_group * replicates_per_group]."""
  geo = resampled_means_geometry(dtype)
  per, ahead = geo['replicates_per_group'], geo['steps_ahead']
  n_rep, n_time = counts.shape
  n_group = -(-n_rep // per)
  lay = np.zeros((n_group * per, -(-n_time // ahead) * ahead),
                 dtype=np.float64)
  lay[:n_rep, :n_time] = counts
  weights = np.ascontiguousarray(
      lay.reshape(n_group, per, -1).transpose(0, 2, 1))
  return torch.from_numpy(weights), torch.from_numpy(lay.sum(axis=1))


def resampled_means(x: torch.Tensor, slab, n_outer: int, n_time: int,
                    n_point: int, counts, skipna: bool = False
                    ) -> torch.Tensor:
  """K23, wb2_resampled_means: float64 [n_replicate, n_outer, n_point], the
  mean of the series x[o, :, i] with time step t taken counts[b, t] times, in
  the order stated in wb2hip.h (a step with count 0 is left out; with `skipna`
  a NaN is).  Time step t of outer index o starts `slab[o * n_time + t] *
  n_point` elements after the first element of `x`; `slab` (None = identity)
  and `counts` are HOST arrays.  Both and every size are checked here, the
  table against the storage of `x` -- the kernel trusts it --, before anything
  is uploaded or launched."""
  _require_float(x)
  n_outer, n_time, n_point = int(n_outer), int(n_time), int(n_point)
  if n_outer < 0 or n_time < 1 or n_point < 1:
    raise ValueError(f'bad sizes: n_outer={n_outer} n_time={n_time} '
                     f'n_point={n_point}')
  counts = checked_counts(counts, n_time)
  n_rep = counts.shape[0]
  table = _event_slabs(slab, n_outer * n_time, x, n_point, 0, 'time step')
  dev = x.device
  out = torch.empty((n_rep, n_outer, n_point), dtype=torch.float64, device=dev)
  if n_outer == 0:
    return out
  weights, totals = resampled_means_tables(counts, x.dtype)
  weights, totals = weights.to(dev), totals.to(dev)
  if table is not None:
    table = upload_table(table, dev)
  _launch('resampled_means', 'wb2_resampled_means', dtype_code(x.dtype),
          int(bool(skipna)), _lib.ptr(x), _lib.ptr(table), n_outer, n_time,
          n_point, _lib.ptr(weights), _lib.ptr(totals), n_rep, _lib.ptr(out),
          current_stream_ptr(dev))
  return out


def fss_sums_geometry(n_col: int, n_class: int, n_window: int) -> dict:
  """Extents of the K19 box-sum kernel: a workgroup owns `rows_per_group` rows
  of one cell at full row width, `windows_per_launch` windows share one walk,
  the running sums, the scanned row and the class sums take `lds_bytes` of
  LDS, `max_grid_outer` cells per grid row."""
  return _geometry('wb2_fss_sums_geometry',
                   (int(n_col), int(n_class), int(n_window)),
                   [('rows_per_group', _I32), ('windows_per_launch', _I32),
                    ('lds_bytes', ctypes.c_int64), ('max_grid_outer', _I32)])


def fss_sums(code: torch.Tensor, windows, n_member: int, col_class,
             n_class: int) -> torch.Tensor:
  """K19, wb2_fss_sums: int64 [n_cell, n_window, n_row, n_class, 6] of a
  contiguous uint16 code plane [..., n_row, n_col] (`event_codes`; the leading
  dims are the cells): over the valid centres of every (row, column class)
  the sums of (F - O)^2, F^2, O^2, F, O and 1, F = the window sum of k, O =
  n_member * the window sum of observed; windows are odd sizes in grid points,
  clipped in the rows and cyclic in the columns.  `windows` and `col_class`
  are HOST sequences; `col_class` is checked here, the windows by the entry
  point."""
  if code.dtype != torch.uint16 or code.dim() < 2 or not code.is_contiguous():
    raise ValueError('code must be a contiguous uint16 [..., row, column] '
                     'tensor')
  n_row, n_col = (int(n) for n in code.shape[-2:])
  n_cell = int(np.prod(code.shape[:-2], dtype=np.int64))
  windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
  n_member, n_class = int(n_member), int(n_class)
  if windows.size == 0:
    raise ValueError('no windows')
  cls = _column_classes(col_class, n_col, n_class)
  dev = code.device
  out = torch.empty((n_cell, windows.size, n_row, n_class, 6),
                    dtype=torch.int64, device=dev)
  if out.numel() == 0 or n_col == 0:
    return out.zero_()
  _launch('fss_sums', 'wb2_fss_sums', _lib.ptr(code), n_cell, n_row, n_col,
          n_member, windows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
          windows.size, _lib.ptr(_upload_i32(cls.astype(np.int32), dev)),
          n_class, _lib.ptr(out), current_stream_ptr(dev))
  return out


def fss_fold(sums: torch.Tensor, w, mult) -> torch.Tensor:
  """K19, wb2_fss_fold: float64 [n_cell, n_window, n_region, 6] = sum_i
  w[window, g(q), r, i] * float(sum_c mult[r, c] * sums[.., i, c, q]) with the
  weight group g(q) = 0 for q = 0, 1, 2, 1 for q = 3, 4 and 2 for q = 5, the
  inner sum in int64, the rows in increasing order.  `w` (float64 [n_window, 3,
  n_region, n_row]) and `mult` (int32 [n_region, n_class]) are HOST arrays."""
  if sums.dtype != torch.int64 or sums.dim() != 5 or sums.shape[-1] != 6 or (
      not sums.is_contiguous()):
    raise ValueError('sums must be a contiguous int64 [cell, window, row, '
                     'class, 6] tensor')
  n_cell, n_window, n_row, n_class = (int(n) for n in sums.shape[:4])
  w = np.ascontiguousarray(w, dtype=np.float64)
  mult = np.ascontiguousarray(mult, dtype=np.int32)
  n_region = mult.shape[0] if mult.ndim == 2 else -1
  if w.shape != (n_window, 3, n_region, n_row) or mult.shape != (
      n_region, n_class):
    raise ValueError('w must be [n_window, 3, n_region, n_row] and mult '
                     '[n_region, n_class]')
  dev = sums.device
  out = torch.empty((n_cell, n_window, n_region, 6), dtype=torch.float64,
                    device=dev)
  if out.numel() == 0:
    return out
  _launch('fss_fold', 'wb2_fss_fold', _lib.ptr(sums), n_cell, n_window, n_row,
          n_class, _lib.ptr(upload_f64_table(w, dev) if w.size else None),
          _lib.ptr(_upload_i32(mult.reshape(-1), dev)), n_region,
          _lib.ptr(out), current_stream_ptr(dev))
  return out


def ensemble_threshold_reduce(plan: ReductionPlan, ens: torch.Tensor,
                              member_stride: int, n_member: int, ens_slab,
                              truth: torch.Tensor, truth_slab,
                              thr: torch.Tensor, thr_slab, n_outer: int,
                              skipna: bool, want_sums: bool = False):
  """Exceedance-count kernel + region fold: metrics[4, n_region, n_outer] =
  (Brier, debiased Brier, ignorance, RPS part).  With `want_sums`: (metrics,
  the raw region sums [n_outer, n_region, K])."""
  lib = _lib.load()
  _require_float(ens, truth, thr)
  _check_contiguous(plan.device, 'the plan device', ens, truth, thr)
  mode = _lib.MODE_ENS_THR
  prep = PreparedLaunch(plan, lib.wb2_ens_tile_cols(plan.n_col),
                        lib.wb2_num_slots(mode, int(skipna)), n_outer,
                        plan.wfield)
  stream = current_stream_ptr(plan.device)
  _lib.check(lib.wb2_ens_threshold_partials(
      _DTYPES[ens.dtype], int(skipna), _lib.ptr(ens), _lib.ptr(ens_slab),
      _lib.ptr(truth), _lib.ptr(truth_slab), _lib.ptr(thr), _lib.ptr(thr_slab),
      n_member, member_stride, n_outer, *prep.ens_args(),
      _lib.ptr(prep.partials), stream), 'wb2_ens_threshold_partials')
  metrics, sums = prep.fold('wb2_det_combine', (mode, int(skipna)),
                            _lib.GENERIC_KQ[mode], want_sums, stream)
  return (metrics, sums) if want_sums else metrics


RANK_MEAN_MAX_BINS = 256  # wb2_rank_histogram_mean: 64 x n_bins counts in LDS


def rank_histogram(ens: torch.Tensor, member_stride: int, n_member: int,
                   ens_slab, truth: torch.Tensor, truth_slab, n_outer: int,
                   n_point: int, n_bins: int, break_ties: bool, seed: int,
                   acc_row=None, n_acc: int = 0, numpy_stream=None,
                   mean_over=None) -> torch.Tensor:
  """wb2_rank_histogram: one-hot [n_outer, n_point, n_bins] (float64), or with
  `acc_row` the per-row counts [n_acc, n_point, n_bins], or with `mean_over` =
  (n_lead, n_time, n_tail), n_outer = their product: the MEAN of the one-hots
  over the middle axis [n_lead * n_tail, n_point, n_bins]
  (wb2_rank_histogram_mean: no one-hots, no atomics).

  `numpy_stream` = (pcg_state, pcg_inc, ref_outer_off[n_outer] int64 device
  tensor, (row, col, member) strides, n_col) switches to
  wb2_rank_histogram_seeded: ties are broken with the very perturbations
  np.random.default_rng(seed).uniform hands the reference."""
  lib = _lib.load()
  dev = ens.device
  _require_float(ens, truth)
  _check_contiguous(dev, 'one device', ens, truth)
  if mean_over is not None:
    n_lead, n_time, n_tail = (int(v) for v in mean_over)
    if n_lead * n_time * n_tail != n_outer or n_time < 1:
      raise ValueError(f'mean_over={mean_over} does not factor {n_outer}')
  pcg = st = ref_off = None
  n_col = 1
  if numpy_stream is not None and break_ties:
    state, inc, ref_off, strides, n_col = numpy_stream
    mask = (1 << 64) - 1
    pcg = (ctypes.c_uint64 * 4)(state >> 64, state & mask, inc >> 64, inc & mask)
    st = (ctypes.c_int64 * 3)(*[int(v) for v in strides])
    if ref_off.dtype != torch.int64 or ref_off.numel() != n_outer:
      raise ValueError('ref_outer_off must be int64[n_outer]')
  if mean_over is not None:
    out = torch.empty((n_lead * n_tail, n_point, n_bins), dtype=torch.float64,
                      device=dev)
    _lib.check(lib.wb2_rank_histogram_mean(
        _DTYPES[ens.dtype], _lib.ptr(ens), _lib.ptr(ens_slab), _lib.ptr(truth),
        _lib.ptr(truth_slab), n_member, member_stride, n_lead, n_time, n_tail,
        n_point, int(n_col), n_bins, int(break_ties),
        seed & 0xFFFFFFFFFFFFFFFF, pcg, _lib.ptr(ref_off), st, 1,
        _lib.ptr(out), current_stream_ptr(dev)), 'wb2_rank_histogram_mean')
    return out
  if acc_row is None:
    out = torch.empty((n_outer, n_point, n_bins), dtype=torch.float64,
                      device=dev)
  else:
    out = torch.zeros((n_acc, n_point, n_bins), dtype=torch.float64,
                      device=dev)
  if pcg is not None:
    _lib.check(lib.wb2_rank_histogram_seeded(
        _DTYPES[ens.dtype], _lib.ptr(ens), _lib.ptr(ens_slab), _lib.ptr(truth),
        _lib.ptr(truth_slab), n_member, member_stride, n_outer, n_point,
        int(n_col), n_bins, pcg, _lib.ptr(ref_off), st, _lib.ptr(acc_row),
        _lib.ptr(out), current_stream_ptr(dev)), 'wb2_rank_histogram_seeded')
    return out
  _lib.check(lib.wb2_rank_histogram(
      _DTYPES[ens.dtype], _lib.ptr(ens), _lib.ptr(ens_slab), _lib.ptr(truth),
      _lib.ptr(truth_slab), n_member, member_stride, n_outer, n_point, n_bins,
      int(break_ties), seed & 0xFFFFFFFFFFFFFFFF, _lib.ptr(acc_row),
      _lib.ptr(out), current_stream_ptr(dev)), 'wb2_rank_histogram')
  return out


def ensemble_threshold_maps(ens: torch.Tensor, member_stride: int,
                            n_member: int, ens_slab, truth: torch.Tensor,
                            truth_slab, thr: torch.Tensor, thr_slab,
                            n_outer: int, n_point: int,
                            skipna: bool) -> torch.Tensor:
  """wb2_ens_threshold_maps: [4, n_outer, n_point] float64 (Brier, debiased
  Brier, ignorance, RPS part), unreduced."""
  lib = _lib.load()
  dev = ens.device
  _require_float(ens, truth, thr)
  _check_contiguous(dev, 'one device', ens, truth, thr)
  maps = torch.empty((4, n_outer, n_point), dtype=torch.float64, device=dev)
  _lib.check(lib.wb2_ens_threshold_maps(
      _DTYPES[ens.dtype], int(skipna), _lib.ptr(ens), _lib.ptr(ens_slab),
      _lib.ptr(truth), _lib.ptr(truth_slab), _lib.ptr(thr), _lib.ptr(thr_slab),
      n_member, member_stride, n_outer, n_point, _lib.ptr(maps),
      current_stream_ptr(dev)), 'wb2_ens_threshold_maps')
  return maps


def seeps_map(inputs: t.Sequence[torch.Tensor],
              slabs: t.Sequence[t.Optional[torch.Tensor]], n_outer: int,
              n_point: int, aux: torch.Tensor, scalar: float) -> torch.Tensor:
  """wb2_seeps_map: [n_outer, n_point] float64 per-point SEEPS."""
  lib = _lib.load()
  dev = inputs[0].device
  dtype = inputs[0].dtype
  dtype_code(dtype)  # (TypeError: not one of the kernels' dtypes)
  if any(x.dtype != dtype for x in inputs):
    raise ValueError('inputs must share dtype/device and be contiguous')
  _check_contiguous(dev, 'one device', *inputs)
  if aux.dtype != torch.float64 or aux.numel() != n_point:
    raise ValueError('aux must be float64[n_point]')
  out = torch.empty((n_outer, n_point), dtype=torch.float64, device=dev)
  _lib.check(lib.wb2_seeps_map(
      _DTYPES[dtype], _lib.ptr_array(inputs), _lib.ptr_array(slabs), n_outer,
      n_point, _lib.ptr(aux), float(scalar), _lib.ptr(out),
      current_stream_ptr(dev)), 'wb2_seeps_map')
  return out


def axis_moments(x: torch.Tensor, n_lead: int, n_red: int, n_tail: int,
                 w_red: t.Optional[torch.Tensor], skipna: bool,
                 want_sq: bool = False, w_repeat: int = 1,
                 n_split: t.Optional[int] = None):
  """wb2_axis_moments on a contiguous [n_lead, n_red, n_tail] view of `x`:
  (sum, sumsq or None, count) as float64 tensors of n_lead * n_tail.  `w_red`
  holds n_red / w_repeat weights, each shared by w_repeat consecutive r.
  `n_split` slices of the reduced axis (None: wb2_axis_moments_splits)."""
  lib = _lib.load()
  dev = x.device
  if x.dtype not in _DTYPES or not x.is_contiguous():
    raise ValueError('x must be a contiguous float32/float64 device tensor')
  if x.numel() != n_lead * n_red * n_tail:
    raise ValueError('shape mismatch')
  if w_red is not None and (w_red.dtype != torch.float64
                            or w_red.numel() * w_repeat != n_red):
    raise ValueError('w_red must be float64[n_red / w_repeat]')
  n_out = n_lead * n_tail
  if n_split is None:
    n_split = lib.wb2_axis_moments_splits(n_lead, n_red, n_tail,
                                          w_repeat if w_red is not None else 1)
  work = torch.empty((3 * n_split * max(n_out, 1),), dtype=torch.float64,
                     device=dev)
  total = torch.empty((n_out,), dtype=torch.float64, device=dev)
  count = torch.empty_like(total)
  sq = torch.empty_like(total) if want_sq else None
  _lib.check(lib.wb2_axis_moments(
      _DTYPES[x.dtype], _lib.ptr(x), n_lead, n_red, n_tail, _lib.ptr(w_red),
      w_repeat, int(skipna), n_split, _lib.ptr(work), _lib.ptr(total),
      _lib.ptr(sq), _lib.ptr(count), current_stream_ptr(dev)),
             'wb2_axis_moments')
  return total, sq, count


# ---------------------------------------------------------------------------
# The path's one exchange step through the C ABI (RCCL directly, no
# torch.distributed): for callers that bring their own rendezvous.
# ---------------------------------------------------------------------------
def comm_unique_id() -> bytes:
  """128-byte RCCL id made by rank 0, to be handed to every rank."""
  buf = ctypes.create_string_buffer(128)
  _lib.check(_lib.load().wb2_comm_unique_id(buf), 'wb2_comm_unique_id')
  return buf.raw


def comm_init_rank(unique_id: bytes, n_ranks: int, rank: int):
  """ncclComm_t (opaque handle) of this rank on the current device."""
  if len(unique_id) != 128:
    raise ValueError('unique_id must be the 128 bytes of comm_unique_id()')
  handle = ctypes.c_void_p()
  _lib.check(_lib.load().wb2_comm_init_rank(
      ctypes.create_string_buffer(unique_id, 128), n_ranks, rank,
      ctypes.byref(handle)), 'wb2_comm_init_rank')
  return handle


def comm_destroy(comm) -> None:
  _lib.check(_lib.load().wb2_comm_destroy(comm), 'wb2_comm_destroy')


def time_mean_allreduce(total: torch.Tensor, count: torch.Tensor, comm) -> None:
  """In-place sum of the (sum, count) accumulators over the ranks of `comm`
  (xbeam.Mean's combiner across init-time shards, evaluation.py:735-744), one
  grouped RCCL operation on the current stream."""
  for x in (total, count):
    if x.dtype != torch.float64 or not x.is_contiguous() or not x.is_cuda:
      raise ValueError('accumulators must be contiguous float64 device tensors')
  if total.numel() != count.numel():
    raise ValueError('sum / count size mismatch')
  _lib.check(_lib.load().wb2_time_mean_allreduce(
      _lib.ptr(total), _lib.ptr(count), total.numel(), comm,
      current_stream_ptr(total.device)), 'wb2_time_mean_allreduce')
