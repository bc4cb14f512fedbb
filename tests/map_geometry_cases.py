"""The geometry sweep of the map kernels and the running means: K5
(spatial_maps_kernel, spatial_accumulate_kernel, spatial_accumulate_addr_kernel
of spatial_maps.hip) and seeps_map_kernel, time_accumulate_kernel and
gather_accumulate_kernel of stream_reduce.hip.

One case list for test_map_geometry_gpu.py, which runs it against plain
references (NumPy in the input dtype for the maps, a float64 loop in time
order for the sums), and test_map_geometry_cpu.py, which asserts on the CPU
that the list reaches every instantiation, vector and block edge, grid split,
U-loop remainder and slab-group remainder it is meant to reach.

The geometry is read from the sources, so the cases cannot drift from it: the
vector widths of pick_vec and of the by-address dispatch, the 256-thread
blocks, the 32768 split of the grid's y dimension (grid_for, seeps_map_impl),
the U = 4 time steps of the accumulate loops and kSeepsMapSlabs.
"""
import dataclasses
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     'weatherbench2_amd', 'csrc')
SPATIAL_SRC = os.path.join(_CSRC, 'spatial_maps.hip')
STREAM_SRC = os.path.join(_CSRC, 'stream_reduce.hip')


def _read(path):
  with open(path) as f:
    return f.read()


def _source_constants():
  sp, st = _read(SPATIAL_SRC), _read(STREAM_SRC)
  # `const int w = dtype == WB2_F32 ? 4 : 2;` in pick_vec and in
  # wb2_spatial_accumulate_addr
  widths = set(re.findall(r'const int w = dtype == WB2_F32 \? (\d+) : (\d+);',
                          sp))
  assert len(widths) == 1, widths
  (w32, w64), = widths
  block = set(re.findall(r'__launch_bounds__\((\d+)\)', sp))
  assert len(block) == 1, block
  split = set(re.findall(r'n_y < (\d+) \? n_y : (\d+)', sp))
  assert len(split) == 1 and len(set(*split)) == 1, split
  seeps_split = set(re.findall(r'n_group < (\d+) \? n_group : (\d+)', st))
  assert len(seeps_split) == 1 and len(set(*seeps_split)) == 1, seeps_split
  u = set(re.findall(r'constexpr int U = (\d+);', sp))
  assert len(u) == 1, u
  u_time = re.search(r'for \(; t \+ (\d+) <= n_time; t \+= (\d+)\)', st)
  assert u_time.group(1) == u_time.group(2)
  slabs = int(re.search(r'constexpr int kSeepsMapSlabs = (\d+);', st).group(1))
  return dict(w={'float32': int(w32), 'float64': int(w64)},
              block=int(block.pop()), y_split=int(split.pop()[0]),
              seeps_y_split=int(seeps_split.pop()[0]), u=int(u.pop()),
              u_time=int(u_time.group(1)), seeps_slabs=slabs)


_C = _source_constants()
W = _C['w']                    # elements per 16-byte vector
BLOCK = _C['block']            # threads per workgroup of every kernel here
Y_SPLIT = _C['y_split']        # grid_for: n_y beyond it goes to grid.z
SEEPS_Y_SPLIT = _C['seeps_y_split']  # seeps_map_impl: groups beyond it -> z
U = _C['u']                    # time steps per unrolled group (K5)
U_TIME = _C['u_time']          # the same in time_accumulate_kernel
SEEPS_SLABS = _C['seeps_slabs']  # outer slabs per seeps_map_kernel thread
DTYPES = ('float32', 'float64')
ESIZE = {'float32': 4, 'float64': 8}
OUTS = ('bias', 'mse', 'mae')
N_TIMES = tuple(range(1, 10)) + (13,)


@dataclasses.dataclass(frozen=True)
class Case:
  kind: str             # maps | acc | addr | seeps | time | gather
  dtype: str = 'float64'
  skipna: bool = False
  n_point: int = 1      # maps, acc, addr, seeps
  n_outer: int = 1      # maps / seeps: slabs; acc: n_rest; addr: n_dst;
                        # time: n_lead; gather: n_out
  n_time: int = 1       # acc, addr, time, gather
  n_tail: int = 1       # time
  outs: str = 'bms'     # maps: outputs written; addr: sums wanted
                        # (b = bias, m = mse, s = mae)
  misalign: str = ''    # maps / acc: '' | 'f' | 't' | 'bias' | 'mse' | 'mae'
                        # (that base one element off 16 bytes)
  tables: str = ''      # maps / acc: '' (identity) | 'perm' (permuted and
                        # repeated forecast slabs) | 'bcast' (one truth slab
                        # per rest index, broadcast over time); seeps: '' |
                        # 'wet' (wet thresholds by valid time)
  aligned16: str = ''   # addr: 'yes' | 'off' (slabs one element off, flag 0) |
                        # 'ragged' (flag 1, n_point % w != 0)
  sum_off: bool = False  # addr: sums 8- but not 16-byte aligned
  entry: str = ''       # seeps: 'in' | 'addr'; time: 'plain' | 'scatter' |
                        # 'runs'; gather: 'plain' | 'rows'
  run: int = 1          # time 'runs'
  nan: bool = False     # NaNs in the inputs (which kinds: the data builders)

  @property
  def w(self):
    return W[self.dtype]

  @property
  def vec(self):
    """The instantiation's VEC that the dispatch picks (1 for kernels without
    one): pick_vec for maps / acc (n_point % w, the forecast and truth bases,
    and for maps every output present), the caller's aligned16 for addr."""
    if self.kind == 'maps':
      ok = self.n_point % self.w == 0 and self.misalign == ''
      return self.w if ok else 1
    if self.kind == 'acc':
      ok = self.n_point % self.w == 0 and self.misalign not in ('f', 't')
      return self.w if ok else 1
    if self.kind == 'addr':
      ok = self.aligned16 == 'yes' and self.n_point % self.w == 0
      return self.w if ok else 1
    return 1

  @property
  def instantiation(self):
    """(kernel, dtype, VEC, SKIPNA) as the dispatch launches it; the entry
    point stands in for VEC where the kernel has none."""
    kernel = {'maps': 'spatial_maps_kernel',
              'acc': 'spatial_accumulate_kernel',
              'addr': 'spatial_accumulate_addr_kernel',
              'seeps': 'seeps_map_kernel', 'time': 'time_accumulate_kernel',
              'gather': 'gather_accumulate_kernel'}[self.kind]
    if self.kind in ('maps', 'acc', 'addr'):
      return kernel, self.dtype, self.vec, (self.skipna if self.kind != 'maps'
                                            else None)
    return kernel, self.dtype, self.entry, (self.skipna if self.kind != 'seeps'
                                            else None)

  @property
  def threads(self):
    """Threads along grid.x (one per vector of points, or per element)."""
    if self.kind in ('maps', 'acc', 'addr'):
      return self.n_point // self.vec
    if self.kind == 'seeps':
      return self.n_point
    if self.kind == 'time':
      return self.n_outer * self.n_tail
    return self.n_outer

  @property
  def grid_z(self):
    if self.kind in ('maps', 'acc', 'addr'):
      gy = min(self.n_outer, Y_SPLIT)
      return -(-self.n_outer // gy)
    if self.kind == 'seeps':
      groups = -(-self.n_outer // SEEPS_SLABS)
      return -(-groups // min(groups, SEEPS_Y_SPLIT))
    return 1

  @property
  def accumulates(self):
    return self.kind in ('acc', 'addr', 'time', 'gather')

  @property
  def id(self):
    s = f'{self.kind}-{self.dtype}'
    if self.kind in ('acc', 'addr', 'time', 'gather'):
      s += '-skipna' if self.skipna else '-strict'
    if self.entry:
      s += f'-{self.entry}'
    if self.kind != 'gather' and self.kind != 'time':
      s += f'-p{self.n_point}'
    s += f'-o{self.n_outer}'
    if self.accumulates:
      s += f'-t{self.n_time}'
    if self.kind == 'time':
      s += f'-tail{self.n_tail}' + (f'-run{self.run}' if self.run > 1 else '')
    if self.kind in ('maps', 'addr') and self.outs != 'bms':
      s += f'-{self.outs}'
    if self.misalign:
      s += f'-off_{self.misalign}'
    if self.tables:
      s += f'-{self.tables}'
    if self.aligned16:
      s += f'-a16_{self.aligned16}'
    if self.sum_off:
      s += '-sum8'
    return s + ('-nan' if self.nan else '')


def point_edges(w):
  """1, w - 1, w, w + 1, both sides of one block of vector threads and of
  scalar threads, and several blocks, the last one ragged."""
  b = BLOCK * w
  return sorted({1, max(w - 1, 1), w, w + 1, BLOCK - 1, BLOCK + 1, b - 1, b,
                 b + 1, b + w, 5 * b + 3 * w, 5 * b + 3})


# every non-empty subset of the three outputs
SUBSETS = ('b', 'm', 's', 'bm', 'bs', 'ms', 'bms')
Y_EDGES = (Y_SPLIT - 1, Y_SPLIT, Y_SPLIT + 1, 2 * Y_SPLIT + 1)


def _maps():
  out = []
  tabs = ('', 'perm', 'bcast')
  for dtype in DTYPES:
    w = W[dtype]
    for i, n in enumerate(point_edges(w)):
      out.append(Case('maps', dtype, n_point=n, n_outer=3,
                      tables=tabs[i % 3], nan=i % 2 == 0))
    # the vector path turned off by one reason alone (n_point % w: above)
    for reason in ('f', 't') + OUTS:
      out.append(Case('maps', dtype, n_point=BLOCK * w + w, n_outer=2,
                      misalign=reason))
    # vector and scalar in turn; the scalar cases also meet the subsets
    # of the misaligned outputs above
    for i, sub in enumerate(SUBSETS):
      n = BLOCK * w + (w if i % 2 else 1)
      out.append(Case('maps', dtype, n_point=n, n_outer=3, outs=sub,
                      tables=tabs[i % 3]))
    # grid.z: tiny slabs, vector and scalar
    for i, n_outer in enumerate(Y_EDGES):
      for n in (w, 1):
        out.append(Case('maps', dtype, n_point=n, n_outer=n_outer,
                        tables=tabs[i % 3]))
  return out


def _acc():
  out = []
  tabs = ('', 'perm', 'bcast')
  for dtype in DTYPES:
    w = W[dtype]
    for skipna in (False, True):
      for i, nt in enumerate(N_TIMES):
        # every U-loop remainder, vector and scalar
        out.append(Case('acc', dtype, skipna, n_point=BLOCK * w + w,
                        n_outer=2, n_time=nt, tables=tabs[i % 3],
                        nan=skipna or i % 3 == 0))
        if nt <= 2 * U - 1:
          out.append(Case('acc', dtype, skipna, n_point=BLOCK * w + 1,
                          n_outer=1, n_time=nt, tables=tabs[(i + 1) % 3],
                          nan=True))
      for i, n in enumerate(point_edges(w)):
        out.append(Case('acc', dtype, skipna, n_point=n, n_outer=3,
                        n_time=5 + i % 4, tables=tabs[i % 3], nan=True))
      for reason in ('f', 't'):
        out.append(Case('acc', dtype, skipna, n_point=BLOCK * w + w,
                        n_outer=2, n_time=6, misalign=reason, nan=True))
      for i, n_rest in enumerate((Y_SPLIT, Y_SPLIT + 1)):
        for n in (w, 1):
          out.append(Case('acc', dtype, skipna, n_point=n, n_outer=n_rest,
                          n_time=5, tables=tabs[(i + n) % 3], nan=True))
  return out


def _addr():
  out = []
  modes = ('yes', 'off', 'ragged')
  subsets = ('bms', 'sb', 'm', 'bs', 'ms')
  for dtype in DTYPES:
    w = W[dtype]
    for skipna in (False, True):
      for i, nt in enumerate(N_TIMES):
        mode = modes[i % 3]
        n = BLOCK * w + (1 if mode == 'ragged' else w)
        out.append(Case('addr', dtype, skipna, n_point=n, n_outer=3,
                        n_time=nt, aligned16=mode, outs=subsets[i % 5],
                        sum_off=i % 2 == 1, nan=True))
      for i, n in enumerate(point_edges(w)):
        if i % 2 != skipna:
          continue  # each point count once per dtype
        mode = 'yes' if n % w == 0 else 'ragged'
        out.append(Case('addr', dtype, skipna, n_point=n, n_outer=2,
                        n_time=5 + i % 4, aligned16=mode, sum_off=i % 3 == 0,
                        nan=True))
      out.append(Case('addr', dtype, skipna, n_point=BLOCK * w + w,
                      n_outer=2, n_time=6, aligned16='off', nan=True))
      for i, n_dst in enumerate((1, Y_SPLIT, Y_SPLIT + 1)):
        for n in (w, w + 1):
          out.append(Case('addr', dtype, skipna, n_point=n, n_outer=n_dst,
                          n_time=6, aligned16='yes' if n == w else 'ragged',
                          outs=subsets[(i + n) % 5], nan=True))
  return out


SEEPS_OUTER = tuple(range(1, 10)) + (15, 16, 17)
SEEPS_POINTS = (1, BLOCK - 1, BLOCK, BLOCK + 1)


def _seeps():
  out = []
  for dtype in DTYPES:
    for entry in ('in', 'addr'):
      for i, n_outer in enumerate(SEEPS_OUTER):
        out.append(Case('seeps', dtype, n_point=SEEPS_POINTS[i % 4],
                        n_outer=n_outer, entry=entry,
                        tables='wet' if i % 2 else '', nan=True))
      # grid.z: both sides of SEEPS_Y_SPLIT groups, one point per slab
      for n_outer in (SEEPS_SLABS * SEEPS_Y_SPLIT,
                      SEEPS_SLABS * SEEPS_Y_SPLIT + 1):
        out.append(Case('seeps', dtype, n_point=1, n_outer=n_outer,
                        entry=entry, tables='wet', nan=True))
  return out


# n_lead * n_tail on both sides of one and two 256-thread blocks
TIME_SHAPES = ((3, 85), (1, 256), (257, 1), (7, 73), (2, 256), (3, 171),
               (9, 29), (5, 51), (1, 255))


def _runs_of(n):
  """A run length > 1 that divides n (n itself when n is prime)."""
  for r in (7, 5, 4, 3, 2):
    if n % r == 0 and r < n:
      return r
  return n


def _time():
  out = []
  for dtype in DTYPES:
    for skipna in (False, True):
      for entry in ('plain', 'scatter', 'runs'):
        if entry == 'plain' and dtype == 'float32':
          continue  # wb2_time_accumulate takes float64 values only
        for i, nt in enumerate(range(1, 10)):
          n_lead, n_tail = TIME_SHAPES[(i + len(entry)) % len(TIME_SHAPES)]
          run = _runs_of(n_lead * n_tail) if entry == 'runs' else 1
          if entry == 'runs' and run == 1:
            n_lead, n_tail = 2, 256
            run = _runs_of(512)
          out.append(Case('time', dtype, skipna, n_outer=n_lead, n_time=nt,
                          n_tail=n_tail, entry=entry, run=run, nan=True))
  return out


GATHER_OUT = (7, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)


def _gather():
  out = []
  for entry in ('plain', 'rows'):
    for skipna in (False, True):
      for i, nt in enumerate(range(1, 10)):
        out.append(Case('gather', 'float64', skipna,
                        n_outer=GATHER_OUT[i % len(GATHER_OUT)], n_time=nt,
                        entry=entry, nan=True))
  return out


def _cases():
  out, seen = [], set()
  for c in _maps() + _acc() + _addr() + _seeps() + _time() + _gather():
    if c.id not in seen:
      seen.add(c.id)
      out.append(c)
  return out


CASES = _cases()
