"""The geometry sweep of the rank histogram (K6, rank_histogram.hip): its three
kernel forms (one-hot, atomic counts, the LDS mean kernel with its sums
branch), the member loads in groups of 16, 4 and 1, the one-hot store loop of a
wave against the bin count, the 32768 split of the grid, slab tables and
strides, the seeded NumPy stream's layouts and jumps, and the data that makes
ties, NaNs, infinities and tiny gaps.

One case list for test_rank_geometry_gpu.py, which runs it against the plain
references of tests/rank_np.py, and test_rank_geometry_cpu.py, which asserts on
the CPU that the list reaches every edge it is meant to reach.  The geometry is
read from the sources, so the cases cannot drift from it.  The builders below
(data, buffers and tables, stream indices) are NumPy only.
"""
import dataclasses
import os
import re
import types
import zlib

import numpy as np

_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    'weatherbench2_amd')
RANK_SRC = os.path.join(_PKG, 'csrc', 'rank_histogram.hip')
COMMON_SRC = os.path.join(_PKG, 'csrc', 'common.hpp')
ENGINE_SRC = os.path.join(_PKG, 'engine.py')


def _read(path):
  with open(path) as f:
    return f.read()


def _once(pattern, text):
  found = re.findall(pattern, text)
  assert len(found) == 1, (pattern, found)
  return found[0]


def _source_constants():
  src = _read(RANK_SRC)
  g16 = _once(r'for \(; m \+ (16) <= M; m \+= (\d+)\)', src)
  g4 = _once(r'for \(; m \+ (4) <= M; m \+= (\d+)\)', src)
  groups = re.findall(r'for \(; m \+ (\d+) <= M; m \+= (\d+)\)', src)
  assert groups == [g16, g4] and all(a == b for a, b in groups), groups
  _once(r'for \(; m < M; \+\+m\)', src)
  block = _once(r'__launch_bounds__\((\d+)\) rank_histogram_kernel', src)
  assert _once(r'\(n_point \+ (\d+)\) / ' + block + r'\), \(unsigned\)gy',
               src) == str(int(block) - 1)
  launches = re.findall(r'rank_histogram_kernel<\w+>, grid, dim3\((\d+)\)', src)
  assert launches == [block, block], launches
  wave = _once(r'constexpr int kWave = (\d+);', _read(COMMON_SRC))
  _once(r'__launch_bounds__\(kWave\)\s+rank_histogram_mean_kernel', src)
  split = _once(r'n_outer < (\d+) \? n_outer : (\d+);', src)
  row_split = _once(r'n_row < (\d+) \? n_row : (\d+);', src)
  assert split[0] == split[1] and row_split[0] == row_split[1]
  max_bins = _once(r'(?m)^RANK_MEAN_MAX_BINS = (\d+)\b', _read(ENGINE_SRC))
  return dict(groups=tuple(int(a) for a, _ in groups), block=int(block),
              wave=int(wave), split=int(split[0]), row_split=int(row_split[0]),
              max_bins=int(max_bins))


_C = _source_constants()
GROUPS = _C['groups']        # member loads in flight: (16, 4), then one by one
BLOCK = _C['block']          # threads per workgroup of rank_histogram_kernel
WAVE = _C['wave']            # lanes; the mean kernel's workgroup is one wave
SPLIT = _C['split']          # n_outer beyond it goes to grid.z
ROW_SPLIT = _C['row_split']  # the same for the mean kernel's result rows
MAX_BINS = _C['max_bins']    # bins the mean kernel's LDS counts hold
DTYPES = ('float32', 'float64')
FORMS = ('onehot', 'counts', 'mean', 'sum')
TIES = ('none', 'first', 'hash', 'numpy')
SLABS = ('identity', 'padded', 'member_inner', 'permuted', 'shared_truth')
BASES = {'base_2_32_5': 2**32 + 5, 'base_2_40_1': 2**40 + 1,
         'base_2_62': 2**62}
STREAMS = ('member1', 'strided', 'rowmajor', 'transposed',
           'nonmonotonic') + tuple(BASES)
RECIPES = ('plain', 'quantised', 'specials', 'all_equal', 'one_ulp',
           'subnormal_gap')
PAD = 7      # `padded`: elements between one member's slabs and the next's
SHARE = 3    # `shared_truth`: outer indices per truth slab
TINY = float(np.nextafter(np.float32(0), np.float32(1)))  # 2**-149

MEMBERS = (1, 2, 3, 4, 5, 15, 16, 17, 19, 20, 21, 31, 32, 33, 35, 36, 50, 255)
WAVE_BINS = (1, 2, 3, 5, 7, 21, 32, 33, 51, 64, 65, 100, 127, 128, 256)
POINTS = (1, 2, 63, 64, 65, 127, 129, 255, 256, 257, WAVE * 5 + 1)
MEAN_SHAPES = tuple((a, b, c) for a in (1, 2) for b in (1, 2, 5)
                    for c in (1, 3))


@dataclasses.dataclass(frozen=True)
class Case:
  group: str            # the axis the case belongs to (one GPU test each)
  form: str             # onehot | counts | mean | sum
  ties: str             # none (untied data) | first (break_ties = 0) | hash |
                        # numpy (the seeded stream)
  dtype: str
  n_member: int
  n_bins: int
  n_outer: int = 1      # onehot, counts (mean, sum: the product of `shape`)
  shape: tuple = None   # mean, sum: (n_lead, n_time, n_tail)
  n_point: int = 1
  n_col: int = 0        # numpy ties: columns of the point grid (0: n_point)
  slab: str = 'identity'
  stream: str = 'strided'
  recipe: str = 'plain'
  seed: int = 5

  def __post_init__(self):
    assert self.form in FORMS and self.ties in TIES and self.slab in SLABS
    assert self.stream in STREAMS and self.recipe in RECIPES
    assert (self.n_member + 1) % self.n_bins == 0
    if self.form in ('mean', 'sum'):
      object.__setattr__(self, 'n_outer', int(np.prod(self.shape)))
    else:
      assert self.shape is None
    if not self.n_col:
      object.__setattr__(self, 'n_col', self.n_point)
    assert self.n_point % self.n_col == 0

  @property
  def n_sample(self):
    return self.n_outer * self.n_point

  @property
  def groups16(self):
    return self.n_member // GROUPS[0]

  @property
  def groups4(self):
    return self.n_member % GROUPS[0] // GROUPS[1]

  @property
  def tail(self):
    return self.n_member % GROUPS[1]

  @property
  def bin_class(self):
    b = self.n_bins
    if b == 1:
      return '1'
    if b < WAVE:
      return 'divides' if WAVE % b == 0 else 'below'
    if b == WAVE:
      return 'wave'
    return 'above' if b < 2 * WAVE else 'many'

  @property
  def last_wave(self):
    """Points the last wave of a slab holds."""
    return (self.n_point - 1) % WAVE + 1

  @property
  def waves_per_block(self):
    return min(-(-self.n_point // WAVE), BLOCK // WAVE)

  @property
  def grid_z(self):
    if self.form in ('mean', 'sum'):
      rows = self.shape[0] * self.shape[2]
      return -(-rows // min(rows, ROW_SPLIT))
    return -(-self.n_outer // min(self.n_outer, SPLIT))

  @property
  def n_acc(self):
    """Result rows: counts sum every second outer index into one row and leave
    one more row that no acc_row names."""
    if self.form == 'counts':
      return -(-self.n_outer // 2) + 1
    if self.form in ('mean', 'sum'):
      return self.shape[0] * self.shape[2]
    return self.n_outer

  @property
  def id(self):
    s = f'{self.form}-{self.ties}-{self.dtype}-m{self.n_member}-b{self.n_bins}'
    s += (f'-o{self.n_outer}' if self.shape is None
          else '-t' + 'x'.join(str(n) for n in self.shape))
    s += f'-p{self.n_point}'
    if self.ties == 'numpy':
      s += f'-{self.stream}-c{self.n_col}-s{self.seed}'
    elif self.ties == 'hash':
      s += f'-s{self.seed}'
    if self.slab != 'identity':
      s += f'-{self.slab}'
    return f'{s}-{self.recipe}'


def bins_for(n_member):
  """1, M + 1 and the middle proper divisor of M + 1 where there is one."""
  n = n_member + 1
  proper = [d for d in range(2, n) if n % d == 0]
  out = [1, n] + ([proper[len(proper) // 2]] if proper else [])
  return sorted(set(out))


def _smallest_divisor(n):
  """The smallest divisor of n above 1 and below n (1 for a prime)."""
  for d in range(2, n):
    if n % d == 0:
      return d
  return 1


def _recipe_for(ties, k=0):
  if ties == 'none':
    return 'plain'
  return ('quantised', 'specials')[k % 2]


def _members():
  out = []
  for i, m in enumerate(MEMBERS):
    for k, nb in enumerate(bins_for(m)):
      ties = TIES[(i // 2 + k) % 4]
      out.append(Case('members', 'onehot', ties, DTYPES[(i + k) % 2], m, nb,
                      n_outer=2, n_point=(65, 63, 129)[k % 3],
                      stream=('member1', 'strided')[i % 2],
                      recipe=_recipe_for(ties, i)))
  # the exact multiples and every remainder again in the other forms
  for i, m in enumerate((4, 16, 20, 32, 19, 35)):
    form = ('counts', 'mean', 'sum')[i % 3]
    out.append(Case('members', form, 'first', DTYPES[i % 2], m, m + 1,
                    n_outer=4 if form == 'counts' else 1,
                    shape=None if form == 'counts' else (1, 2, 2),
                    n_point=65, recipe='quantised'))
  return out


# point counts by the occupancy of the last wave
_OCCUPANCY = {1: (1, 65, 129, 257, WAVE * 5 + 1), 63: (63, 127, 255),
              64: (64, 256)}


def _bins():
  out = []
  for i, nb in enumerate(WAVE_BINS):
    for k, occ in enumerate((1, 63, 64)):
      pts = _OCCUPANCY[occ]
      mult = 1 if nb >= 64 else (1, 2, 3)[(i + k) % 3] + (nb == 1)
      ties = TIES[(i + k) % 4]
      out.append(Case('bins', 'onehot', ties, DTYPES[(i + k) % 2],
                      nb * mult - 1, nb, n_outer=2,
                      n_point=pts[(i + k) % len(pts)],
                      stream=('member1', 'strided')[k % 2],
                      recipe=_recipe_for(ties)))
  return out


def _points():
  out = []
  for i, p in enumerate(POINTS):
    for k, dtype in enumerate(DTYPES):
      ties = TIES[(i + 2 * k + 1) % 4]
      out.append(Case('points', 'onehot', ties, dtype, (3, 5)[k], (4, 3)[k],
                      n_outer=3, n_point=p, n_col=_smallest_divisor(p),
                      stream=('rowmajor', 'transposed')[(i + k) % 2],
                      recipe=_recipe_for(ties, i)))
      if k != i % 2:
        continue
      form = ('counts', 'mean', 'sum')[i % 3]
      out.append(Case('points', form, 'first', dtype, 3, 2,
                      n_outer=3 if form == 'counts' else 1,
                      shape=None if form == 'counts' else (1, 3, 1),
                      n_point=p, recipe='specials'))
  # a last wave of 63, 64 and 1 points in every form
  for i, p in enumerate((63, 64, 65)):
    for k, form in enumerate(('counts', 'mean', 'sum')):
      out.append(Case('points', form, 'first', DTYPES[(i + k) % 2], 3, 2,
                      n_outer=3 if form == 'counts' else 1,
                      shape=None if form == 'counts' else (1, 3, 1),
                      n_point=p, recipe='specials'))
  return out


def _grid():
  out = []
  for i, dtype in enumerate(DTYPES):
    for k, form in enumerate(('onehot', 'counts')):
      out.append(Case('grid', form, ('numpy', 'first')[(i + k) % 2], dtype, 3,
                      (4, 2)[k], n_outer=SPLIT + 70, n_point=3,
                      stream=('member1', 'strided')[i], recipe='quantised'))
      out.append(Case('grid', form, ('first', 'numpy')[(i + k) % 2], dtype, 3,
                      (2, 4)[k], n_outer=SPLIT + 70, n_point=3,
                      stream=('strided', 'member1')[i], recipe='quantised'))
    for k, (lead, tail) in enumerate(((1, ROW_SPLIT + 5), (ROW_SPLIT + 5, 1))):
      out.append(Case('grid', ('mean', 'sum')[(i + k) % 2],
                      ('numpy', 'first')[k], dtype, 1, 2,
                      shape=(lead, 2, tail), n_point=2, recipe='quantised'))
  return out


_MEAN_BINS = ((5, 6), (5, 3), (255, 256), (7, 1), (50, 51), (127, 128),
              (255, 64), (1, 2))
_MEAN_POINTS = (1, 63, 64, 65, 129)


def _mean():
  out = []
  i = 0
  for shape in MEAN_SHAPES:
    for form in ('mean', 'sum'):
      m, nb = _MEAN_BINS[i % len(_MEAN_BINS)]
      ties = ('first', 'numpy', 'none', 'first', 'numpy')[i % 5]
      out.append(Case('mean', form, ties, DTYPES[(i // 2 + i) % 2], m, nb,
                      shape=shape, n_point=_MEAN_POINTS[i % 5],
                      stream=('member1', 'strided', 'nonmonotonic')[i % 3],
                      recipe={'first': 'specials', 'numpy': 'quantised',
                              'none': 'plain'}[ties]))
      i += 1
  # the LDS limit in both dtypes and both outputs, a ragged last wave
  for k, dtype in enumerate(DTYPES):
    for form in ('mean', 'sum'):
      out.append(Case('mean', form, 'first', dtype, MAX_BINS - 1, MAX_BINS,
                      shape=(2, 5, 3), n_point=(63, 65)[k], recipe='specials'))
  return out


def _slabs():
  out = []
  for i, slab in enumerate(SLABS):
    for k, form in enumerate(FORMS):
      for j, dtype in enumerate(DTYPES):
        if j != (i + k // 2) % 2:
          continue  # each layout meets each form once, and both dtypes
        ties = ('numpy', 'first')[(i + k) % 2]
        out.append(Case('slabs', form, ties, dtype, 5, (3, 6)[j],
                        n_outer=6 if form in ('onehot', 'counts') else 1,
                        shape=None if form in ('onehot', 'counts')
                        else (1, 3, 2),
                        n_point=65, slab=slab,
                        stream=('strided', 'member1')[(i + k) % 2],
                        recipe='quantised'))
  # hash ties: the draw depends on (o, pt) alone, whatever the tables say
  for j, dtype in enumerate(DTYPES):
    for slab in ('identity', 'permuted'):
      out.append(Case('slabs', 'onehot', 'hash', dtype, 5, 6, n_outer=6,
                      n_point=65, slab=slab, recipe='quantised', seed=77))
  return out


def _streams():
  out = []
  for i, stream in enumerate(STREAMS):
    for j, dtype in enumerate(DTYPES):
      few = stream in BASES
      n_point = 6 if few else 130
      n_col = {'member1': 0, 'strided': 0, 'rowmajor': 3 if few else 10,
               'transposed': 2 if few else 13}.get(stream, 0 if j else 2)
      out.append(Case('streams', 'onehot', 'numpy', dtype, (4, 17)[j],
                      (5, 6)[j], n_outer=2 if few else 3, n_point=n_point,
                      n_col=n_col, stream=stream, recipe='quantised',
                      seed=(0, 802701)[(i + j) % 2]))
    # the mean kernel walks the same stream through its own outer index
    if i % 2:
      continue
    out.append(Case('streams', ('mean', 'sum')[i // 2 % 2], 'numpy',
                    DTYPES[(i // 2 + 1) % 2], 3, 4, shape=(2, 2, 3),
                    n_point=6 if stream in BASES else 66,
                    n_col=0 if stream in ('member1', 'strided') else 3,
                    stream=stream, recipe='quantised', seed=9))
  return out


def _recipes():
  out = []
  for r, recipe in enumerate(RECIPES):
    for j, dtype in enumerate(DTYPES):
      if recipe == 'subnormal_gap' and dtype != 'float32':
        continue
      others = (('hash', 'first') if recipe == 'subnormal_gap'
                else (('hash', 'first')[(r + j) % 2],))
      for k, ties in enumerate(('numpy',) + others):
        for m in ((1, 3, 7) if ties == 'numpy' else ((3, 7)[(r + j) % 2],)):
          if ties == 'numpy' and m == 3 and recipe != 'subnormal_gap':
            continue
          big = recipe == 'subnormal_gap' and ties == 'numpy' and m == 3
          out.append(Case('recipes', 'onehot', ties, dtype, m, m + 1,
                          n_outer=8 if big else 4,
                          n_point=512 if big else 129,
                          stream=('member1', 'strided')[(r + m) % 2],
                          recipe=recipe, seed=(5, 11)[k % 2]))
  # the NaN and infinity rates against the member count: how many samples the
  # reference itself leaves open (asserted on the CPU)
  for j, dtype in enumerate(DTYPES):
    for m in (50, 255):
      out.append(Case('recipes', 'onehot', 'numpy', dtype, m, m + 1,
                      n_outer=2, n_point=257, stream=('member1', 'strided')[j],
                      recipe='specials', seed=3))
  return out


def _uniform():
  """all_equal under hash ties: the draw is uniform over 0..M (only that every
  rank occurs is asked here)."""
  return [Case('uniform', 'onehot', 'hash', DTYPES[m % 2], m, m + 1,
               n_outer=40, n_point=512, recipe='all_equal', seed=11 + m)
          for m in (1, 2, 3, 4, 5)]


def _cases():
  out, seen = [], set()
  for c in (_members() + _bins() + _points() + _grid() + _mean() + _slabs() +
            _streams() + _recipes() + _uniform()):
    if c.id not in seen:
      seen.add(c.id)
      out.append(c)
  return out


CASES = _cases()
GROUP_NAMES = tuple(dict.fromkeys(c.group for c in CASES))


# ---- data -------------------------------------------------------------------
def _rs(*key):
  return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _step(x, k):
  """x moved k representable values up (k < 0: down)."""
  toward = np.asarray(np.inf if k > 0 else -np.inf, dtype=x.dtype)
  for _ in range(abs(k)):
    x = np.nextafter(x, toward)
  return x


def _quantised(rs, shape, dtype, n_member):
  # few members: coarser values, so that ties stay common
  scale = 4.0 if n_member >= 8 else 1.0
  return (np.round(rs.standard_normal(shape) * scale) / 4).astype(dtype)


def _subnormal(rs, truth_shape, m):
  """float32 samples whose smallest positive gap is 4 ... 64 times the smallest
  subnormal.  Three classes of the tied value X (truth and one member):
  within the subnormals, where float64 holds every perturbed value exactly;
  near 2**-99, where the float64 sum rounds the perturbation to a few levels
  (the only place where the size's own rounding in float32 can show); and 1.0
  in a few samples, where the perturbation vanishes and the reference's order
  is open."""
  t = np.float64(TINY)
  n = int(np.prod(truth_shape))
  gap = lambda lo=4, hi=65: rs.randint(lo, hi, size=n).astype(np.float64)
  cls = rs.choice(3, size=n, p=[0.83, 0.15, 0.02])
  a = rs.randint(0, 100, size=n) * t
  small = np.where(cls == 1, gap(5, 8), gap())
  b = a + small * t
  x = np.where(cls == 0, b + gap() * t,
               np.where(cls == 1, 2.0**-99 * (1 + rs.randint(0, 2**20, size=n)
                                              / 2.0**21), 1.0))
  tied = rs.rand(n) < 0.7
  members = np.empty((n, m))
  if m >= 3:
    members[:, 0], members[:, 1] = a, b
    members[:, 2] = np.where(tied, x, x + gap() * t * (cls == 0) +
                             x * 0.5 * (cls != 0))
    for j in range(3, m):
      members[:, j] = rs.standard_normal(n) * 1e-10 * (j - 2)
    for row in members:
      rs.shuffle(row)
    truth = x
  else:
    # the truth in a chain of subnormal gaps, tied with the first member
    truth = b
    members[:, 0] = np.where(tied, b, a)
    if m == 2:
      members[:, 1] = b + gap() * t
  f32 = np.float32
  return truth.astype(f32).reshape(truth_shape), members.astype(f32).reshape(
      truth_shape + (m,))


def make_data(case):
  """The logical arrays the kernel sees through its tables: truth[o, pt] and
  ens[o, pt, m], plus the truth slabs and the map from o to them.  Cases that
  differ only in form, ties, slab or stream layout share their data."""
  o, p, m = case.n_outer, case.n_point, case.n_member
  dtype = np.dtype(case.dtype)
  shared = case.slab == 'shared_truth'
  rs = _rs('data', case.recipe, case.dtype, m, o, p, shared)
  tmap = np.arange(o) // SHARE if shared else np.arange(o)
  n_slab = int(tmap.max()) + 1
  recipe = case.recipe
  if recipe == 'plain':
    truth_slabs = rs.standard_normal((n_slab, p)).astype(dtype)
    ens = rs.standard_normal((o, p, m)).astype(dtype)
    truth = truth_slabs[tmap]
    ens = np.where(ens == truth[..., None], ens + dtype.type(1), ens)
  elif recipe in ('quantised', 'specials'):
    truth_slabs = _quantised(rs, (n_slab, p), dtype, m)
    ens = _quantised(rs, (o, p, m), dtype, m)
    if recipe == 'specials':
      rate = min(0.01, 0.5 / m)
      for value in (np.nan, np.inf, -np.inf):
        ens[rs.rand(o, p, m) < rate] = value
        truth_slabs[rs.rand(n_slab, p) < 0.02] = value
  elif recipe == 'all_equal':
    truth_slabs = _quantised(rs, (n_slab, p), dtype, m)
    ens = np.repeat(truth_slabs[tmap][..., None], m, axis=-1)
  elif recipe == 'one_ulp':
    truth_slabs = rs.standard_normal((n_slab, p)).astype(dtype)
    # powers of two: the gap below is half the gap above
    truth_slabs.ravel()[::7] = dtype.type(1.0)
    truth_slabs.ravel()[3::11] = dtype.type(-2.0)
    truth = truth_slabs[tmap]
    ens = np.empty((o, p, m), dtype=dtype)
    for j in range(m):
      steps = rs.choice([-3, -2, -1, 1, 2, 3], size=(o, p))
      for k in (-3, -2, -1, 1, 2, 3):
        ens[..., j] = np.where(steps == k, _step(truth, k), ens[..., j])
    # one exact tie in every 32nd sample
    tie = (np.arange(o * p).reshape(o, p) % 32) == 5
    ens[..., 0] = np.where(tie, truth, ens[..., 0])
  elif recipe == 'subnormal_gap':
    assert case.dtype == 'float32' and not shared
    truth_slabs, ens = _subnormal(rs, (o, p), m)
  else:
    raise ValueError(recipe)
  truth = truth_slabs[tmap]
  assert truth.dtype == dtype and ens.dtype == dtype
  return types.SimpleNamespace(truth=truth, ens=ens, truth_slabs=truth_slabs,
                               tmap=tmap)


def make_buffers(case, data):
  """The device-side picture: flat member and truth buffers, the member
  stride and the two slab tables (None: identity)."""
  o, p, m = case.n_outer, case.n_point, case.n_member
  dtype = np.dtype(case.dtype)
  rs = _rs('tables', case.id)
  by_member = np.ascontiguousarray(np.moveaxis(data.ens, -1, 0))  # [m, o, p]
  ens_slab = truth_slab = None
  truth_buf = data.truth
  stride = o * p
  if case.slab == 'identity':
    ens_buf = by_member
  elif case.slab == 'padded':
    stride = o * p + PAD
    ens_buf = np.full((m, stride), np.nan, dtype=dtype)
    ens_buf[:, :o * p] = by_member.reshape(m, o * p)
  elif case.slab == 'member_inner':
    ens_buf = np.ascontiguousarray(np.moveaxis(data.ens, -1, 1))  # [o, m, p]
    ens_slab = np.arange(o, dtype=np.int64) * m
    stride = p
  elif case.slab == 'permuted':
    ens_slab = rs.permutation(o).astype(np.int64)
    truth_slab = rs.permutation(o).astype(np.int64)
    ens_buf = np.empty_like(by_member)
    ens_buf[:, ens_slab] = by_member
    truth_buf = np.empty_like(data.truth)
    truth_buf[truth_slab] = data.truth
  elif case.slab == 'shared_truth':
    ens_buf = by_member
    truth_buf = data.truth_slabs
    truth_slab = data.tmap.astype(np.int64)
  return types.SimpleNamespace(
      ens=np.ascontiguousarray(ens_buf).ravel(), member_stride=int(stride),
      ens_slab=ens_slab, truth=np.ascontiguousarray(truth_buf).ravel(),
      truth_slab=truth_slab)


def make_stream(case):
  """Where the reference's concatenated [truth, members] array keeps element
  (o, pt, j) in C order: ref_outer_off[o], the (row, col, member) strides, and
  the index of every element, int64 [o, pt, M + 1]."""
  o, p, m1 = case.n_outer, case.n_point, case.n_member + 1
  n_col = case.n_col
  n_row = p // n_col
  if case.stream == 'member1':
    strides = (n_col * m1, m1, 1)      # truth's dims, then the members
  elif case.stream == 'transposed':
    strides = (1, n_row, p)            # [o, member, col, row]
  else:
    strides = (n_col, 1, p)            # [o, member, row, col]
  off = np.arange(o, dtype=np.int64) * (p * m1)
  if case.stream == 'nonmonotonic':
    # neighbours swapped: 1, 0, 3, 2, ... goes down and up
    order = np.arange(o) ^ 1
    order[order >= o] = o - 1
    off = off[order]
    assert o < 3 or ((np.diff(off) < 0).any() and (np.diff(off) > 0).any())
  off = off + BASES.get(case.stream, 0)
  pt = np.arange(p, dtype=np.int64)
  at = (pt // n_col) * strides[0] + (pt % n_col) * strides[1]
  index = (off[:, None, None] + at[None, :, None] +
           np.arange(m1, dtype=np.int64)[None, None, :] * strides[2])
  return types.SimpleNamespace(off=off, strides=strides, n_col=n_col,
                               index=index)


def acc_rows(case):
  """counts: outer indices 2r and 2r + 1 add into row r, in a shuffled order of
  rows; the last row is named by nobody."""
  assert case.form == 'counts'
  order = _rs('rows', case.id).permutation(case.n_acc - 1)
  return order[np.arange(case.n_outer) // 2].astype(np.int64)


def expected(case, data=None):
  """What the references of tests/rank_np.py say about a case: lo, eq, nn and
  the rank without tie breaking per sample [o, pt]; under numpy ties also the
  reference's rank, its perturbed values, where it leaves the order open
  (`open`) and the bounds (#less, #equal) that hold even there."""
  from tests import rank_np
  data = make_data(case) if data is None else data
  lo, eq, nn = rank_np.counts(data.ens, data.truth)
  out = types.SimpleNamespace(lo=lo, eq=eq, nn=nn, data=data,
                              first=rank_np.first_rank(data.ens, data.truth))
  if case.ties == 'numpy':
    stream = make_stream(case)
    values = np.concatenate([data.truth[..., None], data.ens], axis=-1)
    out.rank, out.perturbed = rank_np.numpy_rank(values, stream.index,
                                                 case.seed, case.dtype)
    out.open = rank_np.ambiguous(out.perturbed)
    out.less, out.equal = rank_np.perturbed_bounds(out.perturbed)
    out.stream = stream
  return out
