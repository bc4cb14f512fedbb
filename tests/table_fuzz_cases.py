"""The seeded case list of the verification-table fuzz: K18 event tables, K19
fractions / FSS, K20 CRPS bins, K21 twCRPS, K22 pooling, K24 conditional
tables -- 40 cases per family, drawn with np.random.RandomState alone.

One list for tests/test_table_fuzz_cpu.py, which holds the package's host path
to the independent definitions of tests/*_np.py on the CPU and asserts what
the list reaches, and tests/test_table_fuzz_gpu.py, which holds the kernels to
both.  A case is a frozen record of its draw; `arrays`, `engine_tables` and
`oracle_region_set` make its arrays, classes, fold weights and regions from
its seed.

The draw:

  rows, columns   n_row in 1..24; half the n_col uniform in 1..200, half from
                  1, 2, 3 and 62..66, 126..130, 190..194 (the 64-column tile
                  and the 16-byte lane borders from both sides; a family's
                  cases walk through all of them).  K21 and K24
                  take n_col >= 2: their bounds (twcrps_np.table_rtol,
                  conditional_np.table_atol) are derived for n_lon >= 2.
  outer, dtype    n_outer in 1..3 (metric level: time x prediction_timedelta);
                  float32 or float64, K21 at metric level also float32 data
                  under float64 thresholds ('mixed').
  members         1..64 (K20, K21, K24), 1..128 (K18, K19), 1..4 fields per
                  outer index for K22; every third case from the borders of
                  the padded networks (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33,
                  63, 64, and 127, 128 for K18 / K19)
  values          a 0.1 grid.  K18 / K19: events_cases.edge_case (NaN in the
                  truth, a member and the threshold, +-inf, planted ties).
                  K20 / K21 / K24: a NaN pattern of the family's NANS; no
                  +-inf, which these tables do not pin (a sum would hold inf
                  - inf).  K22: NaN, +-inf and -0.0 sprinkled.
  thresholds      1..6 (K18, K19, K21): 5 and 6 are a second launch
  windows         1..6 odd windows <= min(n_col, 255) -- K22: also <= the
                  largest window its kernel stages (POOL_MAX_WINDOW) --, one
                  of them taller than n_row where n_col allows, n_col itself
                  where it is odd and allowed
  tail, by, kind  K21 / K24 / K22; K24 with 1..8 bin edges on the grid of the
                  values, one of them a value of the truth
  level           even cases 'engine': random int32 column classes -- unsorted
                  labels, runs of random length, the first class again at the
                  row end, n_class in 1..64 with a class that no column has
                  (n_class > 1) -- and random fold weights; odd cases
                  'metric': a subset of events_cases.oracle_regions() and two
                  random lat / lon boxes, through `compute_chunk`, with the
                  forecast in one of FORMS
"""
import dataclasses
import functools
import typing as t

import numpy as np

FAMILIES = ('k18', 'k19', 'k20', 'k21', 'k22', 'k24')
N_PER_FAMILY = 40
NAME = 'x'
FORMS = ('contiguous', 'lead_view', 'gather', 'lonlat', 'offset')
SPECIAL_COLS = (1, 2, 3) + tuple(range(62, 67)) + tuple(range(126, 131)) + (
    tuple(range(190, 195)))
SPECIAL_MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
WIDE_MEMBERS = SPECIAL_MEMBERS + (127, 128)
# engine.pool_geometry(dtype)['max_window'] (asserted on the CPU)
POOL_MAX_WINDOW = {'float32': 123, 'float64': 87}
TAILS = ('upper', 'lower')
N_FOLD_REGION = 3  # regions of the random fold weights (engine level)
_SEED0 = {f: 1000 * (k + 1) for k, f in enumerate(FAMILIES)}


@dataclasses.dataclass(frozen=True)
class Case:
  family: str
  index: int
  seed: int
  level: str                 # 'engine' | 'metric'
  form: t.Optional[str]      # metric level: one of FORMS
  dtype: str                 # 'float32' | 'float64' | 'mixed'
  n_outer: int
  lead_major: bool           # metric level: the outer indices are leads
  n_row: int
  n_col: int
  n_member: int
  nan: str                   # the family's NaN pattern ('edge': edge_case)
  skipna: bool
  n_thr: int                 # K18, K19, K21
  windows: tuple             # K19, K22
  tail: t.Optional[str]      # K21
  by: t.Optional[str]        # K24
  n_edge: int                # K24
  kind: t.Optional[str]      # K22
  n_class: int               # engine level

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'float64' else np.float32

  @property
  def thr_dtype(self):
    return np.float32 if self.dtype == 'float32' else np.float64

  @property
  def outer_shape(self):
    """(time, prediction_timedelta) of the metric level."""
    return (1, self.n_outer) if self.lead_major else (self.n_outer, 1)

  @property
  def id(self):
    parts = [self.family, str(self.index), self.level[0] + (
        '-' + self.form if self.form else ''), self.dtype,
             f'o{self.n_outer}r{self.n_row}c{self.n_col}m{self.n_member}',
             self.nan, 'skipna' if self.skipna else 'strict']
    if self.n_thr:
      parts.append(f't{self.n_thr}')
    if self.windows:
      parts.append('w' + '.'.join(map(str, self.windows)))
    for extra in (self.tail, self.kind):
      if extra:
        parts.append(extra)
    if self.by:
      parts.append(f'{self.by}{self.n_edge}')
    if self.level == 'engine':
      parts.append(f'k{self.n_class}')
    return '-'.join(parts)


# ---------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------
def _windows(rs, n_row, n_col, limit):
  """1..6 distinct odd windows <= min(n_col, limit): one taller than the grid
  and n_col itself where they are allowed, the rest random, in random order."""
  top = min(n_col, limit)
  odd = np.arange(1, top + 1, 2)
  want = min(int(rs.randint(1, 7)), odd.size)
  picked = []
  tall = odd[odd > n_row]
  if tall.size:
    picked.append(int(tall[rs.randint(min(tall.size, 4))]))
  if n_col % 2 == 1 and n_col <= top and n_col not in picked:
    picked.append(n_col)
  # (small windows more often than large ones)
  pool = [int(n) for n in odd if n not in picked]
  rs.shuffle(pool)
  pool.sort(key=lambda n: n > 17)
  picked += pool[:max(0, want - len(picked))]
  rs.shuffle(picked)
  return tuple(picked)


def _case(family, index):
  seed = _SEED0[family] + index
  rs = np.random.RandomState(seed)
  level = 'engine' if index % 2 == 0 else 'metric'
  # (the 20 metric cases of a family take every form four times)
  form = FORMS[(index // 2) % len(FORMS)] if level == 'metric' else None
  n_row = int(rs.randint(1, 25))
  # pairs of cases (one of each level) take turns: uniform columns, then the
  # special ones, which the 20 such cases of a family walk through in order
  # from a start of the family's own, so that every one of them is met
  if (index // 2) % 2:
    n_col = int(rs.randint(1, 201))
  else:
    k = (index // 4) * 2 + index % 2 + 5 * FAMILIES.index(family)
    n_col = int(SPECIAL_COLS[k % len(SPECIAL_COLS)])
  if family in ('k21', 'k24'):
    n_col = max(n_col, 2)
  n_outer = int(rs.randint(1, 4))
  dtypes = ['float32', 'float64']
  if family == 'k21' and level == 'metric':
    dtypes.append('mixed')
  dtype = dtypes[rs.randint(len(dtypes))]
  if family == 'k22':
    n_member = int(rs.randint(1, 5))
  else:
    top, special = ((128, WIDE_MEMBERS) if family in ('k18', 'k19')
                    else (64, SPECIAL_MEMBERS))
    if index % 3 == 0:
      # (every third case walks down the border counts, largest first)
      n_member = int(special[-1 - (index // 3) % len(special)])
    else:
      n_member = int(rs.randint(1, top + 1))
  skipna = bool(rs.randint(2))
  if family in ('k18', 'k19'):
    nan = 'edge'
  elif family == 'k22':
    nan = ('none', 'planted')[rs.randint(2)]
  else:
    from tests import crps_decomposition_cases, twcrps_cases
    nans = (twcrps_cases.NANS if family == 'k21'
            else crps_decomposition_cases.NANS)
    # (without skipna a NaN voids its slab: half of those cases have none)
    nan = 'none' if (not skipna and rs.rand() < 0.5) else str(
        nans[rs.randint(len(nans))])
  n_thr = int(rs.randint(1, 7)) if family in ('k18', 'k19', 'k21') else 0
  windows = ()
  if family == 'k19':
    windows = _windows(rs, n_row, n_col, 255)
  elif family == 'k22':
    windows = _windows(rs, n_row, n_col,
                       POOL_MAX_WINDOW['float64' if dtype == 'float64'
                                       else 'float32'])
  tail = TAILS[rs.randint(2)] if family == 'k21' else None
  by, n_edge = None, 0
  if family == 'k24':
    from tests import conditional_cases
    by = str(conditional_cases.BYS[rs.randint(len(conditional_cases.BYS))])
    n_edge = int(rs.randint(1, 9))
    if by == 'spread':
      n_member = max(n_member, 2)  # (one member has no spread to bin by)
  kind = None
  if family == 'k22':
    from tests import pooling_cases
    kind = str(pooling_cases.KINDS[rs.randint(len(pooling_cases.KINDS))])
  n_class = 0
  if level == 'engine' and family != 'k22':
    # (two cases of a family have the one class that cannot be left unused)
    n_class = 1 if index % 16 == 8 else int(rs.randint(2, 65))
  return Case(family, index, seed, level, form, dtype, n_outer,
              bool(rs.randint(2)), n_row, n_col, n_member, nan, skipna, n_thr,
              windows, tail, by, n_edge, kind, n_class)


CASES = tuple(_case(f, i) for f in FAMILIES for i in range(N_PER_FAMILY))
BY_FAMILY = {f: tuple(c for c in CASES if c.family == f) for f in FAMILIES}


# ---------------------------------------------------------------------------
# the arrays of a case
# ---------------------------------------------------------------------------
def _grid_values(rs, shape, dtype, shift=0.0):
  return (np.round(rs.normal(size=shape), 1) + shift).astype(dtype)


def column_classes(case, rs):
  """int32 [n_col]: unsorted labels in runs of random length, the first class
  again in the last column, and (n_class > 1) a class that no column has."""
  n_col, n_class = case.n_col, case.n_class
  n_used = int(rs.randint(1, max(2, min(n_class, n_col + 1))))
  labels = rs.permutation(n_class)[:n_used]
  cls = np.empty(n_col, np.int32)
  j = 0
  while j < n_col:
    run = int(rs.randint(1, 18))
    cls[j:j + run] = labels[rs.randint(n_used)]
    j += run
  if n_col >= 3 and n_used >= 2 and (cls == cls[0]).all():
    cls[n_col // 2] = labels[1] if labels[0] == cls[0] else labels[0]
  # every other row longer than a 64-column tile changes its class exactly at
  # the tile border
  if n_col > 65 and n_used >= 2 and rs.randint(2):
    other = labels[labels != cls[63]]
    cls[64:64 + int(rs.randint(1, 18))] = other[rs.randint(other.size)]
  cls[-1] = cls[0]
  return cls


def fold_weights(case, rs):
  """(wrow float64 [3, n_row], mult int32 [3, n_class]) of the engine level:
  row weights times 0, 1 or 2 and column multiplicities 0, 1, 2; region 0
  weighs every point."""
  wrow = (rs.rand(N_FOLD_REGION, case.n_row) + 0.1) * rs.randint(
      0, 3, size=(N_FOLD_REGION, case.n_row))
  mult = rs.randint(0, 3, size=(N_FOLD_REGION, case.n_class)).astype(np.int32)
  wrow[0] = rs.rand(case.n_row) + 0.1
  mult[0] = 1
  return wrow, mult


def _plant_nans(case, rs, ens, truth, thrs):
  """The NaN pattern of K20 / K21 / K24 (arrays [M, O, R, C], [O, R, C]): 8%
  of the points with skipna; without it a few points of outer index 0 alone
  (a NaN voids its slab; the other slabs stay)."""
  shape = truth.shape
  if case.skipna:
    hits = lambda: rs.rand(*shape) < 0.08
  else:
    def hits():
      h = np.zeros(shape, bool)
      n = int(rs.randint(1, 4))
      h[0].reshape(-1)[rs.randint(0, h[0].size, size=n)] = True
      return h
  if case.nan in ('truth', 'both', 'threshold'):
    truth[hits()] = np.nan
  if case.nan in ('member', 'both', 'threshold'):
    member = rs.randint(case.n_member, size=shape)
    for idx in zip(*np.nonzero(hits())):
      ens[(member[idx],) + idx] = np.nan
  if case.nan == 'threshold':
    # in the first threshold (and the fifth: the second launch) alone, so
    # that validity differs between the thresholds of one launch
    for k in (0, 4):
      if k < len(thrs):
        thrs[k][hits()] = np.nan
  # at least one valid point in every slab
  ens[:, :, 0, 0] = np.where(np.isnan(ens[:, :, 0, 0]), 0.5, ens[:, :, 0, 0])
  truth[:, 0, 0] = np.where(np.isnan(truth[:, 0, 0]), -0.5, truth[:, 0, 0])
  if thrs:
    thrs[0][:, 0, 0] = np.where(np.isnan(thrs[0][:, 0, 0]), 0.0,
                                thrs[0][:, 0, 0])


def _bin_edges(case, rs, truth):
  """1..8 strictly increasing edges on the 0.1 grid as the metric takes them
  ('spread': standard deviations >= 0), one of them a value of the truth."""
  finite = truth[np.isfinite(truth)].astype(np.float64)
  pin = float(finite[rs.randint(finite.size)])
  if case.by == 'spread':
    pin = abs(pin)
    pool = np.round(np.arange(0, 31) * 0.1, 1)
  else:
    pool = np.round(np.arange(-25, 26) * 0.1, 1)
  # (the grid in the dtype of the data, widened: where the values lie)
  pool = pool.astype(case.np_dtype).astype(np.float64)
  picked = {pin}
  for v in rs.permutation(pool):
    if len(picked) >= case.n_edge:
      break
    picked.add(float(v))
  return tuple(sorted(picked))


@functools.lru_cache(maxsize=None)
def arrays(case):
  """The arrays of a case, as a dict, computed once and left unchanged:
  'ens' [M, O, R, C] and 'truth' [O, R, C] (K22: 'x' [O, M, R, C]), 'thrs' (a
  list of [O, R, C]), 'edges' (K24, as the metric takes them)."""
  rs = np.random.RandomState(case.seed + 500000)
  m, o, r, c = case.n_member, case.n_outer, case.n_row, case.n_col
  out = {}
  if case.family in ('k18', 'k19'):
    from tests import events_cases
    ens, truth, thrs = events_cases.edge_case(m, case.n_thr, o, r, c,
                                              case.np_dtype, seed=case.seed)
    if not case.skipna and o > 1:
      # (edge_case plants NaNs in every slab; without skipna they void it:
      # outer index 0 alone keeps them)
      fill = case.np_dtype(0.3)
      ens[:, 1:] = np.where(np.isnan(ens[:, 1:]), fill, ens[:, 1:])
      truth[1:] = np.where(np.isnan(truth[1:]), -fill, truth[1:])
    out.update(ens=ens, truth=truth, thrs=thrs)
  elif case.family == 'k22':
    x = _grid_values(rs, (o, m, r, c), case.np_dtype)
    if case.nan == 'planted':
      n = x.size
      flat = x.reshape(-1)
      for value, share in ((np.nan, 0.01), (np.inf, 0.01), (-np.inf, 0.01),
                           (-0.0, 0.05)):
        flat[rs.randint(0, n, size=max(1, int(share * n)))] = value
      x[..., 0, 0] = 0.7  # (a finite value in every field)
    out.update(x=x)
  else:
    ens = _grid_values(rs, (m, o, r, c), case.np_dtype)
    truth = _grid_values(rs, (o, r, c), case.np_dtype)
    thrs = [_grid_values(rs, (o, r, c), case.thr_dtype, 0.3 * k - 0.4)
            for k in range(case.n_thr)]
    _plant_nans(case, rs, ens, truth, thrs)
    out.update(ens=ens, truth=truth, thrs=thrs)
    if case.family == 'k24':
      out.update(edges=_bin_edges(case, rs, truth))
  for v in out.values():
    for a in (v if isinstance(v, list) else [v]):
      if isinstance(a, np.ndarray):
        a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def engine_tables(case):
  """(col_class, wrow, mult) of an engine-level case."""
  rs = np.random.RandomState(case.seed + 600000)
  cls = column_classes(case, rs)
  wrow, mult = fold_weights(case, rs)
  for a in (cls, wrow, mult):
    a.setflags(write=False)
  return cls, wrow, mult


def axes(n_row, n_col):
  """Increasing latitudes and a cyclic longitude axis."""
  lat = np.linspace(-80.0, 80.0, n_row) if n_row > 1 else np.array([30.0])
  return lat, np.arange(n_col) * (360.0 / n_col)


@functools.lru_cache(maxsize=None)
def oracle_region_set(case):
  """{name: oracle region} of a metric-level case: 'global', a random subset
  of events_cases.oracle_regions() and two random lat / lon boxes (slices
  that hold at least one point)."""
  from oracle import regions_np as oreg
  from tests import events_cases
  rs = np.random.RandomState(case.seed + 700000)
  known = events_cases.oracle_regions()
  names = [n for n in known if n != 'global']
  picked = ['global'] + [names[k] for k in sorted(
      rs.permutation(len(names))[:rs.randint(1, 6)])]
  out = {n: known[n] for n in picked}
  lat, lon = axes(case.n_row, case.n_col)
  step = 360.0 / case.n_col
  for k in range(2):
    i0 = int(rs.randint(case.n_row))
    i1 = int(rs.randint(i0, case.n_row))
    j0 = int(rs.randint(case.n_col))
    j1 = int(rs.randint(j0, case.n_col))
    out[f'box{k}'] = oreg.SliceRegion(
        lat_slice=slice(float(lat[i0]) - 0.01, float(lat[i1]) + 0.01),
        lon_slice=slice(float(lon[j0]) - step / 4, float(lon[j1]) + step / 4))
  return out


def coords(case):
  n_time, n_lead = case.outer_shape
  lat, lon = axes(case.n_row, case.n_col)
  return {'realization': np.arange(case.n_member),
          'time': (np.datetime64('2020-01-01', 'ns') +
                   np.arange(n_time) * np.timedelta64(1, 'D')),
          'prediction_timedelta': np.arange(n_lead) * np.timedelta64(1, 'D'),
          'latitude': lat, 'longitude': lon}


OUTER_DIMS = ('time', 'prediction_timedelta')
SPATIAL = ('latitude', 'longitude')
