"""The geometry sweep of the ensemble reductions: K3 (ens_partials_kernel +
wb2_ens_combine), K3t (ens_threshold_kernel + wb2_det_combine) and K3e
(energy_partials_kernel), which fold into region segments through
fold_tile_to_segs like K1.

One case list for test_ens_geometry_gpu.py, which runs it against a plain
float64 reference, and test_ens_geometry_cpu.py, which asserts on the CPU that
the list reaches every kernel family, tile, row-end, 64-row-block and segment
edge it is meant to reach.  The column tile of all three kernels is T = 64
columns (wb2_ens_tile_cols), one column per lane.
"""
import dataclasses
import typing as t

from tests import stream_geometry_cases as sg

T = 64
# 1 and 2 (one wave, few lanes), both sides of 1 and 2 tiles, an odd tile count
# (3: the second wave of the last two-wave workgroup has no tile), 5 tiles + 3
N_COL = (1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T,
         5 * T + 3)
N_ROW = (1, 2, 9, 37, 131)
ROWS_PER_CHUNK = (1, 5, 7, 64, 65, 130)  # 5 = plan.ENSEMBLE_ROWS_PER_CHUNK
LONG_ROWS = 131  # chunks of 65 and 129 rows: a second 64-row block

# K3's kernel families (ensemble.hip launch_ens_npad): dtype, the member
# counts that select the family, members gathered through member_ptrs or not
FAMILIES = {
    'exact50': ('float32', (50,), False),           # the exact-50 program
    'exact': ('float32', (5, 36), False),           # a WB2_SORT3_SIZES count
    'hosted': ('float32', (7, 70), False),          # inside a larger program
    'hosted_gather': ('float32', (44, 70), True),   # 70: two address lanes
    'f32_m1': ('float32', (1,), False),
    'pad128': ('float32', (110,), False),           # the padded-128 network
    'pad128_gather': ('float32', (120,), True),
    'stream_f32': ('float32', (130,), False),       # NPAD = 0: no sort
    'stream_f64': ('float64', (66,), False),
    'f64pad': ('float64', (3, 16, 30, 64), False),  # padded 4, 16, 32, 64
    'f64pad_gather': ('float64', (3, 16, 30, 64), True),
}
TWO_PASS = ('exact50', 'exact', 'hosted', 'hosted_gather')
STRIDED_SLABS = ('contiguous', 'table', 'addr', 'addr_offset', 'stride')
ENERGY_M = (1, 8, 9, 17, 50)  # across the kernel's 8-member blocks
ZGRID_OUTER = 32768 + 70      # past the grid's y limit: blockIdx.z > 0


@dataclasses.dataclass(frozen=True)
class Case:
  kernel: str            # 'k3' | 'k3t' | 'k3e'
  family: str            # K3: a key of FAMILIES; else the dtype
  dtype: str
  n_member: int
  layout: str            # 'latlon' | 'lonlat'
  skipna: bool
  n_col: int
  n_row: int
  rows_per_chunk: int
  field: t.Optional[str]  # None, 'f32' (float32 numbers) or 'f64'
  slabs: str             # STRIDED_SLABS, 'gather' or 'zgrid'

  @property
  def gather(self):
    return self.slabs == 'gather'

  @property
  def n_outer(self):
    return ZGRID_OUTER if self.slabs == 'zgrid' else None

  @property
  def id(self):
    return (f'{self.kernel}-{self.family}-m{self.n_member}-{self.layout}-'
            f'{"skipna" if self.skipna else "strict"}-c{self.n_col}-'
            f'r{self.n_row}-k{self.rows_per_chunk}-{self.field or "nofield"}-'
            f'{self.slabs}')


def _rows(i, n_col):
  """(n_row, rows_per_chunk) of the i-th case: few rows on wide grids."""
  n_row = N_ROW[i % 4] if n_col <= 2 * T + 1 else (1, 2, 9)[i % 3]
  return n_row, ROWS_PER_CHUNK[i % 4] if n_row > 1 else 1


def _cases():
  out = []
  i = 0
  for fam, (dtype, ms, gather) in FAMILIES.items():
    for skipna in (False, True):
      for j, n_col in enumerate(N_COL):
        n_row, rpc = _rows(i, n_col)
        out.append(Case(
            'k3', fam, dtype, ms[j % len(ms)], ('latlon', 'lonlat')[i % 2],
            skipna, n_col, n_row, rpc, ('f32', None, 'f64')[i % 3],
            'gather' if gather else STRIDED_SLABS[i % 5]))
        i += 1
    # a chunk of more than 64 rows (lonlat: the extratropics cut no rows)
    if fam in TWO_PASS:
      for j, rpc in enumerate((64, 65, 130)):
        out.append(Case(
            'k3', fam, dtype, ms[j % len(ms)], 'lonlat', True,
            (T + 1, 2 * T - 1, 2 * T + 1)[j], LONG_ROWS, rpc, (None, 'f64')[j % 2],
            'gather' if gather else STRIDED_SLABS[j]))
  for dtype in ('float32', 'float64'):
    for skipna in (False, True):
      for j, n_col in enumerate(N_COL):
        n_row, rpc = _rows(i, n_col)
        out.append(Case('k3t', dtype, dtype, (3, 8, 50)[j % 3],
                        ('latlon', 'lonlat')[i % 2], skipna, n_col, n_row, rpc,
                        ('f32', None, 'f64')[i % 3], ('contiguous',
                                                      'table')[i % 2]))
        i += 1
  for skipna in (False, True):
    for j, n_col in enumerate(N_COL):
      n_row, rpc = _rows(i, n_col)
      dtype = ('float32', 'float64')[j % 2]
      out.append(Case('k3e', dtype, dtype, ENERGY_M[(j + skipna) % 5],
                      ('latlon', 'lonlat')[i % 2], skipna, n_col, n_row, rpc,
                      ('f64', None, None)[i % 3], ('contiguous',
                                                   'table')[i % 2]))
      i += 1
  # n_outer past the grid's y dimension, one case per kernel
  out.append(Case('k3', 'exact', 'float32', 5, 'latlon', False, T + 1, 1, 1,
                  None, 'zgrid'))
  out.append(Case('k3t', 'float32', 'float32', 3, 'latlon', True, T + 1, 1, 1,
                  None, 'zgrid'))
  out.append(Case('k3e', 'float64', 'float64', 9, 'latlon', False, T + 1, 1,
                  1, None, 'zgrid'))
  return out


CASES = _cases()


@dataclasses.dataclass
class Resolved:
  case: Case
  n_row: int
  n_col: int
  lat: t.Any
  lon: t.Any
  regions: dict  # oracle regions


def resolve(case: Case) -> Resolved:
  """Coordinates and oracle regions of a case.  The regions are those of the
  K1 sweep at T = 64 columns per tile and one column per lane, plus 'to_n2':
  the columns just before the last one, ending at n_col - 2."""
  lat, lon = sg.coords(case.n_row, case.n_col, case.layout)
  if case.slabs == 'zgrid':
    from oracle import regions_np as oreg
    regs = {'global': oreg.SliceRegion()}
  else:
    regs = sg.regions(case, case.n_row, case.n_col, 1, T, lat, lon)
  n = case.n_col
  if n >= 2:
    from oracle import regions_np as oreg
    cols = lat if case.layout == 'lonlat' else lon
    c = slice(float(cols[max(n - 5, 0)]), float(cols[n - 2]))
    regs['to_n2'] = (oreg.SliceRegion(lon_slice=c) if case.layout == 'latlon'
                     else oreg.SliceRegion(lat_slice=c))
  return Resolved(case, case.n_row, n, lat, lon, regs)
