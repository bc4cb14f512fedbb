"""The geometry sweep of the streaming reduction (K1 / K1p + the K2 fold).

One case list for test_stream_geometry_gpu.py, which runs it against a plain
float64 reference, and test_stream_geometry_cpu.py, which asserts on the CPU
that the list reaches every tile, tail and segment edge it is meant to reach.

Widths are symbolic in the lane width VEC and the wave's column tile T = 64 VEC
(wb2_tile_cols_ex); `resolve` turns a case into numbers for one library.  A
column count below VEC runs the narrow VEC = 1 instantiation.
"""
import dataclasses
import re
import typing as t

import numpy as np

from oracle import regions_np as oreg
from oracle.named import NA

# n_col: every residue of n_col % VEC, the row-end lane's shift-back across a
# tile edge (T + r, 0 < r < VEC), 1, 2, 3, 4 and 6 tiles, the narrow path
N_COL = ('1', 'VEC-1', 'VEC', 'VEC+1', 'T-1', 'T', 'T+1', 'T+2', 'T+VEC-1',
         '2T+1', '3T-1', '3T+VEC-1', '5T+3')
N_ROW = (1, 2, 9, 37)
ROWS_PER_CHUNK = (1, 3, 7, 9, None)  # None: plan.DEFAULT_ROWS_PER_CHUNK
SLABS = ('contiguous', 'table', 'addr', 'addr_offset')
MODES = ('det', 'det_acc', 'wind')


def n_col_of(sym: str, vec: int, tile: int) -> int:
  """'3T+VEC-1' -> 3 * tile + vec - 1."""
  total = 0
  for term in re.findall(r'[+-]?[^+-]+', sym):
    sign = -1 if term[0] == '-' else 1
    term = term.lstrip('+-')
    if term.endswith('VEC'):
      total += sign * int(term[:-3] or 1) * vec
    elif term.endswith('T'):
      total += sign * int(term[:-1] or 1) * tile
    else:
      total += sign * int(term)
  return total


@dataclasses.dataclass(frozen=True)
class Case:
  mode: str              # 'det' | 'det_acc' | 'wind'
  dtype: str             # 'float32' | 'float64'
  layout: str            # 'latlon' | 'lonlat'
  skipna: bool
  n_col: str             # a symbol of N_COL
  n_row: int
  rows_per_chunk: t.Optional[int]
  field: t.Optional[str]  # None, 'f32' (float32 numbers) or 'f64'
  slabs: str             # one of SLABS

  @property
  def id(self):
    rpc = 'dflt' if self.rows_per_chunk is None else self.rows_per_chunk
    return (f'{self.mode}-{self.dtype}-{self.layout}-'
            f'{"skipna" if self.skipna else "strict"}-c{self.n_col}-'
            f'r{self.n_row}-k{rpc}-{self.field or "nofield"}-{self.slabs}')


def _cases():
  out = []
  i = 0
  # DET: every n_col x dtype x layout x skipna
  for dtype in ('float32', 'float64'):
    for layout in ('latlon', 'lonlat'):
      for skipna in (False, True):
        for sym in N_COL:
          out.append(Case('det', dtype, layout, skipna, sym, N_ROW[i % 4],
                          ROWS_PER_CHUNK[i % 5], None, SLABS[(i // 3) % 4]))
          i += 1
  # DET_ACC, WIND and the weight-field regions: every n_col once per mode and
  # dtype; layout, skipna and field rotate
  for mode in MODES:
    for dtype in ('float32', 'float64'):
      for j, sym in enumerate(N_COL):
        field = ('f32', 'f64', None)[(j + (mode == 'wind')) % 3]
        out.append(Case(mode, dtype, ('latlon', 'lonlat')[(i // 2) % 2],
                        bool((i // 3) % 2), sym, N_ROW[(i + 1) % 4],
                        ROWS_PER_CHUNK[i % 5], field, SLABS[i % 4]))
        i += 1
  return out


CASES = _cases()


def lib_vec(lib, case: Case) -> int:
  """The wide lane width of the case's launch (columns per lane)."""
  from weatherbench2_amd import _lib
  mode = {'det': _lib.MODE_DET, 'det_acc': _lib.MODE_DET_ACC,
          'wind': _lib.MODE_WIND}[case.mode]
  code = _lib.WB2_F32 if case.dtype == 'float32' else _lib.WB2_F64
  return lib.wb2_tile_cols_ex(mode, code, int(case.skipna),
                              int(case.field is not None), 1 << 20, 1) // 64


def coords(n_row: int, n_col: int, layout: str):
  """(latitude, longitude) labels of a slab of n_row x n_col in `layout`.
  Latitudes stay inside +-88.5 degrees: no cell weight is tiny."""
  n_lat, n_lon = (n_row, n_col) if layout == 'latlon' else (n_col, n_row)
  lat = np.linspace(-88.5, 88.5, n_lat) if n_lat > 1 else np.array([30.0])
  lon = np.arange(n_lon) * (360.0 / n_lon)
  return lat, lon


def land_mask(kind: str, lat, lon, seed=7):
  """A land fraction [n_lat, n_lon]: zeros, and values in [0.25, 1] that are
  float32 numbers ('f32') or not ('f64')."""
  rs = np.random.RandomState(seed)
  shape = (len(lat), len(lon))
  if kind == 'f32':
    m = rs.randint(2, 9, size=shape) / 8.0
  else:
    m = 0.25 + 0.75 * rs.uniform(size=shape) + 1e-9
  m[rs.uniform(size=shape) < 0.25] = 0.0
  return np.minimum(m, 1.0)


def regions(case: Case, n_row: int, n_col: int, vec: int, tile: int,
            lat, lon) -> dict:
  """Ordered {name: oracle region} with edges on and around the tile edges
  and inside the row-end window [n_col - VEC, n_col)."""
  T, V, n = tile, vec, n_col
  cols = lat if case.layout == 'lonlat' else lon
  rows = lon if case.layout == 'lonlat' else lat

  def cs(a, b):  # column indices a..b, both inclusive, as a label slice
    return slice(float(cols[a]), float(cols[b]))

  def rsl(a, b):
    return slice(float(rows[a]), float(rows[b]))

  def region(col_spans, row_span=None):
    spans = [(max(a, 0), min(b, n - 1)) for a, b in col_spans]
    spans = [s for s in spans if s[0] <= s[1]]
    if not spans:
      return None
    c = [cs(a, b) for a, b in spans]
    c = c if len(c) > 1 else c[0]
    r = slice(None) if row_span is None else rsl(*row_span)
    if case.layout == 'latlon':
      return oreg.SliceRegion(lat_slice=r, lon_slice=c)
    return oreg.SliceRegion(lat_slice=c, lon_slice=r)

  out = {'global': oreg.SliceRegion()}
  cand = {
      # a segment from exactly k * T
      'from_T': region([(T, n - 1)]) if n > T else region([(n // 2, n - 1)]),
      # a one-column segment at the end of tile 0
      'one_col': region([(min(T - 1, n - 1), min(T - 1, n - 1))]),
      # starts at T + 1 (inside tile 1), spans tiles 1..3
      'inside': region([(T + 1, 3 * T + 1)]),
      # spans tiles 0..3 from column 1
      'wide': region([(1, 3 * T + 1)]),
      # the row-end window: columns loaded by two lanes, the last alone
      'tail': region([(n - V + 1, n - 1)]),
      'last': region([(n - 1, n - 1)]),
      # three and more segments inside tile 0, one of multiplicity 2
      'multi': region([(2, 2), (4, 6), (5, 9)]),
      # a box of rows: bands cut the row chunks
      'box': region([(T - 1, T + 1)], (min(1, n_row - 1),
                                       max(n_row - 2, min(1, n_row - 1)))),
  }
  out.update({k: v for k, v in cand.items() if v is not None})
  out['extratropics'] = oreg.ExtraTropicalRegion()
  if case.field is not None:
    mask = NA(land_mask(case.field, lat, lon), ('latitude', 'longitude'))
    out['land'] = oreg.LandRegion(mask, lat, lon)
    sl = region([(T - 1, n - 1)]) or region([(0, n - 1)])
    out['land_cols'] = oreg.CombinedRegion(
        [sl, oreg.LandRegion(mask, lat, lon)])
  return out


@dataclasses.dataclass
class Resolved:
  case: Case
  vec: int       # wide lane width of the launch
  tile: int      # 64 * vec
  n_row: int
  n_col: int
  lat: np.ndarray
  lon: np.ndarray
  regions: dict  # oracle regions


def resolve(lib, case: Case) -> Resolved:
  vec = lib_vec(lib, case)
  tile = 64 * vec
  n_col = n_col_of(case.n_col, vec, tile)
  lat, lon = coords(case.n_row, n_col, case.layout)
  return Resolved(case, vec, tile, case.n_row, n_col, lat, lon,
                  regions(case, case.n_row, n_col, vec, tile, lat, lon))


def launch_vec(res: Resolved) -> int:
  """Columns per lane of the actual launch (1 when n_col < VEC)."""
  return res.vec if res.n_col >= res.vec else 1
