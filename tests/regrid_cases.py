"""Seeded cases of the regridding fixtures: shared by the generator
(tests/golden/make_regrid_vectors.py, which runs the reference on them) and by
the tests (which rebuild the same inputs from the seed).

A case is {'source': grid spec, 'target': grid spec, 'field': float64 array of
(..., lon, lat), 'seed', 'nan' (whether the field holds NaN)}; a grid spec is
the keyword arguments of `Grid`.  The grids are small and each case exists
because of a way the kernels can go wrong (see `cases`).  The field's values
are float32 numbers held as float64, so the float32 run of a test reads the
very same values as the float64 reference.
"""
import numpy as np

CLASSES = ('NearestRegridder', 'BilinearRegridder', 'ConservativeRegridder')
LABELS = {'NearestRegridder': 'nearest', 'BilinearRegridder': 'bilinear',
          'ConservativeRegridder': 'conservative'}
GOLDEN_STEM = 'reference_regrid_v1'
TIE_GAP = 1e-9  # radians between the nearest and the second-nearest node


def lon_values(scheme: str, num: int) -> np.ndarray:
  delta = 360 / num
  if scheme == 'START_AT_ZERO':
    return np.linspace(0, 360 - delta, num=num)
  return np.linspace(-180 + delta / 2, 180 - delta / 2, num=num)


def lat_values(poles: bool, num: int) -> np.ndarray:
  if poles:
    return np.linspace(-90, 90, num=num)
  return np.linspace(-90 + 0.5 * 180 / num, 90 - 0.5 * 180 / num, num=num)


def spec(n_lon, n_lat, poles, scheme='START_AT_ZERO', periodic=True) -> dict:
  return dict(longitudes=lon_values(scheme, n_lon),
              latitudes=lat_values(poles, n_lat), periodic=periodic,
              includes_poles=poles)


def make_grid(module, grid_spec: dict):
  return module.Grid(**grid_spec)


def _custom_lat(rs, n) -> np.ndarray:
  """Gaussian-like: equiangular nodes moved by up to a fifth of the spacing."""
  base = np.linspace(-87.5, 87.5, n)
  step = base[1] - base[0]
  return base + (rs.random_sample(n) - 0.5) * 0.4 * step


def _field(rs, shape) -> np.ndarray:
  """Smooth + noise, some hundreds in size (a temperature in K), as float32
  numbers in float64."""
  lon = np.linspace(0, 2 * np.pi, shape[-2], endpoint=False)[:, None]
  lat = np.linspace(-1, 1, shape[-1])[None, :]
  smooth = 280 + 30 * np.cos(lat * 1.4) + 8 * np.sin(2 * lon + lat)
  noise = rs.standard_normal(shape) * 3
  return (smooth + noise).astype(np.float32).astype(np.float64)


def _case(seed, source, target, lead=(), nan=None) -> dict:
  rs = np.random.RandomState(seed)
  n_lon, n_lat = len(source['longitudes']), len(source['latitudes'])
  field = _field(rs, tuple(lead) + (n_lon, n_lat))
  if nan is not None:
    field = nan(field, source)
  return {'seed': seed, 'source': source, 'target': target, 'field': field,
          'nan': nan is not None}


def _nan_patches(field, source) -> np.ndarray:
  """A NaN disc around (lon 180, lat 0) of a quarter of the globe's width, as
  the reference's own NaN test draws it, plus the whole footprint of the
  target cell (lon index 3, lat index 7) of the 20 x 11 target, 45 .. 63
  degrees east and 27 .. 45 degrees north: the source nodes at 45 .. 60 and
  30 .. 45 degrees."""
  lat = np.deg2rad(source['latitudes'])[None, :]
  lon = np.deg2rad(source['longitudes'])[:, None]
  out = np.where(lat ** 2 + (lon - np.pi) ** 2 < (np.pi / 4) ** 2, np.nan,
                 field)
  lo, la = source['longitudes'], source['latitudes']
  out[np.ix_((lo >= 44) & (lo <= 64), (la >= 26) & (la <= 46))] = np.nan
  return out


def cases() -> dict:
  """{case name: builder}."""
  def custom():
    rs = np.random.RandomState(41)
    src = dict(longitudes=lon_values('START_AT_ZERO', 50),
               latitudes=_custom_lat(rs, 23), periodic=True,
               includes_poles=False)
    tgt = dict(longitudes=lon_values('START_AT_ZERO', 21),
               latitudes=_custom_lat(rs, 10), periodic=True,
               includes_poles=False)
    return _case(42, src, tgt)

  def uncovered():
    # the target reaches beyond the source on every side; no target node lies
    # midway between two source nodes
    src = dict(longitudes=10 + 4.0 * np.arange(12),
               latitudes=-20 + 5.0 * np.arange(9), periodic=False,
               includes_poles=False)
    tgt = dict(longitudes=3 + 9.3 * np.arange(6),
               latitudes=-29 + 10.7 * np.arange(6), periodic=False,
               includes_poles=False)
    return _case(43, src, tgt)

  return {
      # plain bands, pole rows
      'global': lambda: _case(40, spec(48, 25, True), spec(20, 11, True)),
      # the longitude band of target 0 wraps, phase alignment, mixed poles
      'wrap': lambda: _case(41, spec(48, 24, False),
                            spec(20, 11, True, 'CENTER_AT_ZERO')),
      # band lengths that differ per row
      'custom_lat': custom,
      # NaN rows and columns from the coverage rule
      'uncovered': uncovered,
      # bands of 1-2 entries, rows bound by output
      'upsample': lambda: _case(44, spec(21, 10, False), spec(50, 23, False)),
      # the weights are the unit matrix
      'identity': lambda: _case(45, spec(20, 11, True), spec(20, 11, True)),
      # nanmean, 0 / 0
      'nan_patches': lambda: _case(46, spec(48, 25, True), spec(20, 11, True),
                                   nan=_nan_patches),
      # slab counting: leading dims (), (1,), (3, 2)
      'batch': lambda: _case(47, spec(48, 25, True), spec(20, 11, True),
                             lead=(3, 2)),
  }


BATCH_LEADS = ((), (1,), (3, 2))


def batch_view(field: np.ndarray, lead: tuple) -> np.ndarray:
  """The `batch` case's field with the leading dims `lead`."""
  if lead == ():
    return field[0, 0]
  if lead == (1,):
    return field[:1, 1]
  return field


# The reference's known-answer tests (regridding_test.py:313-330, 495-591,
# 593-618) as data: (class, source spec, target spec, field, expected, atol;
# expected None = "every value is finite").
def known_answers() -> dict:
  f = np.array
  g = lambda lon, lat, periodic, poles: dict(
      longitudes=f(lon), latitudes=f(lat), periodic=periodic,
      includes_poles=poles)
  nan = np.nan
  out = {
      'extrapolation': (
          'ConservativeRegridder', g([1, 3, 5], [1, 3], False, False),
          g([0, 2, 4], [0, 2], False, False), f([[1, 1], [2, 2], [3, 3]]),
          f([[nan, nan], [nan, 1.5], [nan, 2.5]])),
      'bilinear_periodic': (
          'BilinearRegridder', g([0., 90., 180., 270.], [0], True, True),
          g([45., 135., 225., 315.], [0], True, True),
          f([[0.], [1.], [2.], [3.]]), f([[.5], [1.5], [2.5], [1.5]])),
      'bilinear_not_periodic': (
          'BilinearRegridder', g([0., 90., 180., 270.], [0], False, True),
          g([45., 135., 225., 315.], [0], False, True),
          f([[0.], [1.], [2.], [3.]]), f([[.5], [1.5], [2.5], [nan]])),
      'bilinear_poles_down': (
          'BilinearRegridder', g([0.], [-90., -30., 30., 90.], True, True),
          g([0.], [-60., 0., 60.], True, True), f([[0., 1., 2., 3.]]),
          f([[.5, 1.5, 2.5]])),
      'bilinear_poles_up': (
          'BilinearRegridder', g([0.], [-60., 0., 60.], True, True),
          g([0.], [-90., -30., 30., 90.], True, True), f([[0., 1., 2.]]),
          f([[0., .5, 1.5, 2.]])),
      'bilinear_no_poles': (
          'BilinearRegridder', g([0.], [-60., -20., 20., 60.], True, False),
          g([0.], [-70., 0., 70.], True, False), f([[0., 1., 2., 3.]]),
          f([[nan, 1.5, nan]])),
      'nearest_exact': (
          'NearestRegridder', g([0, 90, 180, 270], [-30, 0, 30], True, True),
          g([0, 180], [-30, 0, 30], True, True),
          f([[0, 1, 2], [4, 5, 6], [7, 8, 9], [10, 11, 12]]),
          f([[0, 1, 2], [7, 8, 9]])),
      'quarter_degree': (
          'ConservativeRegridder', g([0., 1.], [31., 31.25, 31.5], False,
                                     False),
          g([0., 1.], [31., 31.25, 31.5], False, False), np.ones((2, 3)),
          None),
  }
  return out


KNOWN_ATOL = 1e-6

# regridding_test.py:252-311 and :273-283, through the private helpers
LATITUDE_WEIGHTS = dict(
    source=np.array([-75, -45, -15, 15, 45, 75]), target=np.array([-45, 45]),
    expected=np.array([
        [1 - np.sqrt(3) / 2, (np.sqrt(3) - 1) / 2, 1 / 2, 0, 0, 0],
        [0, 0, 0, 1 / 2, (np.sqrt(3) - 1) / 2, 1 - np.sqrt(3) / 2]]))
LONGITUDE_WEIGHTS = (
    dict(source=np.array([0, 60, 120, 180, 240, 300]),
         target=np.array([0, 90, 180, 270]),
         expected=np.array([[4, 1, 0, 0, 0, 1], [0, 3, 3, 0, 0, 0],
                            [0, 0, 1, 4, 1, 0], [0, 0, 0, 0, 3, 3]]) / 6),
    dict(source=np.array([90, 180, 270, 360]),
         target=np.array([-270, -180, -90, 0]), expected=np.eye(4)),
)
ALIGN_PHASE = ((1, 0, 1), (-1, 0, -1), (5, 0, 5), (6, 0, -4), (1, 9, 11),
               (5, 9, 5))


def structure(module) -> dict:
  """Names of the public surface: classes, Grid's fields, enum members."""
  import dataclasses
  return {
      'classes': [n for n in ('Grid', 'Regridder') + CLASSES
                  if hasattr(module, n)],
      'grid_fields': [[f.name, bool(f.kw_only)]
                      for f in dataclasses.fields(module.Grid)],
      'regridder_fields': [f.name for f in
                           dataclasses.fields(module.Regridder)],
      'LongitudeScheme': [m.name for m in module.LongitudeScheme],
      'LatitudeSpacing': [m.name for m in module.LatitudeSpacing],
      'functions': [n for n in ('latitude_values', 'longitude_values',
                                '_align_phase_with',
                                '_conservative_latitude_weights',
                                '_conservative_longitude_weights')
                    if callable(getattr(module, n, None))],
      'subclasses': [n for n in CLASSES
                     if issubclass(getattr(module, n), module.Regridder)],
  }


def tie_rows_and_columns(source: dict, target: dict) -> tuple:
  """Where an exact geometric tie of the nearest neighbour is expected:
  (target longitude indices, target latitude indices).  Pole rows of the
  target (every longitude is equally far), target nodes exactly midway between
  two neighbouring source nodes of one axis."""
  def midway(src, tgt, period):
    src = np.asarray(src, dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)
    mids = (src[:-1] + src[1:]) / 2
    if period:
      mids = np.concatenate([mids, [(src[-1] + src[0] + period) / 2]])
      d = np.abs((tgt[:, None] - mids[None, :] + period / 2) % period
                 - period / 2)
    else:
      d = np.abs(tgt[:, None] - mids[None, :])
    return set(np.flatnonzero((d < 1e-9).any(axis=1)).tolist())
  lat = np.asarray(target['latitudes'], dtype=np.float64)
  rows = set(np.flatnonzero(np.abs(np.abs(lat) - 90) < 1e-9).tolist())
  rows |= midway(source['latitudes'], lat, None)
  cols = midway(source['longitudes'], target['longitudes'],
                360 if source['periodic'] else None)
  return cols, rows


def golden_paths(directory: str) -> list:
  import glob
  import os
  return sorted(glob.glob(os.path.join(directory, GOLDEN_STEM + '.*.npz')))


def load_golden(directory: str) -> dict:
  """Every array of every shard, by its key."""
  out = {}
  for path in golden_paths(directory):
    with np.load(path) as z:
      for k in z.files:
        assert k not in out, k
        out[k] = z[k]
  return out
