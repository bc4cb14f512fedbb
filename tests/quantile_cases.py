"""Seeded cases of the quantile fixtures: shared by the generator
(tests/golden/make_quantile_vectors.py, which runs the reference on them) and
by the tests (which rebuild the same inputs from the seed).

A case is {'vars': {name: (dims, array)}, 'coords': {name: 1-D array},
'dim': the reduced dims, 'q': a list (or, with 'scalar', one number),
'name_suffix': str}.  Every case is run with `skipna` off and on (MODES).
Each holds a few thousand elements.
"""
import numpy as np

GOLDEN_STEM = 'reference_quantile_v1'
MODES = {'keepna': False, 'skipna': True}
QUANTILE = 'quantile'
# the reference's own test (scripts/compute_quantiles_test.py): the seeds are
# 802701 + the number of chunk settings of its parameter sets
KNOWN_SEEDS = (0, 2, 3, 4)
KNOWN_QUANTILES = [0.2, 0.8]


def _coords(sizes: dict) -> dict:
  out = {}
  for d, n in sizes.items():
    if d == 'time':
      out[d] = (np.arange(n) * np.timedelta64(6, 'h')
                + np.datetime64('2020-01-01T00', 'ns'))
    elif d == 'latitude':
      out[d] = np.linspace(-90, 90, n)
    elif d == 'longitude':
      out[d] = np.arange(n) * (360.0 / n)
    else:
      out[d] = np.arange(n)
  return out


def _case(seed, variables, sizes, dim, q, name_suffix='', scalar=False):
  return {'seed': seed, 'vars': variables, 'coords': _coords(sizes),
          'dim': dim, 'q': q, 'name_suffix': name_suffix, 'scalar': scalar}


def _leading(seed=51):
  """The leading axis of (time, latitude, longitude): float32 of mixed sign, a
  small-integer variable and one without the reduced dim; 37 samples, so that
  v is an exact integer for q = 0.25, 0.5 and 0.75."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 37, 'latitude': 5, 'longitude': 9}
  shape = tuple(sizes.values())
  variables = {
      'temperature': (tuple(sizes), (rs.standard_normal(shape) * 12
                                     ).astype(np.float32)),
      'counts': (tuple(sizes), rs.randint(-3, 4, size=shape).astype(np.int16)),
      'orography': (('latitude', 'longitude'),
                    rs.standard_normal(shape[1:]).astype(np.float32)),
  }
  return _case(seed, variables, sizes, 'time', [0.1, 0.25, 0.5, 0.75, 0.99],
               name_suffix='_quantile')


def _middle(seed=52):
  """A middle axis, float64 (the layout of the reference's own test)."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 3, 'lat': 41, 'timedelta': 7}
  x = rs.gamma(0.5, 4e-3, size=tuple(sizes.values()))
  return _case(seed, {'precip': (tuple(sizes), x)}, sizes, 'lat', [0.2, 0.8])


def _innermost(seed=53):
  """The innermost axis, an even count: t is exactly 0.5 for q = 0.5."""
  rs = np.random.RandomState(seed)
  sizes = {'latitude': 6, 'longitude': 7, 'time': 24}
  x = (rs.standard_normal(tuple(sizes.values())) * 3).astype(np.float32)
  return _case(seed, {'wind': (tuple(sizes), x)}, sizes, ['time'],
               [0.5, 0.0, 1.0, 0.3])


def _two_dims(seed, dim):
  rs = np.random.RandomState(seed)
  sizes = {'time': 9, 'level': 4, 'latitude': 5, 'longitude': 11}
  x = (rs.standard_normal(tuple(sizes.values())) * 5 + 270).astype(np.float32)
  return _case(seed, {'temperature': (tuple(sizes), x)}, sizes, dim,
               [0.05, 0.5, 0.95])


def _ties(seed=56):
  """Exact ties: point 0 is all equal; points 1 .. 7 are mostly exact zeros
  (precipitation) with the targets inside the run; unsorted q with
  duplicates."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 40, 'point': 12}
  x = rs.gamma(0.5, 4e-3, size=tuple(sizes.values())).astype(np.float32)
  x[:, 0] = np.float32(0.125)
  x[:, 1:8] = np.where(rs.random_sample((40, 7)) < 0.8, 0, x[:, 1:8])
  return _case(seed, {'precip': (tuple(sizes), x)}, sizes, 'time',
               [0.9, 0.1, 0.5, 0.9, 0.0, 0.75, 0.1, 1.0])


def _specials(seed, dtype):
  """Mixed signs, denormals, both zeros, +-inf.  Point 0 is (1, 2, 3, 4, +inf
  ): q = 0.75 has lo = 3, t = 0, a finite, b = +inf, which is NaN in NumPy."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 5, 'point': 24}
  info = np.finfo(dtype)
  pool = np.array([0.0, -0.0, info.smallest_subnormal,
                   -info.smallest_subnormal, info.tiny / 4, -info.tiny / 2,
                   info.tiny, 1.0, -1.0, 1.5, -2.5, info.max, -info.max,
                   np.inf, -np.inf], dtype=dtype)
  x = pool[rs.randint(0, len(pool), size=tuple(sizes.values()))]
  x[:, 0] = np.array([3, 1, np.inf, 4, 2], dtype=dtype)
  x[:, 1] = np.array([-np.inf, 0.0, -0.0, np.inf, 1], dtype=dtype)
  x[:, 2] = np.array([0.0, -0.0, -0.0, 0.0, 0.0], dtype=dtype)
  x[:, 3] = np.inf
  x[:, 4] = np.array([-np.inf, -np.inf, 1, np.inf, np.inf], dtype=dtype)
  return _case(seed, {'field': (tuple(sizes), x)}, sizes, 'time',
               [0.0, 0.25, 0.5, 0.75, 1.0, 0.6, 0.4])


def _nan_patterns(seed, dtype):
  """NaN in one point only (3), different valid counts in adjacent points
  (4 .. 9), an all-NaN point (10), a single valid sample (11), NaN together
  with infinities (12)."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 21, 'point': 20}
  x = (rs.standard_normal(tuple(sizes.values())) * 4).astype(dtype)
  x[7, 3] = np.nan
  for k, p in enumerate(range(4, 10)):
    x[rs.permutation(21)[:2 * k + 1], p] = np.nan
  x[:, 10] = np.nan
  x[:, 11] = np.nan
  x[13, 11] = 2.5
  x[[0, 5, 9], 12] = [np.nan, np.inf, -np.inf]
  return _case(seed, {'field': (tuple(sizes), x)}, sizes, 'time',
               [0.0, 0.1, 0.5, 0.9, 1.0])


def _many_quantiles(seed=61):
  """21 quantiles (more than share a streaming pass), unsorted, over a
  series longer than the resident regime holds."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 2700, 'point': 3}
  x = (rs.standard_normal(tuple(sizes.values())) * 8 + 280).astype(np.float32)
  x[rs.permutation(2700)[:40], 1] = np.nan
  q = np.linspace(0, 1, 21)[rs.permutation(21)].tolist()
  return _case(seed, {'temperature': (tuple(sizes), x)}, sizes, 'time', q)


def _scalar(seed=62):
  rs = np.random.RandomState(seed)
  sizes = {'time': 17, 'latitude': 4, 'longitude': 6}
  shape = tuple(sizes.values())
  variables = {
      'a': (tuple(sizes), rs.standard_normal(shape)),
      'b': (('latitude', 'longitude'), rs.standard_normal(shape[1:])),
  }
  return _case(seed, variables, sizes, 'time', 0.3, scalar=True)


def known(k: int, name_suffix: str = ''):
  """The inputs of the reference's own test: `rand(4, 50, 6)`, its first
  three times, dim='lat'."""
  precip = np.random.RandomState(802701 + k).rand(4, 50, 6)[:3]
  sizes = {'time': 3, 'lat': 50, 'timedelta': 6}
  case = _case(802701 + k, {'precip': (tuple(sizes), precip)}, sizes, 'lat',
               list(KNOWN_QUANTILES), name_suffix=name_suffix)
  case['coords']['time'] = np.array(
      ['2023-01-01', '2023-01-02', '2023-01-03'], dtype='datetime64[ns]')
  return case


def cases() -> dict:
  """{case name: builder}."""
  return {
      'leading_f32': _leading,
      'middle_f64': _middle,
      'innermost_f32': _innermost,
      'two_adjacent': lambda: _two_dims(54, ['time', 'level']),
      'two_split': lambda: _two_dims(55, ['latitude', 'time']),
      'ties': _ties,
      'specials_f32': lambda: _specials(57, np.float32),
      'specials_f64': lambda: _specials(58, np.float64),
      'nan_f32': lambda: _nan_patterns(59, np.float32),
      'nan_f64': lambda: _nan_patterns(60, np.float64),
      'many_quantiles': _many_quantiles,
      'scalar_q': _scalar,
  }


def known_cases() -> dict:
  out = {f'known_{k}': (lambda k=k: known(k)) for k in KNOWN_SEEDS}
  out['known_2_suffix'] = lambda: known(2, '_quantile')
  return out


def all_cases() -> dict:
  return {**cases(), **known_cases()}


def reduced_axes(case, name) -> tuple:
  """Axes of variable `name` that the case reduces (empty: passes through)."""
  dims = case['vars'][name][0]
  dim = [case['dim']] if isinstance(case['dim'], str) else list(case['dim'])
  return tuple(dims.index(d) for d in dim if d in dims)


def expected_structure(case) -> dict:
  """Output dims, dtypes and coordinate names of a case, from the rules of
  xarray's quantile (what the fixtures' `structure` entry records from the
  reference)."""
  dim = [case['dim']] if isinstance(case['dim'], str) else list(case['dim'])
  variables = {}
  for name, (dims, array) in case['vars'].items():
    if not set(dims) & set(dim):
      variables[name + case['name_suffix']] = {
          'dims': list(dims), 'dtype': array.dtype.name}
      continue
    keep = [d for d in dims if d not in dim]
    variables[name + case['name_suffix']] = {
        'dims': keep if case['scalar'] else [QUANTILE] + keep,
        'dtype': 'float64'}
  coords = sorted([c for c in case['coords'] if c not in dim] + [QUANTILE])
  return {'vars': variables, 'coords': coords, 'quantile_dtype': 'float64',
          'quantile_ndim': 0 if case['scalar'] else 1}


def shard_of(key: str) -> str:
  head = key.split('/')[0]
  return 'known' if head.startswith('known') else head


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
