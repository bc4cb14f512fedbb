"""Seeded cases of the resampling fixtures: shared by the generator
(tests/golden/make_resample_vectors.py, which runs the reference on them) and
by the tests (which rebuild the same inputs from the seed).

A case is {'vars': {name: (dims, array)}, 'coords': {name: 1-D array},
'time_dim', 'method', 'period', 'label_side', 'add_mean_suffix', 'stats':
{'mean' | 'min' | 'max' | 'sum': [variable names]}}.  Every case is run with
`skipna` off and on (MODES).  Each holds a few kB.
"""
import numpy as np

GOLDEN_STEM = 'reference_resample_v1'
MODES = {'keepna': False, 'skipna': True}
STATS = ('mean', 'min', 'max', 'sum')
# the reference's own test (scripts/resample_in_time_test.py:119-127)
KNOWN_COMBINATIONS = ((20, '3d', None), (21, '3d', None), (21, '8d', None),
                      (5, '1d', None), (20, '3d', [0, 4, 8]),
                      (21, '3d', [20]), (21, '8d', [15]))
KNOWN_SEED = 802701


def time_axis(start: str, step_hours: int, n: int, drop=()) -> np.ndarray:
  idx = np.array([i for i in range(n) if i not in set(drop)])
  return (np.datetime64(start, 'ns')
          + idx * np.timedelta64(step_hours * 3600 * 10**9, 'ns'))


def _coords(sizes: dict, times: np.ndarray, time_dim: str) -> dict:
  out = {}
  for d, n in sizes.items():
    if d == time_dim:
      out[d] = times
    elif d == 'time':
      out[d] = time_axis('2020-01-01T00', 12, n)
    elif d == 'latitude':
      out[d] = np.linspace(-90, 90, n)
    elif d == 'longitude':
      out[d] = np.arange(n) * (360.0 / n)
    else:
      out[d] = np.arange(n)
  return out


def _case(seed, variables, sizes, times, method, period, label_side='left',
          stats=None, add_mean_suffix=False, time_dim='time'):
  assert sizes[time_dim] == len(times)
  with_time = [k for k, (d, _) in variables.items() if time_dim in d]
  stats = stats or {s: list(with_time) for s in STATS}
  return {'seed': seed, 'vars': variables,
          'coords': _coords(sizes, times, time_dim), 'time_dim': time_dim,
          'method': method, 'period': period, 'label_side': label_side,
          'add_mean_suffix': add_mean_suffix,
          'stats': {s: list(stats.get(s, [])) for s in STATS}}


def _first(seed=71):
  """Time first, float32 of mixed sign, a small-integer variable and one
  without time; 3-hourly from 15:00, so the first daily bin is short (3 of 8),
  and the last one too (2)."""
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
  stats = {'mean': ['temperature', 'counts'], 'min': ['temperature'],
           'max': ['temperature', 'counts'], 'sum': ['counts', 'temperature']}
  return _case(seed, variables, sizes, time_axis('2020-01-01T15', 3, 37),
               'resample', '1d', stats=stats, add_mean_suffix=True)


def _middle(seed=72):
  """Time in the middle, float64, hourly into 6 h, labelled on the right."""
  rs = np.random.RandomState(seed)
  sizes = {'member': 3, 'time': 50, 'latitude': 4, 'longitude': 6}
  x = rs.standard_normal(tuple(sizes.values())) * 5 + 270
  return _case(seed, {'temperature': (tuple(sizes), x)}, sizes,
               time_axis('2020-03-01T02', 1, 50), 'resample', '6h', 'right')


def _innermost(seed=73):
  """Time innermost, 3-hourly from 21:00 into 30 h (a period that does not
  divide the day)."""
  rs = np.random.RandomState(seed)
  sizes = {'latitude': 6, 'longitude': 7, 'time': 41}
  x = (rs.standard_normal(tuple(sizes.values())) * 3).astype(np.float32)
  return _case(seed, {'wind': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T21', 3, 41), 'resample', '30h')


def _nan_patterns(seed, dtype, label_side):
  """6-hourly into days: a NaN in one point only (3), NaN patches with
  different valid counts in adjacent points (4 .. 9), an all-NaN series (10),
  one all-NaN bin (11), +inf and -inf in separate bins (12), both in one bin
  (13), NaN with an infinity (14), zeros of both signs (15, 16)."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 22, 'point': 20}
  x = (rs.standard_normal(tuple(sizes.values())) * 4).astype(dtype)
  x[7, 3] = np.nan
  for k, p in enumerate(range(4, 10)):
    x[rs.permutation(22)[:2 * k + 1], p] = np.nan
  x[:, 10] = np.nan
  x[4:8, 11] = np.nan
  x[1, 12], x[9, 12] = np.inf, -np.inf
  x[4, 13], x[6, 13] = np.inf, -np.inf
  x[12, 14], x[13, 14] = np.nan, np.inf
  x[0:4, 15] = -0.0
  x[:, 16] = np.where(np.arange(22) % 2, 0.0, -0.0).astype(dtype)
  return _case(seed, {'field': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T00', 6, 22), 'resample', '1d', label_side)


def _gap(seed, label_side):
  """6-hourly with a gap of three days: two empty daily bins."""
  rs = np.random.RandomState(seed)
  times = time_axis('2020-01-01T06', 6, 40, drop=range(9, 20))
  sizes = {'time': len(times), 'point': 7}
  x = (rs.standard_normal(tuple(sizes.values())) * 2).astype(np.float32)
  return _case(seed, {'field': (tuple(sizes), x)}, sizes, times, 'resample',
               '1d', label_side)


def _single_bin(seed=78):
  rs = np.random.RandomState(seed)
  sizes = {'time': 5, 'point': 11}
  x = rs.standard_normal(tuple(sizes.values()))
  return _case(seed, {'field': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-06T00', 24, 5), 'resample', '1w')


def _length_one(seed=79):
  """The period is the spacing: every bin holds one sample."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 9, 'point': 6}
  x = rs.standard_normal(tuple(sizes.values())).astype(np.float32)
  x[2, 1] = np.nan
  x[3, 2] = -0.0
  return _case(seed, {'field': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T00', 6, 9), 'resample', '6h')


def _three_day(seed=80):
  rs = np.random.RandomState(seed)
  sizes = {'time': 20, 'level': 2, 'point': 5}
  x = (rs.standard_normal(tuple(sizes.values())) + 3).astype(np.float32)
  return _case(seed, {'field': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T00', 24, 20), 'resample', '3d', 'right')


def _weekly(seed=81):
  """6-hourly into weeks of 28 samples (the averaged-forecast evaluations)."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 60, 'latitude': 3, 'longitude': 4}
  x = (rs.standard_normal(tuple(sizes.values())) * 8 + 280).astype(np.float32)
  return _case(seed, {'temperature': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T00', 6, 60), 'resample', '1w')


def _lead(seed=82):
  """A timedelta axis (prediction_timedelta) in the middle."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 2, 'prediction_timedelta': 13, 'point': 9}
  x = rs.gamma(0.5, 4e-3, size=tuple(sizes.values())).astype(np.float32)
  leads = np.arange(13) * np.timedelta64(6 * 3600 * 10**9, 'ns')
  return _case(seed, {'precip': (tuple(sizes), x)}, sizes, leads, 'resample',
               '1d', time_dim='prediction_timedelta')


def _rolling(seed, period, label_side='left', axis_last=False):
  """12 6-hourly times; w = period / 6 h.  A NaN at (5, point 2)."""
  rs = np.random.RandomState(seed)
  sizes = {'time': 12, 'point': 10}
  x = (rs.standard_normal(tuple(sizes.values())) * 3).astype(np.float32)
  x[5, 2] = np.nan
  x[3, 4] = np.inf
  if axis_last:
    sizes = {'point': 10, 'time': 12}
    x = np.ascontiguousarray(x.T)
  return _case(seed, {'field': (tuple(sizes), x)}, sizes,
               time_axis('2020-01-01T00', 6, 12), 'rolling', period, label_side)


def known_ten_days(insert_nan: bool, method: str):
  """resample_in_time_test.py:30-117: ten days, period 3d, mean of ALL."""
  times = np.array(['2023-01-%02d' % d for d in range(1, 11)],
                   dtype='datetime64[ns]')
  temperatures = np.arange(len(times)).astype(float)
  if insert_nan:
    temperatures[0] = np.nan
  return _case(0, {'temperature': (('time',), temperatures)},
               {'time': len(times)}, times, method, '3d',
               stats={'mean': ['temperature']})


def known_combination(k: int, method: str):
  """resample_in_time_test.py:119-189."""
  n_times, period, nan_locations = KNOWN_COMBINATIONS[k]
  times = (np.datetime64('2010-01-01', 'ns')
           + np.arange(n_times) * np.timedelta64(86400 * 10**9, 'ns'))
  temperatures = np.random.RandomState(KNOWN_SEED).rand(n_times)
  for i in nan_locations or []:
    temperatures[i] = np.nan
  return _case(KNOWN_SEED, {'temperature': (('time',), temperatures)},
               {'time': n_times}, times, method, period,
               stats={'mean': ['temperature']})


def cases() -> dict:
  """{case name: builder}."""
  return {
      'first_f32': _first,
      'middle_f64': _middle,
      'innermost_f32': _innermost,
      'nan_f32': lambda: _nan_patterns(74, np.float32, 'left'),
      'nan_f64': lambda: _nan_patterns(75, np.float64, 'right'),
      'gap_left': lambda: _gap(76, 'left'),
      'gap_right': lambda: _gap(77, 'right'),
      'single_bin': _single_bin,
      'length_one': _length_one,
      'three_day': _three_day,
      'weekly': _weekly,
      'lead': _lead,
      'rolling_1': lambda: _rolling(83, '6h'),
      'rolling_4': lambda: _rolling(84, '1d', 'right'),
      'rolling_7': lambda: _rolling(85, '42h', axis_last=True),
      'rolling_all': lambda: _rolling(86, '72h'),
  }


def known_cases() -> dict:
  out = {}
  for method in ('resample', 'rolling'):
    for nan in (False, True):
      out[f'known_ten_{"nan" if nan else "clean"}_{method}'] = (
          lambda nan=nan, method=method: known_ten_days(nan, method))
    for k in range(len(KNOWN_COMBINATIONS)):
      out[f'known_{k}_{method}'] = (
          lambda k=k, method=method: known_combination(k, method))
  return out


def all_cases() -> dict:
  return {**cases(), **known_cases()}


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
