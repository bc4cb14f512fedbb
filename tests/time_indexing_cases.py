"""Seeded cases of the time re-indexing fixtures: shared by the generator
(tests/golden/make_time_indexing_vectors.py, which runs the reference on them)
and by the tests (which rebuild the same inputs from the seed).

Four families, each `{name: builder}`:
  sampler   keyword arguments of `get_sampled_init_times` ('output_times' is a
            datetime64[ns] array)
  expand    {'vars': {name: (dims, array)}, 'coords', 'times'}
  index     {'vars', 'coords', 'mode'}
  ensemble  {'vars', 'coords', 'kwargs'}: the keyword arguments of
            `probabilistic_climatological_forecasts`
`known_*` are the inputs of the reference's own tests (on a smaller grid where
theirs is large).
"""
import glob
import itertools
import os

import numpy as np

GOLDEN_STEM = 'reference_time_indexing_v1'
EDGES = ('WRAP_YEAR', 'NO_EDGE', 'REFLECT_RANGE')
HOUR = np.timedelta64(3600 * 10**9, 'ns')


def time_axis(start: str, step_hours: int, n: int) -> np.ndarray:
  return np.datetime64(start, 'ns') + np.arange(n) * (step_hours * HOUR)


def time_range(start: str, stop: str, step_hours: int) -> np.ndarray:
  """`start` .. `stop`, both inclusive."""
  first, last = np.datetime64(start, 'ns'), np.datetime64(stop, 'ns')
  return first + np.arange((last - first) // (step_hours * HOUR) + 1) * (
      step_hours * HOUR)


def lead_axis(start_hours: int, step_hours: int, n: int) -> np.ndarray:
  return (start_hours + np.arange(n) * step_hours) * HOUR


def _grid(n_lat: int, n_lon: int) -> dict:
  return {'latitude': np.linspace(-90, 90, n_lat),
          'longitude': np.arange(n_lon) * (360.0 / n_lon)}


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def _sampler(output_times, **kw):
  base = dict(output_times=output_times, climatology_start_year=2012,
              climatology_end_year=2021, day_window_size=15, ensemble_size=3,
              with_replacement=True, sample_hold_days=0,
              initial_time_edge_behavior='WRAP_YEAR',
              leave_out_if_in_climatology=False, num_years_to_exclude=1,
              seed=802701)
  base.update(kw)
  return base


def sampler_cases() -> dict:
  """The 24 combinations of edge behaviour, replacement, hold and leave-out
  on 12-hourly output times that cross a year end (2019 -> 2020, inside the
  climatology years, so leaving out bites); the same across a leap day;
  `ensemble_size = -1`; the reference test's own arguments."""
  cases = {}
  year_end = time_axis('2019-12-29T00', 12, 10)
  leap_day = time_axis('2020-02-27T12', 12, 8)
  for k, (edge, repl, hold, leave) in enumerate(itertools.product(
      EDGES, (True, False), (0, 2), (False, True))):
    name = f'combo_{edge.lower()}_{"repl" if repl else "norepl"}_hold{hold}' \
           f'_{"leave" if leave else "all"}'
    cases[name] = lambda e=edge, r=repl, h=hold, l=leave, k=k: _sampler(
        year_end, initial_time_edge_behavior=e, with_replacement=r,
        sample_hold_days=h, leave_out_if_in_climatology=l, seed=1000 + k)
  for edge in EDGES:
    cases[f'leap_{edge.lower()}'] = lambda e=edge: _sampler(
        leap_day, initial_time_edge_behavior=e, day_window_size=40,
        ensemble_size=5, seed=17)
    cases[f'all_{edge.lower()}'] = lambda e=edge: _sampler(
        year_end[:4], initial_time_edge_behavior=e, ensemble_size=-1,
        day_window_size=4, climatology_start_year=2018,
        climatology_end_year=2020, with_replacement=False, seed=5)
  cases['all_with_replacement'] = lambda: _sampler(
      leap_day, ensemble_size=-1, day_window_size=3,
      climatology_start_year=2019, climatology_end_year=2020, seed=6)
  cases['window_one_daily'] = lambda: _sampler(
      time_axis('2020-12-30T06', 24, 5), day_window_size=1, ensemble_size=2,
      sample_hold_days=2, seed=7)
  # compute_probabilistic_climatological_forecasts_test.py:
  # test_leave_out_climatology_true_behavior (excluding one further year and
  # none), test_sample_statistics_no_hold_time, ..._with_hold_time
  for exclude in (1, 0):
    cases[f'known_leave_out_{exclude}'] = lambda n=exclude: _sampler(
        np.array(['2005-06-15T12:00:00'], dtype='datetime64[ns]'),
        climatology_start_year=2000, climatology_end_year=2010,
        day_window_size=5, ensemble_size=100, leave_out_if_in_climatology=True,
        num_years_to_exclude=n, seed=12345)
  no_hold = np.array(['1990-01-02T12', '1995-06-01T00', '2000-12-30T07'],
                     dtype='datetime64[ns]')
  for edge, repl, size in (('REFLECT_RANGE', True, 200), ('NO_EDGE', True, 200),
                           ('WRAP_YEAR', True, 200), ('WRAP_YEAR', False, 50),
                           ('WRAP_YEAR', True, -1), ('WRAP_YEAR', False, -1),
                           ('REFLECT_RANGE', False, -1),
                           ('NO_EDGE', False, -1)):
    name = f'known_no_hold_{edge.lower()}_{"repl" if repl else "norepl"}' \
           f'_{"all" if size < 0 else size}'
    cases[name] = lambda e=edge, r=repl, s=size: _sampler(
        no_hold, climatology_start_year=1990, climatology_end_year=2001,
        day_window_size=6, ensemble_size=s, with_replacement=r,
        initial_time_edge_behavior=e, num_years_to_exclude=0, seed=802701)
  with_hold = time_range('2021-01-01', '2025-01-01', 240)
  for edge, repl, size in itertools.product(EDGES, (False, True), (-1, 10)):
    name = f'known_hold_{edge.lower()}_{"repl" if repl else "norepl"}' \
           f'_{"all" if size < 0 else size}'
    cases[name] = lambda e=edge, r=repl, s=size: _sampler(
        with_hold, climatology_start_year=1990, climatology_end_year=2000,
        day_window_size=5, ensemble_size=s, with_replacement=r,
        sample_hold_days=30, initial_time_edge_behavior=e,
        num_years_to_exclude=0, seed=802701)
  return cases


# ---------------------------------------------------------------------------
# expand_climatology
# ---------------------------------------------------------------------------
def _expand_hourly(seed=81):
  """6-hourly, float32 3-D and float64 2-D variables, the times cross a year
  end and a leap day."""
  rs = np.random.RandomState(seed)
  coords = dict({'hour': np.arange(0, 24, 6), 'dayofyear': 1 + np.arange(366),
                 'level': np.array([500, 850])}, **_grid(3, 4))
  d3 = ('hour', 'dayofyear', 'level', 'longitude', 'latitude')
  d2 = ('hour', 'dayofyear', 'longitude', 'latitude')
  variables = {
      'temperature': (d3, rs.standard_normal((4, 366, 2, 4, 3)
                                             ).astype(np.float32)),
      '2m_temperature': (d2, rs.standard_normal((4, 366, 4, 3)))}
  return {'seed': seed, 'vars': variables, 'coords': coords,
          'times': time_range('2019-12-30T00', '2020-03-02T18', 6)}


def _expand_daily(seed=82):
  """No `hour` coordinate; `dayofyear` first, in the middle and before one dim
  only; integers; a variable without it."""
  rs = np.random.RandomState(seed)
  coords = dict({'dayofyear': 1 + np.arange(366), 'level': np.arange(3)},
                **_grid(5, 6))
  variables = {
      'surface': (('dayofyear', 'latitude', 'longitude'),
                  rs.standard_normal((366, 5, 6)).astype(np.float32)),
      'column': (('level', 'dayofyear', 'latitude', 'longitude'),
                 rs.standard_normal((3, 366, 5, 6))),
      'zonal': (('latitude', 'dayofyear'), rs.standard_normal((5, 366))),
      'counts': (('dayofyear', 'latitude', 'longitude'),
                 rs.randint(-9, 9, size=(366, 5, 6)).astype(np.int32)),
      'orography': (('latitude', 'longitude'), rs.standard_normal((5, 6)))}
  return {'seed': seed, 'vars': variables, 'coords': coords,
          'times': time_range('2020-12-25', '2021-01-05', 24)}


def _expand_two_hours(seed=83):
  """2 hours x 366 days x 2 levels on an 8 x 16 grid, times out of order and
  repeated."""
  rs = np.random.RandomState(seed)
  coords = dict({'hour': np.array([0, 12]), 'dayofyear': 1 + np.arange(366),
                 'level': np.array([500, 850])}, **_grid(8, 16))
  dims = ('hour', 'dayofyear', 'level', 'latitude', 'longitude')
  x = rs.standard_normal((2, 366, 2, 8, 16)).astype(np.float32)
  x[1, 59, 0, 2, 3] = np.nan
  x[0, 365, 1, 0, 0] = np.inf
  times = time_range('2024-02-27T00', '2024-03-03T12', 12)
  times = np.concatenate([times[::-1], times[:3],
                          time_axis('2023-12-31T12', 12, 2)])
  return {'seed': seed, 'vars': {'geopotential': (dims, x)}, 'coords': coords,
          'times': times}


def _known_expand(seed=0):
  """expand_climatology_test.py: a 6-hourly climatology of normal(seed 0)
  values onto 2019-12-01 .. 2020-03-30 every 6 hours (on a 3 x 2 grid)."""
  rs = np.random.RandomState(seed)
  coords = dict({'hour': np.arange(0, 24, 6), 'dayofyear': 1 + np.arange(366),
                 'level': np.array([500, 700])}, **_grid(2, 3))
  d3 = ('hour', 'dayofyear', 'level', 'longitude', 'latitude')
  d2 = ('hour', 'dayofyear', 'longitude', 'latitude')
  variables = {}
  for name, dims in (('geopotential', d3), ('temperature', d3),
                     ('2m_temperature', d2)):
    shape = tuple(len(coords[d]) for d in dims)
    variables[name] = (dims, rs.normal(size=shape))
  return {'seed': seed, 'vars': variables, 'coords': coords,
          'times': time_range('2019-12-01', '2020-03-30', 6)}


def expand_cases() -> dict:
  return {'expand_hourly': _expand_hourly, 'expand_daily': _expand_daily,
          'expand_two_hours': _expand_two_hours, 'known_expand': _known_expand}


# ---------------------------------------------------------------------------
# index_on_valid_time
# ---------------------------------------------------------------------------
def _known_index(offset: bool, mode: str):
  """index_on_valid_time_test.py: 4 inits every 12 h, leads every 6 h from 0 h
  or from 6 h, integers."""
  foo = np.arange(1, 21).reshape(4, 5)
  leads = lead_axis(0, 6, 5)
  if offset:
    foo, leads = foo[:, 1:], leads[1:]
  return {'seed': 0, 'mode': mode,
          'vars': {'foo': (('time', 'prediction_timedelta'), foo)},
          'coords': {'time': time_axis('2000-01-01T00', 12, 4),
                     'prediction_timedelta': leads}}


KNOWN_INDEX_ANSWERS = {
    'known_index_zero_delta': [[1, np.nan, np.nan], [6, 3, np.nan], [11, 8, 5],
                               [16, 13, 10], [np.nan, 18, 15],
                               [np.nan, np.nan, 20]],
    'known_index_offset_delta': [[3, np.nan], [8, 5], [13, 10], [18, 15],
                                 [np.nan, 20]],
}


def _index_grid(mode: str, seed=91):
  """6 inits every 12 h x 5 leads every 6 h x 2 levels on an 8 x 16 grid,
  float64 with values float32 cannot hold, and a float32 variable whose dims
  come in another order."""
  rs = np.random.RandomState(seed)
  coords = dict({'time': time_axis('2020-02-28T00', 12, 6),
                 'prediction_timedelta': lead_axis(0, 6, 5),
                 'level': np.array([500, 850])}, **_grid(8, 16))
  x = rs.standard_normal((6, 5, 2, 8, 16)) * 1e3
  x[0, 0, 0, 0, :6] = [np.nan, np.inf, -np.inf, 1e300, -0.0, 1e-310]
  y = rs.standard_normal((2, 6, 5, 8, 16)).astype(np.float32)
  return {'seed': seed, 'mode': mode, 'coords': coords, 'vars': {
      'geopotential': (('time', 'prediction_timedelta', 'level', 'latitude',
                        'longitude'), x),
      'temperature': (('level', 'time', 'prediction_timedelta', 'latitude',
                       'longitude'), y)}}


def _index_lead_first(mode: str, seed=92):
  """The lead dim before the init dim, leads from 12 h, inits every 24 h."""
  rs = np.random.RandomState(seed)
  coords = dict({'time': time_axis('2021-06-01T06', 24, 5),
                 'prediction_timedelta': lead_axis(12, 12, 7)}, **_grid(3, 5))
  x = rs.standard_normal((7, 5, 3, 5)).astype(np.float32)
  return {'seed': seed, 'mode': mode, 'coords': coords, 'vars': {
      'wind': (('prediction_timedelta', 'time', 'latitude', 'longitude'), x)}}


def index_cases() -> dict:
  cases = {}
  for mode in ('valid_and_delta', 'valid_and_init'):
    short = mode.split('_')[-1]
    cases[f'known_index_zero_{short}'] = lambda m=mode: _known_index(False, m)
    cases[f'known_index_offset_{short}'] = lambda m=mode: _known_index(True, m)
    cases[f'index_grid_{short}'] = lambda m=mode: _index_grid(m)
    cases[f'index_lead_first_{short}'] = lambda m=mode: _index_lead_first(m)
  return cases


# ---------------------------------------------------------------------------
# the sampled climatological ensemble
# ---------------------------------------------------------------------------
def _ens_grid(seed=95):
  """3 members x 5 leads x 4 inits of 2 levels on an 8 x 16 grid, 6-hourly
  truth of 2015 .. 2018, float32, and a float64 variable with the time dim in
  the middle."""
  rs = np.random.RandomState(seed)
  times = time_range('2015-01-01T00', '2018-12-31T18', 6)
  coords = dict({'time': times, 'level': np.array([500, 850])}, **_grid(8, 16))
  x = rs.standard_normal((len(times), 2, 8, 16)).astype(np.float32)
  y = rs.standard_normal((2, len(times), 3))
  kwargs = dict(initial_time_start='2018-02-27T06',
                initial_time_end='2018-02-28T18', initial_time_spacing='12h',
                forecast_duration='1d', timedelta_spacing='6h',
                climatology_start_year=2015, climatology_end_year=2017,
                day_window_size=9, ensemble_size=3, seed=11,
                add_source_time=True)
  return {'seed': seed, 'coords': dict(coords, band=np.arange(3)),
          'kwargs': kwargs, 'vars': {
              'geopotential': (('time', 'level', 'latitude', 'longitude'), x),
              'index': (('level', 'time', 'band'), y)}}


# compute_probabilistic_climatological_forecasts_test.py, test_standard_workflow
KNOWN_ENSEMBLE = {
    'default': {},
    'hold_7d': dict(sample_hold_days=7),
    'custom_time_name': dict(time_dim='init', add_source_time=False),
    'odd_window_no_edge': dict(day_window_size=3,
                               initial_time_edge_behavior='NO_EDGE'),
    'leap_feb_reflect': dict(leap='feb',
                             initial_time_edge_behavior='REFLECT_RANGE'),
    'leap_dec': dict(leap='dec'),
    'data_leap': dict(data_leap=True),
    'delta_less_than_init': dict(initial_time_spacing='2d',
                                 timedelta_spacing='1d',
                                 with_replacement=False, ensemble_size=-1),
    'subday_delta_less': dict(initial_time_spacing='12h',
                              timedelta_spacing='6h', resolution_hours=6),
    'subday_delta_greater': dict(initial_time_spacing='6h',
                                 timedelta_spacing='12h', resolution_hours=6),
    'delta_greater_than_init': dict(initial_time_spacing='1d',
                                    timedelta_spacing='2d',
                                    with_replacement=False, ensemble_size=-1),
}


def _known_ensemble(leap=None, data_leap=False, resolution_hours=24,
                    time_dim='time', seed=0, **kw):
  """A truth of 1999 .. 2005 that grows by one with every lead step."""
  kwargs = dict(initial_time_spacing='1d', timedelta_spacing='1d',
                forecast_duration='3d', day_window_size=4, ensemble_size=20,
                with_replacement=True, sample_hold_days=0,
                initial_time_edge_behavior='WRAP_YEAR', add_source_time=True,
                seed=802701, time_dim=time_dim)
  kwargs.update(kw)
  start, end = {'feb': ('2004-02-25', '2004-03-01'),
                'dec': ('2004-12-25', '2005-01-05'),
                None: ('2004-01-01', '2004-01-15')}[leap]
  years = (2000, 2002) if data_leap else (2001, 2003)
  kwargs.update(initial_time_start=start, initial_time_end=end,
                climatology_start_year=years[0], climatology_end_year=years[1])
  rs = np.random.RandomState(seed)
  times = time_range('1999-01-01', '2005-01-01', resolution_hours)
  unit = {'d': 24, 'h': 1}[kwargs['timedelta_spacing'][-1]] * int(
      kwargs['timedelta_spacing'][:-1])
  field = rs.standard_normal((2, 3, 2))
  x = (field[None] + np.arange(len(times))[:, None, None, None]
       ) * (resolution_hours / unit)
  coords = dict({time_dim: times, 'level': np.array([500, 850])},
                **_grid(2, 3))
  return {'seed': seed, 'coords': coords, 'kwargs': kwargs, 'vars': {
      'temperature': ((time_dim, 'level', 'longitude', 'latitude'), x)}}


def ensemble_cases() -> dict:
  cases = {'ens_grid': _ens_grid}
  for name, kw in KNOWN_ENSEMBLE.items():
    cases[f'known_ens_{name}'] = lambda kw=kw: _known_ensemble(**kw)
  return cases


# ---------------------------------------------------------------------------
# the fixture files
# ---------------------------------------------------------------------------
def shard_of(key: str) -> str:
  """The file a fixture entry goes to: one per case, the sampler's in one."""
  family, case = key.split('/')[:2]
  return 'sampler' if family == 'sampler' else case


def golden_dir() -> str:
  return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden() -> dict:
  out = {}
  for path in sorted(glob.glob(os.path.join(golden_dir(),
                                            GOLDEN_STEM + '.*.npz'))):
    with np.load(path) as z:
      out.update({k: z[k] for k in z.files})
  return out
