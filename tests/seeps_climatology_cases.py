"""Seeded cases of the window quantile and SEEPS climatology: gamma-like
"precipitation" in metres with 30 - 60 % samples below the dry threshold, so
that thresholds exist.  The cases marked `reference` are run through the
reference's own code by tests/golden/make_seeps_climatology_vectors.py."""
import glob
import os

import numpy as np

GOLDEN_STEM = 'reference_seeps_climatology_v1'
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VAR = 'total_precipitation_24hr'
DRY_MM = 0.25
QUANTILES = (1.0, 0.0, 2 / 3, 0.2, 0.2)  # unsorted, with a duplicate


def precipitation(rng, shape, dtype=np.float32, dry=0.45, quantum=None):
  """Gamma-distributed amounts in metres; a share `dry` of them a drizzle
  below 0.25 mm, some exactly zero."""
  wet = rng.gamma(0.7, 0.006, size=shape) + DRY_MM / 1000
  drizzle = rng.uniform(0, 0.9 * DRY_MM / 1000, size=shape)
  drizzle[rng.uniform(size=shape) < 0.5] = 0.0
  x = np.where(rng.uniform(size=shape) < dry, drizzle, wet)
  if quantum:
    x = np.round(x / quantum) * quantum
  return x.astype(dtype)


def times_of(first, last, hour_interval):
  """Every `hour_interval` hours from the day `first` to the end of `last`."""
  return np.arange(np.datetime64(first, 'h'),
                   np.datetime64(last, 'h') + np.timedelta64(24, 'h'),
                   np.timedelta64(hour_interval, 'h')).astype('datetime64[ns]')


def _case(times, data, dims, *, frequency, hour_interval, window_size,
          reference=False, quantiles=QUANTILES):
  return dict(times=times, data=data, dims=tuple(dims), frequency=frequency,
              hour_interval=hour_interval, window_size=window_size,
              clim_years=slice(None, None), reference=reference,
              quantiles=tuple(quantiles))


def hourly(dtype=np.float32, n_point=5, seed=1, window_size=5, reference=False,
           dims=('time', 'point'), hour_interval=12, quantum=None):
  """2019 - 2021 (2020 is a leap year: day 366 filled from 365), two hours."""
  rng = np.random.default_rng(seed)
  times = times_of('2019-01-01', '2021-12-31', hour_interval)
  data = precipitation(rng, (times.size, n_point), dtype, quantum=quantum)
  if dims[0] != 'time':
    data = np.ascontiguousarray(data.T)
  return _case(times, data, dims, frequency='hourly',
               hour_interval=hour_interval, window_size=window_size,
               reference=reference)


def daily(dtype=np.float64, n_point=3, seed=2, window_size=5, reference=False):
  """Twelve-hourly steps, daily means first."""
  rng = np.random.default_rng(seed)
  times = times_of('2019-01-01', '2021-12-31', 12)
  data = precipitation(rng, (times.size, n_point), dtype)
  return _case(times, data, ('time', 'point'), frequency='daily',
               hour_interval=None, window_size=window_size,
               reference=reference)


def edge_data(dtype=np.float32, seed=3, reference=False):
  """NaNs in the data, a gap day, a point that is dry throughout (threshold
  NaN, dry fraction 1) and a point that is all NaN."""
  rng = np.random.default_rng(seed)
  times = times_of('2019-01-01', '2021-12-31', 24)
  data = precipitation(rng, (times.size, 6), dtype)
  data[rng.uniform(size=data.shape) < 0.05] = np.nan
  data[:, 4] = (rng.uniform(0, 0.2e-3, size=times.size)).astype(dtype)
  data[:, 5] = np.nan
  keep = np.ones(times.size, dtype=bool)
  keep[400] = False  # a gap day
  return _case(times[keep], data[keep], ('time', 'point'), frequency='hourly',
               hour_interval=24, window_size=5, reference=reference)


def long_window(dtype=np.float32, seed=4, reference=False):
  """Seven years and the script's default window of 61 days."""
  rng = np.random.default_rng(seed)
  times = times_of('2014-01-01', '2020-12-31', 24)
  data = precipitation(rng, (times.size, 3), dtype)
  return _case(times, data, ('time', 'point'), frequency='hourly',
               hour_interval=24, window_size=61, reference=reference,
               quantiles=(0.1, 2 / 3, 0.99))


def december(dtype=np.float32, n_year=3, n_point=3, seed=5, window_size=21,
             n_pos=7, quantum=None, reference=False):
  """Late-December series: `n_pos` days of year ending with day 365, so a
  window of 21 wraps three times."""
  rng = np.random.default_rng(seed)
  # (common years: each ends on day 365)
  years = [y for y in range(2001, 2001 + 2 * n_year) if y % 4][:n_year]
  days = np.concatenate([
      np.arange(np.datetime64(f'{y}-12-31') - (n_pos - 1),
                np.datetime64(f'{y}-12-31') + 1) for y in years])
  times = days.astype('datetime64[ns]')
  data = precipitation(rng, (times.size, n_point), dtype, quantum=quantum)
  return _case(times, data, ('time', 'point'), frequency='hourly',
               hour_interval=24, window_size=window_size, reference=reference)


def reference_cases() -> dict:
  return {
      'hourly12': hourly(reference=True),
      'hourly12__f64': hourly(np.float64, reference=True),
      'daily': daily(reference=True),
      'edge_data': edge_data(reference=True),
      'long_window': long_window(reference=True),
      'december': december(reference=True),
      'ties': hourly(np.float64, n_point=3, seed=7, quantum=0.5e-3,
                     hour_interval=24, reference=True),
  }


def known_input():
  """The input of the reference's testSEEPSThreshold
  (scripts/compute_climatology_test.py:23-41)."""
  return np.array([0, 0.25, 2, 4, 6]) / 1000


def shard_of(key: str) -> str:
  return key.split('/')[0]


def load_golden() -> dict:
  out = {}
  for path in sorted(glob.glob(os.path.join(GOLDEN_DIR,
                                            GOLDEN_STEM + '.*.npz'))):
    with np.load(path) as f:
      out.update({k: f[k] for k in f.files})
  return out
