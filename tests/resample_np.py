"""NumPy restatement of weatherbench2_amd/resampling.py and of the K13 kernel
(csrc/time_window.hip): the bins from the formulas of the module docstring,
the statistics by a sequential loop over the time steps of each bin, in the
data's own float type.  Independent of the product code; checked against the
fixtures of tests/golden/make_resample_vectors.py and against pandas in
tests/test_resampling_cpu.py.
"""
import numpy as np

NS = {'w': 7 * 86400 * 10**9, 'd': 86400 * 10**9, 'h': 3600 * 10**9,
      'min': 60 * 10**9, 's': 10**9}
DAY = NS['d']
STATS = ('mean', 'min', 'max', 'sum')


def period_ns(period: str) -> int:
  for unit in ('min', 'w', 'd', 'h', 's'):
    if period.endswith(unit):
      return int(period[:-len(unit)]) * NS[unit]
  raise ValueError(period)


def _ns(times):
  times = np.asarray(times)
  kind = times.dtype.kind
  unit = 'datetime64[ns]' if kind == 'M' else 'timedelta64[ns]'
  return [int(v) for v in times.astype(unit).astype(np.int64)], unit


def resample_bins(times, period: int, label_side: str):
  """(labels, [(begin, end)]) by walking the edges one at a time."""
  ns, unit = _ns(times)
  t0, last = ns[0], ns[-1]
  off = ((t0 % DAY) % period) if unit.startswith('datetime') else 0
  labels, ranges = [], []
  if label_side == 'left':
    edge = t0 - off
    while edge <= last:
      members = [i for i, v in enumerate(ns) if edge <= v < edge + period]
      labels.append(edge)
      ranges.append((members[0], members[-1] + 1) if members else (0, 0))
      edge += period
  else:
    edge = t0 - off if off > 0 else t0 - period
    # pandas' timedelta binner runs one period past a last time on an edge
    extra = unit.startswith('timedelta') and (last - edge) % period == 0
    while edge < last or (extra and edge == last):
      members = [i for i, v in enumerate(ns) if edge < v <= edge + period]
      labels.append(edge + period)
      ranges.append((members[0], members[-1] + 1) if members else (0, 0))
      edge += period
    labels, ranges = labels[1:], ranges[1:]  # the script drops the first bin
  return np.array(labels, dtype=np.int64).astype(unit), ranges


def rolling_bins(n_time: int, w: int):
  return [(t - w + 1, t + 1) for t in range(n_time)]


def bin_stats(x: np.ndarray, axis: int, ranges, skipna: bool) -> dict:
  """{'sum', 'mean', 'min', 'max'}: arrays of the shape of `x` with `axis`
  replaced by the bins.  Integers are taken as float64."""
  x = np.asarray(x)
  if x.dtype not in (np.float32, np.float64):
    x = x.astype(np.float64)
  T = x.dtype.type
  x = np.moveaxis(x, axis, 0)
  n_time = x.shape[0]
  flat = x.reshape(n_time, -1)
  n_point = flat.shape[1]
  out = {s: np.full((len(ranges), n_point), np.nan, dtype=x.dtype)
         for s in STATS}
  with np.errstate(all='ignore'):
    for b, (begin, end) in enumerate(ranges):
      if begin < 0 or begin >= end or end > n_time:
        continue  # empty or incomplete: NaN everywhere
      rows = flat[begin:end]
      bad = np.isnan(rows)
      m = (~bad).sum(axis=0)
      terms = np.where(bad, T(0), rows) if skipna else rows
      acc = terms[0].copy()
      for row in terms[1:]:
        acc = acc + row
      lo = np.full(n_point, np.inf, dtype=x.dtype)
      hi = np.full(n_point, -np.inf, dtype=x.dtype)
      for row in rows:
        lo = np.where(row < lo, row, lo)
        hi = np.where(row > hi, row, hi)
      if skipna:
        mean = np.where(m == 0, T(np.nan), acc / m.astype(x.dtype))
        void = m == 0
      else:
        mean = acc / T(end - begin)
        void = bad.any(axis=0)
      out['sum'][b] = acc
      out['mean'][b] = mean
      out['min'][b] = np.where(void, T(np.nan), lo)
      out['max'][b] = np.where(void, T(np.nan), hi)
  shape = (len(ranges),) + x.shape[1:]
  return {s: np.moveaxis(a.reshape(shape), 0, axis) for s, a in out.items()}


def abs_sums(x: np.ndarray, axis: int, ranges) -> tuple:
  """(float64 sum of |x| per bin with NaN as 0, the bin lengths), for the
  error bounds."""
  a = np.abs(np.asarray(x, dtype=np.float64))
  a = np.moveaxis(np.where(np.isnan(a), 0.0, a), axis, 0)
  sums = np.zeros((len(ranges),) + a.shape[1:])
  for b, (begin, end) in enumerate(ranges):
    if 0 <= begin < end <= a.shape[0]:
      sums[b] = a[begin:end].sum(axis=0)
  lengths = np.array([max(e - b, 0) for b, e in ranges])
  return np.moveaxis(sums, 0, axis), lengths


def valid_counts(x: np.ndarray, axis: int, ranges) -> np.ndarray:
  """Samples that are not NaN, per bin."""
  ok = np.moveaxis(~np.isnan(np.asarray(x, dtype=np.float64)), axis, 0)
  counts = np.zeros((len(ranges),) + ok.shape[1:])
  for b, (begin, end) in enumerate(ranges):
    if 0 <= begin < end <= ok.shape[0]:
      counts[b] = ok[begin:end].sum(axis=0)
  return np.moveaxis(counts, 0, axis)


def plan(case) -> tuple:
  """(labels of the core call, ranges) of a case of tests/resample_cases.py."""
  times = case['coords'][case['time_dim']]
  per = period_ns(case['period'])
  if case['method'] == 'rolling':
    ns, unit = _ns(times)
    w = per // (ns[1] - ns[0])
    return np.asarray(times).astype(unit), rolling_bins(len(ns), w)
  return resample_bins(times, per, case['label_side'])


def shifted_labels(case) -> np.ndarray:
  """The labels of `resample_in_time`: `main`'s shift for rolling."""
  labels, _ = plan(case)
  if case['method'] != 'rolling':
    return labels
  ns, unit = _ns(case['coords'][case['time_dim']])
  delta = ns[1] - ns[0]
  per = period_ns(case['period'])
  shift = delta - per if case['label_side'] == 'left' else delta
  return (np.array(ns, dtype=np.int64) + shift).astype(unit)


def output_names(case) -> list:
  """[(output name, input name, statistic)] in the reference's order."""
  out = []
  for name, (dims, _) in case['vars'].items():
    if case['time_dim'] not in dims:
      continue
    for stat in STATS:
      if name in case['stats'][stat]:
        suffix = '_' + stat
        if stat == 'mean' and not case['add_mean_suffix']:
          suffix = ''
        out.append((name + suffix, name, stat))
  return out


def resample(case, skipna: bool) -> dict:
  """{output name: (dims, array)} of `resample_in_time` on a case."""
  _, ranges = plan(case)
  skip = skipna and case['method'] != 'rolling'
  cache, out = {}, {}
  for new, name, stat in output_names(case):
    dims, array = case['vars'][name]
    if name not in cache:
      cache[name] = bin_stats(array, dims.index(case['time_dim']), ranges, skip)
    out[new] = (dims, cache[name][stat])
  return out


def assert_same(got, want, what=''):
  """Equal values with NaN in the same places (zeros of either sign equal),
  same dtype and shape."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  np.testing.assert_array_equal(got, want, err_msg=what)


def assert_within_bound(got, fixture, stat, abs_sum, lengths, axis, skipna,
                        counts=None, what=''):
  """`got` against a fixture value computed in another order of the same
  terms: NaN and inf in the same places; sums within 2 n u sum|x|, means within
  that over the count plus u |mean|; min and max equal."""
  got = np.asarray(got)
  fixture = np.asarray(fixture).astype(got.dtype)
  assert got.shape == fixture.shape, (what, got.shape, fixture.shape)
  assert np.array_equal(np.isnan(got), np.isnan(fixture)), what
  assert np.array_equal(np.isinf(got), np.isinf(fixture)), what
  fin = np.isfinite(got)
  if stat in ('min', 'max'):
    np.testing.assert_array_equal(got, fixture, err_msg=what)
    return
  u = float(np.finfo(got.dtype).eps) / 2
  shape = [1] * got.ndim
  shape[axis] = len(lengths)
  n = lengths.reshape(shape).astype(np.float64)
  bound = 2 * n * u * abs_sum
  if stat == 'mean':
    count = n if counts is None else counts
    with np.errstate(all='ignore'):
      bound = bound / np.maximum(count, 1) + u * np.abs(
          fixture.astype(np.float64))
  with np.errstate(all='ignore'):
    err = np.abs(got.astype(np.float64) - fixture.astype(np.float64))
  bound = np.broadcast_to(bound, got.shape)
  assert np.all(err[fin] <= bound[fin]), (
      what, float(np.max(err[fin] - bound[fin])))
