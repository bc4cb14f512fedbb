"""NumPy restatement of the window quantile and the SEEPS threshold of
scripts/compute_climatology.py (`Quantile`, `SEEPSThreshold`) through
weatherbench2/utils.py:88-124, with no code of the module under test.

The statistic.  Per hour of day and per point the reference builds X[y, a]
(years present x sorted union of the days of year, a NaN entry replaced by the
year's day 365, the day axis wrapped) and hands the samples X[y, (a + k) mod n],
k = -H .. H, with the weights w[k + H] to xarray's weighted quantile
(`_weighted_quantile_1d`, method 'linear', NaNs and zero weights dropped).
xarray is not at hand: this is this build's reading of it.  With the kept
samples sorted by value, their weights normalised to sum 1, cum = [0,
cumsum(w)], n = 1 / S w^2, h = (n - 1) q + 1:
    u = max((h - 1) / n, min(h / n, cum)),  v = u n - h + 1,
    result = S data diff(v)                                            (R)
`cumsum_form` below is (R) written out.  diff(v)_i is n times the length of
[cum_{i-1}, cum_i] ^ [(h - 1) / n, h / n], so (R) is n times the integral of
the step function "sorted value over cumulative weight" over an interval of
length 1 / n.  The window weights are proportional to the integers m = H - |k|
and the normalisation removes the scale, so with M = S m, Q = S m^2 and the
integer cumulative sums c_i:
    n = M M / Q,  A = (h - 1) / n M,  B = h / n M  (clamped to [0, M]),
    result = n / M * S_i x_(i) |[c_{i-1}, c_i] ^ [A, B]|                (I)
`interval_form` is (I).  Only the order statistics the interval touches
contribute, equal values need no order, and with equal weights (I) is NumPy's
linear quantile.

SEEPS.  is_dry = x < T(dry_mm / 1000), compared in the data's dtype T;
dry_fraction = (dry entries of the window) / (W n_year), unweighted, a NaN
entry not dry; threshold = (I) at q = 2 / 3 over the entries that are neither
NaN nor dry.

Bounds (u = 2^-53; K the samples with a positive length, at least 1).
  * Two evaluations of (I) in float64 that form n, h, A, B by the same
    operations (they are then the same numbers) and differ in how the K terms
    are grouped and ordered.  Each length is one subtraction of numbers that
    are exact or shared (relative error u), each product one rounding, a sum
    of K terms in any order at most (K - 1) u S|x len|, n / M and the last
    product one rounding each.  With S len = B - A = M / n and |x| <= X:
        |error| <= (K + 4) u X  per evaluation,
    so two evaluations differ by at most (2 K + 8) u X.  For K = 1 and K = 2
    there is nothing to reorder and the evaluations are identical; for K >= 3,
    2 K + 8 <= 8 K.  The constant 8 of `interval_bound` = 8 K u X holds.
  * (R) as the reference computes it against (I).  The reference's cum is a
    float cumsum of N normalised weights: absolute error at most N u (total
    weight 1), which moves an end of a clipped segment by that much and hence
    diff(v) by at most 2 N n u; since S diff(v) is fixed, shifting all values
    by a constant changes nothing to first order, so this costs at most
    2 N n u * spread, spread = the range of the touched order statistics and
    one neighbour on each side (a moved end can reach the neighbour).  v = u n
    - h + 1 is itself rounded at magnitude <= n: each diff(v) carries up to
    4 n u more, against |x| <= X, over at most K + 2 terms.  With slack for
    n, h and the final sum:
        `reference_bound` = 8 n u (N spread + (K + 2) X).
    For the fixture's sizes (N <= 427, n <= N) the first term is below
    8 * 427^2 * 1.1e-16 = 1.7e-10 of the spread, far from one order statistic
    to the next; the second is 1e-13 of the data's magnitude, the rounding of
    v, and hides a wrong order statistic only where two neighbours agree to
    that.  `reference_bound` asserts the first condition.
"""
import numpy as np

U = 2.0 ** -53


def window_weights(window_size):
  """The integers H - |k| the reference's window weights are proportional
  to."""
  half = window_size // 2
  return half - np.abs(np.arange(-half, half + 1))


def interval_form(values, weights, q):
  """(I) for one point: `values` the kept samples, `weights` their positive
  integer weights -> (result, K, X, spread, n)."""
  values = np.asarray(values, dtype=np.float64)
  weights = np.asarray(weights, dtype=np.int64)
  if values.size == 0:
    return np.nan, 1, 0.0, 0.0, 0.0
  order = np.argsort(values, kind='stable')
  x, m = values[order], weights[order]
  c = np.cumsum(m)
  c0 = c - m
  big = float(c[-1])
  n = big * big / float((m * m).sum())
  h = (n - 1.0) * q + 1.0
  lo = max((h - 1.0) / n * big, 0.0)
  hi = min(h / n * big, big)
  length = np.minimum(c, hi) - np.maximum(c0, lo)
  touched = np.nonzero(length > 0)[0]
  total = 0.0
  for i in touched.tolist():
    total += x[i] * length[i]
  first = max(int(touched[0]) - 1, 0)
  last = min(int(touched[-1]) + 1, x.size - 1)
  with np.errstate(all='ignore'):
    spread = float(x[last] - x[first])
  return (n / big * total, max(int(touched.size), 1),
          float(np.abs(x[first:last + 1]).max()), spread, n)


def cumsum_form(values, weights, q):
  """(R) for one point, float weights of any scale."""
  values = np.asarray(values, dtype=np.float64)
  weights = np.asarray(weights, dtype=np.float64)
  keep = ~np.isnan(values) & (weights != 0)
  values, weights = values[keep], weights[keep]
  if values.size == 0:
    return np.nan
  order = np.argsort(values, kind='stable')
  data, w = values[order], weights[order]
  w = w / w.sum()
  cum = np.append(0.0, np.cumsum(w))
  n = 1.0 / (w * w).sum()
  h = (n - 1.0) * q + 1.0
  u = np.maximum((h - 1.0) / n, np.minimum(h / n, cum))
  v = u * n - h + 1.0
  return float((data * np.diff(v)).sum())


def interval_bound(k, xmax):
  return 8.0 * k * U * xmax


def reference_bound(n_sample, n_eff, k, xmax, spread):
  assert np.all(8.0 * n_sample * n_eff * U < 1e-8)
  return 8.0 * n_eff * U * (n_sample * spread + (k + 2) * xmax)


def window_stat(table, window_size, qs, dry_threshold=None):
  """`table` [n_year, n_pos, n_point] in dtype T (NaN = no sample), already
  filled -> dict of float64 arrays [n_q, n_pos, n_point]: 'quantile', 'k',
  'xmax', 'spread', 'n_eff', and [n_pos, n_point]: 'dry_fraction',
  'n_sample'."""
  n_year, n_pos, n_point = table.shape
  m = window_weights(window_size)
  half = window_size // 2
  qs = np.asarray(qs, dtype=np.float64)
  out = {k: np.zeros((qs.size, n_pos, n_point))
         for k in ('quantile', 'k', 'xmax', 'spread', 'n_eff')}
  out['dry_fraction'] = np.zeros((n_pos, n_point))
  out['n_sample'] = np.zeros((n_pos, n_point))
  threshold = None if dry_threshold is None else table.dtype.type(
      dry_threshold)
  for a in range(n_pos):
    at = (a + np.arange(-half, half + 1)) % n_pos
    for i in range(n_point):
      sample = table[:, at, i]              # [n_year, W]
      weight = np.broadcast_to(m, sample.shape)
      dry = (sample < threshold if threshold is not None
             else np.zeros(sample.shape, dtype=bool))
      keep = ~np.isnan(sample) & ~dry & (weight > 0)
      out['dry_fraction'][a, i] = np.float64(dry.sum()) / np.float64(
          window_size * n_year)
      out['n_sample'][a, i] = keep.sum()
      for j, q in enumerate(qs.tolist()):
        res = interval_form(sample[keep], weight[keep], q)
        for name, value in zip(('quantile', 'k', 'xmax', 'spread', 'n_eff'),
                               res):
          out[name][j, a, i] = value
  return out


def launch(x, group_begin, member, fill, n_cycle, n_pos, window_size, qs,
           dry_threshold=None, n_year=None):
  """The K15 launch: x [n_outer, n_time, n_point], K14's group lists -> the
  dict of `window_stat` with [n_q, n_outer, n_cycle * n_pos, n_point] (and
  [n_outer, n_cycle * n_pos, n_point]) arrays.  `n_year` is the denominator's
  year count (default: the largest group)."""
  n_outer, n_time, n_point = x.shape
  begin = np.asarray(group_begin).tolist()
  member = np.asarray(member).tolist()
  fill = None if fill is None else np.asarray(fill).tolist()
  rows = max([b - a for a, b in zip(begin[:-1], begin[1:])] + [1])
  n_year = rows if n_year is None else n_year
  parts = []
  for o in range(n_outer):
    for c in range(n_cycle):
      table = np.full((max(rows, n_year), n_pos, n_point), np.nan,
                      dtype=x.dtype)
      for a in range(n_pos):
        g = c * n_pos + a
        for y, j in enumerate(range(begin[g], begin[g + 1])):
          v = (x[o, member[j]] if 0 <= member[j] < n_time
               else np.full(n_point, np.nan, dtype=x.dtype))
          if fill is not None and 0 <= fill[j] < n_time:
            v = np.where(np.isnan(v), x[o, fill[j]], v)
          table[y, a] = v
      parts.append(window_stat(table, window_size, qs, dry_threshold))
  out = {}
  for name in parts[0]:
    lead = parts[0][name].shape[:-2]
    stacked = np.stack([p[name] for p in parts]).reshape(
        (n_outer, n_cycle) + parts[0][name].shape)
    if lead:  # [o, c, q, a, i] -> [q, o, c * a, i]
      out[name] = np.moveaxis(stacked, 2, 0).reshape(
          lead + (n_outer, n_cycle * n_pos, n_point))
    else:
      out[name] = stacked.reshape(n_outer, n_cycle * n_pos, n_point)
  return out


def year_tables(times, data, hour=None):
  """The reference's stacked, filled table of one series: `times` datetime64,
  `data` [n_time, n_point]; `hour` None for a series with one step a day, else
  the hour of day to select -> (table [n_year, n_pos, n_point], axis)."""
  times = np.asarray(times)
  day = times.astype('datetime64[D]')
  start = times.astype('datetime64[Y]')
  year = start.astype(np.int64) + 1970
  doy = (day - start.astype('datetime64[D]')).astype(np.int64) + 1
  pick = np.arange(times.size)
  if hour is not None:
    pick = pick[times.astype('datetime64[h]').astype(np.int64)[pick] % 24
                == hour]
  years = np.unique(year[pick])
  axis = np.unique(doy[pick])
  table = np.full((years.size, axis.size, data.shape[1]), np.nan,
                  dtype=data.dtype)
  table[np.searchsorted(years, year[pick]),
        np.searchsorted(axis, doy[pick])] = data[pick]
  at365 = int(np.searchsorted(axis, 365))
  assert axis[at365] == 365
  table = np.where(np.isnan(table), table[:, at365:at365 + 1], table)
  return table, axis


def assert_within(got, want, bound, what=''):
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaNs differ'
  ok = ~np.isnan(want)
  err = np.abs(got[ok] - want[ok])
  lim = np.broadcast_to(bound, want.shape)[ok]
  worst = (err - lim).max() if err.size else 0.0
  assert worst <= 0, (f'{what}: error {err.max():.3e} exceeds its bound by '
                      f'{worst:.3e} (bound at that place '
                      f'{lim[(err - lim).argmax()]:.3e})')


def restate_hourly(times, data, hours, window_size, qs, dry_threshold=None):
  """`window_stat` of every hour of day of a series `data` [n_time, n_point],
  each array with a leading hour axis; `hours` None for one step a day."""
  parts = [window_stat(year_tables(times, data, h)[0], window_size, qs,
                       dry_threshold)
           for h in ([None] if hours is None else list(hours))]
  return {k: np.stack([p[k] for p in parts]) for k in parts[0]}
