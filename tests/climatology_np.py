"""The arithmetic of csrc/climatology.hip (K14) in NumPy, in exactly the
kernels' order, the literal windowed form it replaces, `assert_same`, and the
error bounds against the reference's fixtures.

Restatement.  x is [n_outer, n_time, n_point]; groups are a CSR list
(group_begin, member) of time steps with an optional `fill`:
  first_finite  the first sample of every point, in member order, that is
                neither NaN nor +-inf; 0.0 if none
  group_moments per group, members in order: x, else the fill step where x is
                NaN, skipped if still NaN; y = float64(x) - pivot; count += 1;
                sum += y; sumsq += y * y (starting from +0.0)
  cycle_smooth  explicit: W0, W1, W2 = S_k w[k+H] (C, S, Q)[(a + k) mod n],
                k = -H .. H in order; m = W1 / W0; mean = pivot + m; v = W2 /
                W0 - m * m; std = sqrt(v < 0 ? 0 : v); NaN where W0 == 0.
                fast: per position pivot + S / C and sqrt(max(Q / C - (S /
                C)^2, 0)), NaN where C == 0; then the sum, in the order i = -H
                .. H, of the products value[(a - i) mod n] * w[i+H] that are
                not NaN, divided by their number.
NumPy's +, -, *, / and sqrt on float64 are the IEEE operations, one rounding
each and no fused multiply-add, which is what the kernels are compiled to
(-ffp-contract=off), so the device result has the same bits.

Bounds (restatement against the reference's own output).  u = 2^-53.  For one
output let the terms be the (year, tap) entries that are not NaN after the
fill, N their number, w_t, x_t their weights and values, p the pivot of the
point, y_t = x_t - p, and
  A1 = S w|y| / S w,  A2 = S w y^2 / S w,  X1 = S w|x| / S w.
explicit, mean.  Ours is p + W1 / W0.  Each y_t carries one rounding (u|y_t|);
  the sums over a group and then over the taps add the N products w_t y_t and
  the N products w_t * 1 one after another, each partial sum rounded once:
  |error of W1| <= (N + 1) u S w|y|, likewise for W0, so W1 / W0 is within
  (2N + 4) u A1, and the final p + m adds u|mean|.  The reference forms
  dot(fillna(x, 0), w) / dot(notnull(x), w) on the raw x: its own error is up
  to (2N + 4) u X1.  The bound is the sum of both,
    mean_bound = (2N + 4) u (A1 + X1) + 2 u |mean|;
  the second term is the reference's error, not ours: with x near 1e5 it is
  1e5 times the first.
explicit, variance (variances are compared, not stds).  Ours is W2 / W0 - m^2:
  W2 / W0 is within (2N + 5) u A2 (one more rounding for y * y); m^2 is within
  2 (2N + 4) u A1^2 + u m^2 <= (4N + 9) u A2 by Cauchy-Schwarz (A1^2 <= A2);
  the subtraction adds u A2.  The reference forms S w (x - mean)^2 / S w with
  its own mean: within (2N + 6) u var <= (2N + 6) u A2, plus d^2 where d is
  the error of its mean (the first-order term vanishes: S w (x - mean) = 0).
    var_bound = (8N + 21) u A2 + ((2N + 4) u X1)^2.
  Moments about zero would put x^2 in the place of y^2: at x = 1e5 + N(0, 1)
  that is 1e10 times this bound's A2, and the form fails it.
Inputs that differ.  Where the series itself comes from an earlier float stage
  that the reference and this build round differently (the daily mean of n_d
  samples in the input's dtype T: both sum n_d terms in T, in different
  orders), each sample may differ by e_t <= 2 n_d u_T mean|x|.  The mean then
  moves by at most E1 = S w e / S w and the variance by at most 2 sqrt(A2 E2) +
  E2 + E1^2 with E2 = S w e^2 / S w (Cauchy-Schwarz on S w |y| e); both are
  added.
fast.  v[a] is the mean (or std) of the n_a members of one day of year; the
  output is the mean over the c products v[(a - i) mod n] * w[i+H] that are
  not NaN.  With dv[a] the bound of v[a] (from the formulas above with N = n_a
  and unit weights; for the std, |sqrt(s) - sqrt(t)| <= min(sqrt|s - t|, |s -
  t| / sqrt(s))) the output is within
    S w dv / c + (2c + 2) u S |w v| / c.
  For float32 input the reference keeps float32 in that first stage
  (groupby(...).mean() and .std() keep the dtype): its v[a] is within n_a u32
  mean|x| + u32 |v| for the mean, and for the variance (n_a + 5) u32 (var +
  d^2) + d^2 with d its float32 mean's error, u32 = 2^-24.  These replace the
  reference's float64 terms for the float32 fixtures; the float64 twins of
  the same values get the float64 bound.
"""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def first_finite(x, member):
  n_outer, n_time, n_point = x.shape
  pivot = np.zeros((n_outer, n_point))
  found = np.zeros((n_outer, n_point), dtype=bool)
  for step in np.asarray(member).tolist():
    if not 0 <= step < n_time:
      continue
    v = x[:, step, :]
    take = ~found & ~np.isnan(v) & ~np.isinf(v)
    pivot = np.where(take, v.astype(np.float64), pivot)
    found = found | take
  return pivot


def _members(x, group_begin, member, fill):
  """Yields (group, the samples of one member after the fill)."""
  n_outer, n_time, n_point = x.shape
  begin = np.asarray(group_begin).tolist()
  member = np.asarray(member).tolist()
  fill = None if fill is None else np.asarray(fill).tolist()
  for g in range(len(begin) - 1):
    for j in range(max(0, begin[g]), min(begin[g + 1], len(member))):
      if 0 <= member[j] < n_time:
        v = x[:, member[j], :]
      else:
        v = np.full((n_outer, n_point), np.nan, dtype=x.dtype)
      if fill is not None and 0 <= fill[j] < n_time:
        v = np.where(np.isnan(v), x[:, fill[j], :], v)
      yield g, v


def group_moments(x, group_begin, member, fill=None, pivot=None):
  """(count, sum, sumsq), each float64 [n_outer, n_group, n_point]."""
  n_outer, _, n_point = x.shape
  n_group = len(group_begin) - 1
  pivot = np.zeros((n_outer, n_point)) if pivot is None else pivot
  count = np.zeros((n_outer, n_group, n_point))
  total = np.zeros_like(count)
  sumsq = np.zeros_like(count)
  with np.errstate(all='ignore'):
    for g, v in _members(x, group_begin, member, fill):
      ok = ~np.isnan(v)
      y = v.astype(np.float64) - pivot
      count[:, g] = np.where(ok, count[:, g] + 1.0, count[:, g])
      total[:, g] = np.where(ok, total[:, g] + y, total[:, g])
      sumsq[:, g] = np.where(ok, sumsq[:, g] + y * y, sumsq[:, g])
  return count, total, sumsq


def _sqrt0(v):
  return np.sqrt(np.where(v < 0, 0.0, v))


def _cycles(a, n_cycle, n_pos):
  return a.reshape(a.shape[0], n_cycle, n_pos, a.shape[2])


def cycle_smooth(mode, moments, pivot, n_cycle, n_pos, w):
  """(mean, std), each float64 [n_outer, n_cycle * n_pos, n_point]."""
  shape = moments[0].shape
  c, s, q = (_cycles(a, n_cycle, n_pos) for a in moments)
  p = (np.zeros((shape[0], shape[2])) if pivot is None else pivot)[
      :, None, None, :]
  w = np.asarray(w, dtype=np.float64)
  half = len(w) // 2
  pos = np.arange(n_pos)
  with np.errstate(all='ignore'):
    if mode == 'explicit':
      w0, w1, w2 = np.zeros(c.shape), np.zeros(c.shape), np.zeros(c.shape)
      for k in range(-half, half + 1):
        at = np.mod(pos + k, n_pos)
        w0 = w0 + w[k + half] * c[:, :, at]
        w1 = w1 + w[k + half] * s[:, :, at]
        w2 = w2 + w[k + half] * q[:, :, at]
      m = w1 / w0
      v = w2 / w0 - m * m
      mean = np.where(w0 == 0, np.nan, p + m)
      std = np.where(w0 == 0, np.nan, _sqrt0(v))
    elif mode == 'fast':
      m = s / c
      v = q / c - m * m
      out = []
      for value in (np.where(c == 0, np.nan, p + m),
                    np.where(c == 0, np.nan, _sqrt0(v))):
        total, n = np.zeros(c.shape), np.zeros(c.shape)
        for i in range(-half, half + 1):
          product = value[:, :, np.mod(pos - i, n_pos)] * w[i + half]
          ok = ~np.isnan(product)
          total = np.where(ok, total + product, total)
          n = n + ok
        out.append(np.where(n == 0, np.nan, total / n))
      mean, std = out
    else:
      raise ValueError(mode)
  return mean.reshape(shape), std.reshape(shape)


def assert_same(got, want, what=''):
  """Bit equality: the same NaNs, the same values and the same zero signs."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), f'{what}: NaNs differ'
  same = (got == want) & (np.signbit(got) == np.signbit(want)) | nan
  if not same.all():
    at = np.argwhere(~same)[0]
    raise AssertionError(
        f'{what}: {np.count_nonzero(~same)} of {same.size} differ, first at '
        f'{tuple(at)}: {got[tuple(at)]!r} != {want[tuple(at)]!r}')


def assert_within_ulp(got, want, ulps, what=''):
  got, want = np.asarray(got), np.asarray(want)
  assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaNs differ'
  with np.errstate(all='ignore'):
    bad = np.abs(got - want) > ulps * np.spacing(np.abs(want))
  bad &= ~np.isnan(want) & (got != want)
  assert not bad.any(), f'{what}: {np.count_nonzero(bad)} beyond {ulps} ulp'


# ---------------------------------------------------------------------------
# the literal form: what the reference spells out, for one series
# ---------------------------------------------------------------------------
def literal_explicit(table, w):
  """`table` [n_year, n] (NaN = no sample), already filled -> (mean, variance)
  [n]: the weighted mean and variance over (window, year) of the wrap-padded,
  W-wide windows."""
  w = np.asarray(w, dtype=np.float64)
  half = len(w) // 2
  n = table.shape[1]
  at = np.mod(np.arange(-half, n + half), n)  # np.pad(mode='wrap'), any width
  windows = np.lib.stride_tricks.sliding_window_view(
      table[:, at].astype(np.float64), len(w), axis=1)  # [year, n, W]
  ok = ~np.isnan(windows)
  with np.errstate(all='ignore'):
    sw = (ok * w).sum(axis=(0, 2))
    mean = np.where(ok, windows * w, 0.0).sum(axis=(0, 2)) / sw
    dev = np.where(ok, (windows - mean[None, :, None]) ** 2 * w, 0.0)
    var = dev.sum(axis=(0, 2)) / sw
  return np.where(sw == 0, np.nan, mean), np.where(sw == 0, np.nan, var)


# ---------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------
def _abs_moments(x, group_begin, member, fill, pivot, err):
  """Per group: N, S|y|, S y^2, S|x|, S e, S e^2 (e = `err` at the sample)."""
  n_outer, _, n_point = x.shape
  out = np.zeros((6, n_outer, len(group_begin) - 1, n_point))
  e_all = None if err is None else np.asarray(err, dtype=np.float64)
  for (g, v), (_, e) in zip(
      _members(x, group_begin, member, fill),
      _members(x if e_all is None else e_all, group_begin, member, fill)):
    ok = np.isfinite(v)
    v = np.where(ok, v, 0).astype(np.float64)
    y = np.where(ok, v - pivot, 0.0)
    e = np.zeros_like(y) if e_all is None else np.where(ok & np.isfinite(e),
                                                        e, 0.0)
    for k, term in enumerate((ok, np.abs(y), y * y, np.abs(v), e, e * e)):
      out[k, :, g] += term
  return out


def _window(a, n_cycle, n_pos, w, sign=1):
  a = _cycles(a, n_cycle, n_pos)
  half = len(w) // 2
  pos = np.arange(n_pos)
  out = np.zeros(a.shape)
  for k in range(-half, half + 1):
    out += abs(w[k + half]) * a[:, :, np.mod(pos + sign * k, n_pos)]
  return out.reshape(a.shape[0], n_cycle * n_pos, a.shape[3])


def explicit_bounds(x, group_begin, member, fill, pivot, n_cycle, n_pos, w,
                    mean, err=None):
  """(mean_bound, var_bound) of the module docstring, the shape of `mean`
  [n_outer, n_group, n_point].  Samples that are not finite make their outputs
  NaN or inf on both sides and are left out of the sums here."""
  w = np.asarray(w, dtype=np.float64)
  n, a1, a2, x1, e1, e2 = _abs_moments(x, group_begin, member, fill, pivot,
                                       err)
  ones = np.ones_like(w)
  with np.errstate(all='ignore'):
    big_n = _window(n, n_cycle, n_pos, ones)
    sw = _window(n, n_cycle, n_pos, w)
    a1, a2, x1, e1, e2 = (_window(a, n_cycle, n_pos, w) / sw
                          for a in (a1, a2, x1, e1, e2))
    mean_bound = ((2 * big_n + 4) * U64 * (a1 + x1)
                  + 2 * U64 * np.abs(mean) + e1)
    var_bound = ((8 * big_n + 21) * U64 * a2
                 + ((2 * big_n + 4) * U64 * x1) ** 2
                 + 2 * np.sqrt(a2 * e2) + e2 + e1 ** 2)
  return mean_bound, var_bound


def fast_bounds(x, group_begin, member, pivot, n_cycle, n_pos, w, value_mean,
                value_std, u_ref=U64, err=None):
  """(mean_bound, std_bound) of the `fast` outputs; value_mean, value_std are
  the per-position statistics [n_outer, n_group, n_point] (the restatement's),
  u_ref the unit of the reference's first stage."""
  w = np.asarray(w, dtype=np.float64)
  n, a1, a2, x1, e1, e2 = _abs_moments(x, group_begin, member, None, pivot,
                                       err)
  with np.errstate(all='ignore'):
    a1, a2, x1, e1, e2 = (a / n for a in (a1, a2, x1, e1, e2))
    ref_mean = (2 * n + 4) * u_ref * x1 + u_ref * np.abs(value_mean)
    d_mean = ((2 * n + 4) * U64 * a1 + 2 * U64 * np.abs(value_mean)
              + ref_mean + e1)
    d_var = ((6 * n + 15) * U64 * a2
             + (2 * n + 6) * u_ref * (a2 + ref_mean ** 2) + ref_mean ** 2
             + 2 * np.sqrt(a2 * e2) + e2 + e1 ** 2)
    d_std = np.minimum(np.sqrt(d_var), d_var / value_std)
    d_std = d_std + u_ref * np.abs(value_std)  # (the square root's rounding)
    out = []
    half = len(w) // 2
    pos = np.arange(n_pos)
    for value, d in ((value_mean, d_mean), (value_std, d_std)):
      value, d = _cycles(value, n_cycle, n_pos), _cycles(d, n_cycle, n_pos)
      c, moved, size = (np.zeros(value.shape) for _ in range(3))
      for i in range(-half, half + 1):
        at = np.mod(pos - i, n_pos)
        product = value[:, :, at] * w[i + half]
        ok = np.isfinite(product)  # (inf products make the output inf or NaN)
        c += ~np.isnan(product)
        moved += np.where(ok, abs(w[i + half]) * d[:, :, at], 0.0)
        size += np.where(ok, np.abs(product), 0.0)
      out.append(((moved + (2 * c + 2) * U64 * size) / c).reshape(
          value_mean.shape))
  return tuple(out)
