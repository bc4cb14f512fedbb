"""NumPy restatement of the neighbourhood fractions of
weatherbench2_amd/neighborhood.py (fractions skill score, Roberts & Lean 2008).

Semantics, for one variable, one threshold field `thr`, one outer index (a
slab of n_row x n_col points, (latitude, longitude)), M members and an odd
window n = 2 h + 1 in grid points:

  k = number of members with x > thr (0..M),  o = 1 if truth > thr else 0.
  IEEE comparisons: a NaN threshold makes both false, equality is not
  exceedance, +-inf are ordinary values.  A point is invalid iff the truth or
  any member is NaN; an invalid point has k = o = 0, STAYS in the window count
  and is left out as a window centre ("missing counts as below the threshold
  in both fields": every denominator is constant along a row).

  The window of centre (i, j): rows max(0, i - h) .. min(n_row - 1, i + h)
  (clipped), columns (j - h .. j + h) mod n_col (cyclic), N_i = n * (rows of
  the clipped range) points.  F = sum_window k, O = M sum_window o,
  P_f = F / (M N_i), P_o = O / (M N_i).

  Per valid centre the terms (P_f - P_o)^2, P_f^2 + P_o^2, P_f, P_o; a
  component is the weighted mean of its term over the valid centres with the
  dense region weights W[i, j] = w_lat[i] lat_mult[i] lon_mult[j]:

    fbs, fbs_reference, forecast_fraction, observed_fraction.

  No valid centre with weight: NaN.  skipna=False: one invalid point anywhere
  in the slab makes the slab NaN for every region (windows cross region
  borders).  fss = 1 - fbs / fbs_reference.

Two forms:
  dense_components    straight from the definition: modular column indices,
                      P_f and P_o in float64, weighted sums with dense weights
  ordered_components  the product's rule: the six integer sums per row
                      ((F-O)^2, F^2, O^2, F, O, 1, each times lon_mult[j], in
                      int64), the row weights g2 = wrow / (D D), g1 = wrow / D,
                      g0 = wrow with D = float(M N_i), then acc = acc + g *
                      float(s) over the rows in increasing order

Bound between the two (u = 2**-53), per component, RELATIVE because every
term of every component is non-negative:

* ordered form: s is an exact integer below 2^53 at the test sizes, so
  float(s) is exact; D D is exact, the division rounds once (u), g * s once
  (u), and a sequential sum of n_row non-negative terms adds (n_row - 1) u
  (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  A
  T_q is within (n_row + 1) u, a component T_a / T_5 (or (T_1 + T_2) / T_5)
  within 2 (n_row + 1) u + 2 u.
* dense form: P_f and P_o carry one rounding each.  Where F = O the two are
  the same float and their difference is exactly 0.  Otherwise the difference
  of the two rounded quotients is exact (or rounds once) and inherits the
  absolute error u (P_f + P_o), that is a relative error u (F + O) / |F - O|
  <= 2 M N u with N the largest window count (|F - O| >= 1, F + O <= 2 M N);
  the square doubles it: 4 M N u + u.  The other terms carry at most 3 u.
  The product with W adds u, the sum of the n_point = n_row n_col non-negative
  terms in any order (n_point - 1) u, the weight sum in the denominator the
  same, the division u: (2 n_point + 4 M N + 4) u.
* in all (2 n_point + 2 n_row + 4 M N + 8) u, which `bound` rounds up to
  (2 n_point + 2 n_row + 4 M N + 16) u.  (Cancellation in P_f - P_o is what
  the 4 M N is for; without it the figure would be (n_point + 16) u-like.)
"""
import numpy as np

U = 2.0 ** -53
COMPONENTS = ('fbs', 'fbs_reference', 'forecast_fraction',
              'observed_fraction')


def bound(n_row, n_col, n_member, windows):
  """rtol between dense_components and ordered_components (docstring)."""
  n_max = max(n * min(n, n_row) for n in windows)
  return (2 * n_row * n_col + 2 * n_row + 4 * n_member * n_max + 16) * U


def fields(ens, truth, thr):
  """(k, o, invalid) int64 [..., R, C] of ens [M, ..., R, C], truth and thr
  [..., R, C]; k = o = 0 where invalid."""
  with np.errstate(invalid='ignore'):
    k = (ens > thr[None]).sum(axis=0).astype(np.int64)
    o = (truth > thr).astype(np.int64)
  bad = np.isnan(truth) | np.isnan(ens).any(axis=0)
  return np.where(bad, 0, k), np.where(bad, 0, o), bad


def point_code(members, truth, thr):
  """The uint16 code of one point from Python scalars: k | o << 8 |
  invalid << 9."""
  if truth != truth or any(x != x for x in members):
    return 0x200
  k = sum(1 for x in members if x > thr)
  return k | (0x100 if truth > thr else 0)


def codes_loop(ens, truth, thrs):
  """uint16 [T, O, R, C] from ens [M, O, R, C], truth [O, R, C] and thrs = T
  arrays [O, R, C]: one Python step per point."""
  n_member, n_outer, n_row, n_col = ens.shape
  out = np.zeros((len(thrs), n_outer, n_row, n_col), dtype=np.uint16)
  for t, thr in enumerate(thrs):
    for o in range(n_outer):
      for i in range(n_row):
        for j in range(n_col):
          out[t, o, i, j] = point_code(
              [ens[m, o, i, j] for m in range(n_member)], truth[o, i, j],
              thr[o, i, j])
  return out


def window_sum(field, n):
  """int64 [..., R, C] -> the sum over the window of every centre, and the
  number of rows of every centre's clipped range."""
  h = n // 2
  n_row, n_col = field.shape[-2:]
  cols = np.arange(n_col)
  # (the box is separable and the sums are integers: columns first)
  across = np.zeros(field.shape, dtype=np.int64)
  for dj in range(-h, h + 1):
    across += field[..., (cols + dj) % n_col]
  out = np.zeros(field.shape, dtype=np.int64)
  n_rows = np.zeros(n_row, dtype=np.int64)
  for i in range(n_row):
    for r in range(max(0, i - h), min(n_row - 1, i + h) + 1):
      n_rows[i] += 1
      out[..., i, :] += across[..., r, :]
  return out, n_rows


def sums_loop(code, windows, n_member, col_class, n_class):
  """int64 [n_cell, n_window, R, n_class, 6] of a code plane [n_cell, R, C]:
  wb2_fss_sums restated from the definition."""
  code = np.asarray(code).astype(np.int64)
  k, o, bad = code & 0xff, (code >> 8) & 1, ((code >> 9) & 1).astype(bool)
  n_cell, n_row, n_col = code.shape
  out = np.zeros((n_cell, len(windows), n_row, n_class, 6), dtype=np.int64)
  for w, n in enumerate(windows):
    f = window_sum(k, n)[0]
    ob = window_sum(o, n)[0] * n_member
    terms = ((f - ob) ** 2, f * f, ob * ob, f, ob, np.ones_like(f))
    for j in range(n_col):
      for q, term in enumerate(terms):
        out[:, w, :, col_class[j], q] += np.where(bad[:, :, j], 0,
                                                  term[:, :, j])
  return out


def _finish(num, den, bad, skipna):
  with np.errstate(all='ignore'):
    out = num / den[..., None]
  dead = den == 0
  if not skipna:
    dead = dead | bad.any(axis=(-2, -1))
  out[dead] = np.nan
  return out


def dense_components(ens, truth, thr, weights, windows, skipna):
  """[..., n_window, 4] from the definition, with the dense weights [R, C]."""
  n_member = ens.shape[0]
  k, o, bad = fields(ens, truth, thr)
  w = np.where(bad, 0.0, np.asarray(weights, np.float64))
  den = w.sum(axis=(-2, -1))
  out = []
  for n in windows:
    f, n_rows = window_sum(k, n)
    so = window_sum(o, n)[0]
    count = (n * n_rows).astype(np.float64)[:, None]
    p_f = f / (n_member * count)
    p_o = so / count
    terms = ((p_f - p_o) ** 2, p_f ** 2 + p_o ** 2, p_f, p_o)
    num = np.stack([(w * term).sum(axis=(-2, -1)) for term in terms], axis=-1)
    out.append(_finish(num, den, bad, skipna))
  return np.stack(out, axis=-2)


def ordered_components(ens, truth, thr, wrow, lon_mult, windows, skipna):
  """The same components by the product's rule (module docstring)."""
  n_member = ens.shape[0]
  k, o, bad = fields(ens, truth, thr)
  mult = np.where(bad, 0, np.asarray(lon_mult, dtype=np.int64))
  n_row = k.shape[-2]
  out = []
  for n in windows:
    f, n_rows = window_sum(k, n)
    ob = window_sum(o, n)[0] * n_member
    terms = ((f - ob) ** 2, f * f, ob * ob, f, ob, np.ones_like(f))
    acc = [np.zeros(k.shape[:-2]) for _ in terms]
    for i in range(n_row):
      d = float(n_member * n * n_rows[i])
      g = (wrow[i] / (d * d),) * 3 + (wrow[i] / d,) * 2 + (wrow[i],)
      for q, term in enumerate(terms):
        s = (mult[..., i, :] * term[..., i, :]).sum(axis=-1)
        acc[q] = acc[q] + g[q] * s.astype(np.float64)
    num = np.stack([acc[0], acc[1] + acc[2], acc[3], acc[4]], axis=-1)
    out.append(_finish(num, acc[5], bad, skipna))
  return np.stack(out, axis=-2)


def fold(sums, w, mult):
  """wb2_fss_fold restated with Python loops over regions and rows."""
  n_cell, n_window, n_row, n_class, _ = sums.shape
  group = (0, 0, 0, 1, 1, 2)
  out = np.zeros((n_cell, n_window, len(mult), 6))
  for r in range(len(mult)):
    for win in range(n_window):
      for q in range(6):
        acc = np.zeros(n_cell)
        for i in range(n_row):
          s = np.zeros(n_cell, dtype=np.int64)
          for c in range(n_class):
            s += int(mult[r][c]) * sums[:, win, i, c, q].astype(np.int64)
          acc = acc + float(w[win][group[q]][r][i]) * s.astype(np.float64)
        out[:, win, r, q] = acc
  return out
