"""NumPy restatement of weatherbench2_amd/quantile_scores.py: dense, per
point, float64, nothing from the package.

Members sorted x_0 <= ... <= x_{M-1} (np.sort), level tau at the 0-based
position v clamped to [0, M - 1]: tau (M - 1) ('linear'), M tau - 1/2
('hazen'), (M + 1) tau - 1 ('weibull'); lo = floor(v), t = v - lo, hi = min(lo
+ 1, M - 1); d = x_hi - x_lo in the data's dtype; q = x_lo + d t (t < 1/2), q
= x_hi - d (1 - t) otherwise; u = y - q; pinball = tau u (u >= 0), (1 - tau)
(-u) otherwise; below = y < q; tie = y == q.  Float64 after an exact widening,
every operation rounded once.  The point is invalid iff the truth or any
member is NaN.  These are IEEE operations elementwise, so the per-point values
are IDENTICAL on both sides (`point_terms`).  What differs is the weighted sum
over the points: here both sums of a cell are EXACTLY ROUNDED (math.fsum).

The table of a cell (outer index, region) with the dense weights W[i, j], per
level and term v in (pinball, q, below, tie):

  sum over the valid points of W v  /  sum over the valid points of W

skipna=False: a cell with invalid mass is NaN.  skipna=True: the invalid
points are left out.  A cell without valid mass is NaN.

The bound of the tests (u = 2**-53), first order, RELATIVE TO THE MEAN OF |v|
(`dense_table` returns it as the scale; for pinball, below and tie, which are
non-negative, it is the value itself, for q it is the weighted mean of |q|):
  - the product's numerator.  The chain of a (row, class) adds at most n_col
    terms: (n_col - 1) u.  The class fold rounds float(mult) * sum (1; exact
    for the multiplicities 0, 1, 2) and adds n_class of them (n_class - 1):
    n_class u.  The row fold rounds wrow_i * s_i (1) and adds the n_row rows
    (n_row - 1): n_row u.  Together (n_col + n_row + n_class - 1) u.  (below
    and tie: the class sums are exact integers: n_row u alone.)
  - the product's denominator.  The class sum of a row is an exact int64; the
    row fold rounds wrow_i * float(s_i) (1) and adds n_row rows: n_row u.
  - one division: u.
  - the restatement: W v rounded (1), two exactly rounded sums (2), a division
    (1): 4 u.  The dense weights W_ij = w_lat[i] * lat_mult[i] * lon_mult[j]
    are the product's wrow[i] * mult[j]: multiplicities 0, 1, 2 are exact.
  The worst case of these is (n_col + 2 n_row + n_class + 4) u
  (`worst_case_rtol`): the errors of the numerator's and the denominator's row
  folds need not cancel.  The asserted bound is `table_rtol` = (n_col + n_row +
  n_class + 6) u, the smaller wherever n_row > 2, as in
  tests/variogram_np.py: a recursive sum of n terms meets its (n - 1) u only
  when every rounding errs the same way, and here two independent chains of
  n_row roundings would have to, in opposite directions, on top of a column
  chain at its own worst.  (For below and tie the worst case is (2 n_row + 5)
  u, below `table_rtol` on every grid of the tests: n_row <= n_col.)  The
  tests assert `table_rtol` and print the worst observed fraction of it.  Its
  constant 6 is CHOSEN on that argument, not derived; what is derived is
  `worst_case_rtol`.

The CRPS identity (`crps_identity_tol`).  With 'hazen' levels tau_i = (i - 1/2)
/ M, i = 1 .. M, the position is i - 1 and q = x_(i) in exact arithmetic, and
(2 / M) sum_i pinball_i is the CRPS of the empirical CDF, sum_b alpha_b (b /
M)^2 + beta_b (1 - b / M)^2.  Between `crps_from_quantiles` of the one table
and `crps_decomposition.crps` of the other, first order:
  - each table against its exactly weighted means: `table_rtol` each (all
    terms non-negative), 2 `table_rtol` of the value;
  - the per-point roundings, all on non-negative terms: y - q, tau u and tau
    itself (3 u); alpha, beta as differences (1 u); the weights (b / M)^2, (1
    - b / M)^2 (3 u) and w_l (2 u) and the two weighted sums of M + 1 and M
    terms (M + 1) u each: (2 M + 12) u of the value;
  - the host's position.  tau_i is rounded (u tau_i), M tau_i is rounded, the
    subtraction of 1/2 is exact or rounded: |v - (i - 1)| <= 3 M u.  So q is
    off x_(i) by at most 3 M u times the gap to the neighbouring member, which
    is at most the range R of the data; pinball is Lipschitz in q with
    constant max(tau, 1 - tau) <= 1, and 2 sum_l w_l = 2: 6 M u R ABSOLUTE.
  `crps_identity_tol` returns (rtol, atol) = (2 table_rtol + (2 M + 12) u,
  6 M u R).
"""
import math

import numpy as np

U = 2.0 ** -53


def positions(levels, n_member, method):
  """(lo int64, hi int64, t float64) [L] of the levels among `n_member`
  sorted members."""
  tau = np.asarray(levels, dtype=np.float64)
  m = float(n_member)
  v = {'linear': tau * (m - 1.0), 'hazen': m * tau - 0.5,
       'weibull': (m + 1.0) * tau - 1.0}[method]
  v = np.clip(v, 0.0, m - 1.0)
  lo = np.floor(v)
  return (lo.astype(np.int64),
          np.minimum(lo.astype(np.int64) + 1, n_member - 1), v - lo)


def point_terms(ens, truth, levels, method):
  """(pinball, q float64 [O, R, C, L], below, tie bool likewise, ok bool [O,
  R, C]); ens [M, O, R, C], truth [O, R, C].  The values of an invalid point
  are NaN or arbitrary."""
  ens, truth = np.asarray(ens), np.asarray(truth)
  tau = np.asarray(levels, dtype=np.float64)
  lo, hi, t = positions(tau, ens.shape[0], method)
  ok = ~(np.isnan(truth) | np.isnan(ens).any(axis=0))
  s = np.sort(ens, axis=0)
  y = truth.astype(np.float64)
  out = [np.empty(truth.shape + (tau.size,)) for _ in range(2)]
  flags = [np.empty(truth.shape + (tau.size,), dtype=bool) for _ in range(2)]
  with np.errstate(all='ignore'):
    for l in range(tau.size):
      a, b = s[lo[l]], s[hi[l]]
      d = b - a
      assert d.dtype == ens.dtype
      d = d.astype(np.float64)
      if t[l] < 0.5:
        q = a.astype(np.float64) + d * t[l]
      else:
        q = b.astype(np.float64) - d * (1.0 - t[l])
      u = y - q
      out[0][..., l] = np.where(u >= 0, tau[l] * u, (1.0 - tau[l]) * (-u))
      out[1][..., l] = q
      flags[0][..., l] = y < q
      flags[1][..., l] = y == q
  return out[0], out[1], flags[0], flags[1], ok


def dense_counts(ens, truth, col_class, n_class, levels, method):
  """(int64 [O, R, n_class, L, 2] below and tie among the valid points, int64
  [O, R, n_class, 2] valid and invalid points) of every (outer index, row,
  column class)."""
  _, _, below, tie, ok = point_terms(ens, truth, levels, method)
  n_outer, n_row, _ = ok.shape
  cnt = np.zeros((n_outer, n_row, n_class, below.shape[-1], 2), dtype=np.int64)
  valid = np.zeros((n_outer, n_row, n_class, 2), dtype=np.int64)
  cls = np.asarray(col_class, dtype=np.int64)
  for c in range(n_class):
    at = cls == c
    good = ok[:, :, at]
    cnt[:, :, c, :, 0] = (below[:, :, at] & good[..., None]).sum(axis=2)
    cnt[:, :, c, :, 1] = (tie[:, :, at] & good[..., None]).sum(axis=2)
    valid[:, :, c, 0] = good.sum(axis=-1)
    valid[:, :, c, 1] = (~good).sum(axis=-1)
  return cnt, valid


def dense_table(ens, truth, weights, levels, method, skipna):
  """(table, scale) float64 [O, 4, L]: the table of one region with the dense
  weights [R, C], both sums exactly rounded, and the weighted mean of |v| that
  the bound is relative to."""
  w = np.asarray(weights, dtype=np.float64)
  terms = point_terms(ens, truth, levels, method)
  ok = terms[4]
  n_outer, n_level = ok.shape[0], terms[0].shape[-1]
  out = np.full((n_outer, 4, n_level), np.nan)
  scale = np.full((n_outer, 4, n_level), np.nan)
  for o in range(n_outer):
    mass = math.fsum(w[ok[o]])
    lost = math.fsum(w[~ok[o]])
    if mass == 0 or (not skipna and lost != 0):
      continue
    for k in range(4):
      for l in range(n_level):
        v = terms[k][o][..., l][ok[o]].astype(np.float64)
        out[o, k, l] = math.fsum(w[ok[o]] * v) / mass
        scale[o, k, l] = math.fsum(w[ok[o]] * np.abs(v)) / mass
  return out, scale


def winkler(ens, truth, tau, method):
  """(score float64 [O, R, C], covered bool likewise, ok) of the central
  interval (tau, 1 - tau) per point, from its definition: width + (2 / alpha)
  (distance of the truth outside), alpha = 2 tau; covered = q_lo <= y <=
  q_hi."""
  _, q, _, _, ok = point_terms(ens, truth, (tau, 1.0 - tau), method)
  y = np.asarray(truth).astype(np.float64)
  lo, hi = q[..., 0], q[..., 1]
  with np.errstate(all='ignore'):
    score = (hi - lo) + (np.maximum(lo - y, 0.0) + np.maximum(y - hi, 0.0)
                         ) / tau
    covered = (lo <= y) & (y <= hi)
  return score, covered, ok


def table_rtol(n_row, n_col, n_class):
  return (n_col + n_row + n_class + 6) * U


def worst_case_rtol(n_row, n_col, n_class):
  return (n_col + 2 * n_row + n_class + 4) * U


def crps_identity_tol(n_row, n_col, n_class, n_member, data_range):
  return (2 * table_rtol(n_row, n_col, n_class) + (2 * n_member + 12) * U,
          6 * n_member * U * data_range)
