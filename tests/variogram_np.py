"""NumPy restatement of weatherbench2_amd/structure.py: dense, per pair,
float64, nothing from the package.

A lag is (a, b), a >= 0 rows and b columns in grid points.  The partner of the
anchor (i, j) is (i + a, (j + b) mod n_col); the pair exists iff i + a < n_row.
One existing pair, truth y, y', members x_m, x'_m in storage order, float64
after an exact widening, every operation rounded once (no fused multiply-add):

  g(d) = |d| (order 1),  d * d (order 2),  sqrt(|d|) (order 0.5)
  gy = g(y - y');  G = g(x_0 - x'_0);  G = G + g(x_m - x'_m);  gf = G / M
  s = gy - gf;  sc = s * s

The pair is invalid iff any of y, y', x_m, x'_m is NaN.  These are IEEE
operations elementwise, so the per-pair values are IDENTICAL on both sides
(`pair_terms`), and all three are non-negative.  What differs is the weighted
sum over the pairs: here both sums of a cell are EXACTLY ROUNDED (math.fsum).

The table of a cell (outer index, region) with the dense weights W[i, j] of the
ANCHOR, per lag and term v in (gy, gf, sc):

  sum over the valid pairs of W v  /  sum over the valid pairs of W

skipna=False: a cell with invalid mass is NaN.  skipna=True: the invalid pairs
are left out.  A cell without valid mass is NaN.

The bound of the tests (u = 2**-53; every term is non-negative, so it is
RELATIVE to the value), first order:
  - the product's numerator.  The chain of a (row, class) adds at most n_col
    terms: (n_col - 1) u.  The class fold rounds float(mult) * sum (1; exact
    for the multiplicities 0, 1, 2) and adds n_class of them (n_class - 1):
    n_class u.  The row fold rounds wrow_i * s_i (1) and adds the n_row rows
    (n_row - 1): n_row u.  Together (n_col + n_row + n_class - 1) u.
  - the product's denominator.  The class sum of a row is an exact int64; the
    row fold rounds wrow_i * float(s_i) (1) and adds n_row rows: n_row u.
  - one division: u.
  - the restatement: W v rounded (1), two exactly rounded sums (2), a division
    (1): 4 u.  The dense weights W_ij = w_lat[i] * lat_mult[i] * lon_mult[j]
    are the product's wrow[i] * mult[j]: multiplicities 0, 1, 2 are exact.
  The worst case of these is (n_col + 2 n_row + n_class + 4) u
  (`worst_case_rtol`): the errors of the numerator's and the denominator's row
  folds need not cancel.  The asserted bound is `table_rtol` = (n_col + n_row +
  n_class + 6) u, the smaller wherever n_row > 2: a recursive sum of n
  non-negative terms meets its (n - 1) u only when every rounding errs the same
  way, and here two independent chains of n_row roundings would have to, in
  opposite directions, on top of a column chain at its own worst.  The tests
  assert `table_rtol` and print the worst observed fraction of it.
"""
import math

import numpy as np

U = 2.0 ** -53


def g(d, order):
  if order == 1:
    return np.abs(d)
  if order == 2:
    return d * d
  assert order == 0.5
  return np.sqrt(np.abs(d))


def pair_terms(ens, truth, lag, order):
  """(gy, gf, sc float64 [O, n_row - a, C], ok bool likewise) of the pairs of
  `lag` that exist, at their anchors; ens [M, O, R, C], truth [O, R, C].  None
  where no row reaches the lag.  The values of an invalid pair are NaN."""
  a, b = lag
  x = np.asarray(ens).astype(np.float64)
  y = np.asarray(truth).astype(np.float64)
  n_member, _, n_row, n_col = x.shape
  if a >= n_row:
    return None
  n = n_row - a
  partner = (np.arange(n_col) + b) % n_col
  with np.errstate(all='ignore'):
    gy = g(y[:, :n] - y[:, a:][:, :, partner], order)
    total = g(x[0][:, :n] - x[0][:, a:][:, :, partner], order)
    for m in range(1, n_member):
      total = total + g(x[m][:, :n] - x[m][:, a:][:, :, partner], order)
    gf = total / float(n_member)
    s = gy - gf
    sc = s * s
  bad = np.isnan(y) | np.isnan(x).any(axis=0)
  ok = ~(bad[:, :n] | bad[:, a:][:, :, partner])
  return gy, gf, sc, ok


def dense_counts(ens, truth, col_class, n_class, lags):
  """int64 [O, R, n_class, L, 2]: the valid and the invalid pairs of every
  (outer index, anchor row, anchor's column class, lag)."""
  ens, truth = np.asarray(ens), np.asarray(truth)
  _, n_outer, n_row, n_col = ens.shape
  out = np.zeros((n_outer, n_row, n_class, len(lags), 2), dtype=np.int64)
  cls = np.asarray(col_class, dtype=np.int64)
  for l, lag in enumerate(lags):
    terms = pair_terms(ens, truth, lag, 1)
    if terms is None:
      continue
    ok = terms[3]
    for c in range(n_class):
      out[:, :ok.shape[1], c, l, 0] = ok[:, :, cls == c].sum(axis=-1)
      out[:, :ok.shape[1], c, l, 1] = (~ok)[:, :, cls == c].sum(axis=-1)
  return out


def dense_table(ens, truth, weights, lags, order, skipna):
  """float64 [O, 3, L]: the table of one region with the dense weights [R, C],
  both sums exactly rounded."""
  w = np.asarray(weights, dtype=np.float64)
  n_outer = np.asarray(truth).shape[0]
  out = np.full((n_outer, 3, len(lags)), np.nan)
  for l, lag in enumerate(lags):
    terms = pair_terms(ens, truth, lag, order)
    if terms is None:
      continue
    ok = terms[3]
    wa = w[:ok.shape[1]]
    for o in range(n_outer):
      mass = math.fsum(wa[ok[o]])
      lost = math.fsum(wa[~ok[o]])
      if mass == 0 or (not skipna and lost != 0):
        continue
      for k in range(3):
        out[o, k, l] = math.fsum(wa[ok[o]] * terms[k][o][ok[o]]) / mass
  return out


def table_rtol(n_row, n_col, n_class):
  return (n_col + n_row + n_class + 6) * U


def worst_case_rtol(n_row, n_col, n_class):
  return (n_col + 2 * n_row + n_class + 4) * U
