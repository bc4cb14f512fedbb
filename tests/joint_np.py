"""NumPy restatement of weatherbench2_amd/distribution.py: dense, per point,
float64, nothing from the package.

E edges give B = E + 1 categories.  One grid point with truth y and the members
x_0 .. x_{M-1}, float64 after an exact widening:

  bin(v) = np.searchsorted(edges, v, side)   ('right': #{k : e_k <= v};
                                              'left':  #{k : e_k <  v})
  The point is invalid iff the truth or any member is NaN.
  A valid point adds 1 to code = bin(y) * B + bin(x_m) for every member m, an
  invalid one adds 1 to code B * B.

The comparisons are exact, so the codes -- and with them every integer count --
are IDENTICAL on both sides: the tests assert the counts for equality
(`dense_counts`, np.add.at into int64).  What differs is the weighted sum over
the points: here both sums of a cell are EXACTLY ROUNDED (math.fsum).

The table of a cell (outer index, region) with the dense weights W[i, j]:

  p[o][f] = sum_{valid points, members m} W 1[bin(y) = o] 1[bin(x_m) = f]
            / sum_{valid points, members m} W

(the denominator is M x the valid mass).  skipna=False: a cell with invalid
mass is NaN.  skipna=True: invalid points are left out, a cell without valid
mass is NaN.

The bound of the tests (u = 2**-53; every term is non-negative, so it is
RELATIVE to the value): `table_rtol` = (n_row + n_class + 4) u, first order.
  - the product's numerator.  The class sum of a row is an exact int64; the row
    fold rounds wrow_i * float(s_i) (1) and adds the n_row rows (n_row - 1):
    within n_row u of the exact N.
  - the product's denominator.  The exactly rounded sum (1) of B * B folded
    codes, each within n_row u and all non-negative: within (n_row + 1) u.
  - one division: u.
  - the restatement: two exactly rounded sums and a division, 3 u.  The dense
    weights W_ij = w_lat[i] * lat_mult[i] * lon_mult[j] are the product's
    wrow[i] * mult[j]: multiplicities 0, 1, 2 are exact factors.
  The worst case of these is (2 n_row + 5) u (`worst_case_rtol`): the errors of
  the numerator's and the denominator's recursive sums need not cancel.  The
  asserted bound is the smaller (n_row + n_class + 4) u wherever n_row > n_class
  + 1: a recursive sum of n non-negative terms meets its (n - 1) u only when
  every rounding errs the same way, and the fold's roundings of the numerator
  are among the denominator's.  The tests assert `table_rtol` and print the
  worst observed fraction of it.
"""
import math

import numpy as np

U = 2.0 ** -53


def point_bins(v, edges, side):
  """int category of every element of `v` (0 where it is NaN)."""
  v = np.asarray(v).astype(np.float64)
  e = np.asarray(edges, dtype=np.float64).reshape(-1)
  return np.searchsorted(e, np.where(np.isnan(v), -np.inf, v), side=side)


def valid_points(ens, truth):
  """bool [O, R, C] of ens [M, O, R, C] and truth [O, R, C]."""
  return ~(np.isnan(np.asarray(truth)) | np.isnan(np.asarray(ens)).any(axis=0))


def dense_counts(ens, truth, col_class, n_class, edges, side):
  """int64 [O, R, n_class, B * B + 1]: the counts of every (outer index, row,
  column class) by np.add.at."""
  ens, truth = np.asarray(ens), np.asarray(truth)
  n_member, n_outer, n_row, n_col = ens.shape
  n_bin = len(np.asarray(edges).reshape(-1)) + 1
  out = np.zeros((n_outer, n_row, n_class, n_bin * n_bin + 1), dtype=np.int64)
  ok = valid_points(ens, truth)
  yb = point_bins(truth, edges, side)
  xb = point_bins(ens, edges, side)
  o, r, c = np.meshgrid(np.arange(n_outer), np.arange(n_row),
                        np.asarray(col_class, dtype=np.int64), indexing='ij')
  np.add.at(out, (o[~ok], r[~ok], c[~ok], n_bin * n_bin), 1)
  for m in range(n_member):
    np.add.at(out, (o[ok], r[ok], c[ok], (yb * n_bin + xb[m])[ok]), 1)
  return out


def dense_table(ens, truth, weights, edges, side, skipna):
  """float64 [O, B, B]: the table of one region with the dense weights [R, C],
  both sums exactly rounded."""
  ens, truth = np.asarray(ens), np.asarray(truth)
  n_member = ens.shape[0]
  n_bin = len(np.asarray(edges).reshape(-1)) + 1
  w = np.asarray(weights, dtype=np.float64)
  ok = valid_points(ens, truth)
  yb = point_bins(truth, edges, side)
  xb = point_bins(ens, edges, side)
  out = np.full((truth.shape[0], n_bin, n_bin), np.nan)
  for o in range(truth.shape[0]):
    mass = math.fsum(w[ok[o]])
    lost = math.fsum(w[~ok[o]])
    if mass == 0 or (not skipna and lost != 0):
      continue
    # one entry per (member, valid point): its weight and its code
    each = np.broadcast_to(w, (n_member,) + w.shape)[:, ok[o]].reshape(-1)
    code = (yb[o][None] * n_bin + xb[:, o])[:, ok[o]].reshape(-1)
    total = math.fsum(each)
    out[o] = 0.0
    for k in np.unique(code):
      out[o, k // n_bin, k % n_bin] = math.fsum(each[code == k]) / total
  return out


def table_rtol(n_row, n_class):
  return (n_row + n_class + 4) * U


def worst_case_rtol(n_row):
  return (2 * n_row + 5) * U
