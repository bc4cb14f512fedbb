"""NumPy restatement of weatherbench2_amd/threshold_weighted.py: dense, per
point, float64, nothing from the package.

One grid point with truth y, members sorted x_1 <= ... <= x_M and threshold t
(float64 after an exact widening); v(z) = max(z, t) for tail 'upper', min(z, t)
for 'lower':

  A = sum_{i=1..M} |v(x_i) - v(y)|
  B = sum_{k=1..M-1} k (M - k) (v(x_{k+1}) - v(x_k)),   B = 0 for M = 1
      (the gap form of sum_{i<j} |v(x_i) - v(x_j)|: every term >= 0, the
      integer factor exact, a gap wholly beyond the threshold exactly 0)
  The point is invalid FOR THRESHOLD t iff the truth, any member or t is NaN.
  t = -inf (upper) and t = +inf (lower) are ordinary: the plain CRPS terms.

The table of a cell (threshold, outer index, region) is, with the dense weights
W[i, j], abs_error = the weighted mean over the valid points of A / M and
pair_distance = that of B / M^2.  skipna=False: a cell with invalid mass for
the threshold is NaN.  skipna=True: invalid points are left out, a cell
without valid mass is NaN.

Here A is added in the GIVEN member order (not the sorted one), B in increasing
k over np.sort, and the weighted sums of a cell are EXACTLY ROUNDED
(math.fsum), so that the restatement's own summation error is O(1) roundings
and the bound below is that of the product's order.

Bounds used by the tests (u = 2**-53, n = n_lat * n_lon points of a cell, M
members).  All first-order in u; all summands are non-negative, so every bound
is RELATIVE to the value (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2: a sum of k non-negative floats in any order has
relative error <= (k - 1) u).

* dense_table vs the product (`table_rtol` = (n + 2 M + 12) u), for grids with
  n_lon >= 2:
  - the point terms.  A: each |v(x_i) - v(y)| is one rounding (the clamps are
    exact), the sum of M of them adds (M - 1) u: M u on either side, in either
    order.  B: a gap (u), its product with the exact integer (u), the sum of
    M - 1 of them ((M - 2) u): M u on either side.  The two sides' point terms
    differ by at most 2 M u.
  - the product's sums.  The column chain of a (row, class) adds n_c - 1
    roundings for its n_c columns; the class fold multiplies by 0, 1 or 2
    (exact) and adds the n_class classes (n_class - 1); the classes partition
    the columns and none is empty, so n_c + n_class - 2 <= n_lon - 1.  The row
    fold rounds wrow * s (1) and adds n_lat rows (n_lat - 1).  Numerator: (n_lon
    + n_lat - 1) u.  The valid mass is sum_i wrow_i * float(count_i) with exact
    integer counts: n_lat u.  The divisions by the mass and by M (or M^2; M^2 <=
    4096 is exact): 2 u.  In all (n_lon + 2 n_lat + 1) u <= (n + 3) u, because
    n - n_lon - 2 n_lat + 2 = (n_lat - 1) (n_lon - 2) >= 0 for n_lon >= 2.
  - the restatement's sums.  The products W_ij * term (u, relative, all of one
    sign), the exactly rounded sum (u), the exactly rounded mass (u), the
    divisions by the mass and by M or M^2 (2 u): 5 u.  The dense weights W_ij
    = w_lat[i] * lat_mult[i] * lon_mult[j] are the product's wrow[i] * mult[j]
    (multiplicities 0, 1, 2 are exact factors).
  Sum: (n + 2 M + 8) u; the neglected second-order terms are below (k u)^2 <
  u for k < 2^26, far above any n + 2 M here: c = 8 + 4 = 12 leaves four
  roundings for them and for the two sides' different (but equally exact)
  routes to W_ij.

* twcrps(table, fair=True) vs the oracle's CRPS in the plain limit
  (`fair_atol`): K20's derivation (tests/crps_decomposition_np.py) carries over
  term by term -- the oracle's side is the same; the table's side has FEWER
  roundings here (n + 3 instead of 2 n + 4 for the sums, M instead of M + 4 for
  the point terms, no sum over M + 1 bins) -- so K20's bound holds unchanged:
  atol = 3 S (4 n + 8 M + 32) u with S = max |x - y|.  The result is a
  difference (no relative bound holds for it), hence absolute.

* twcrps(table) vs crps_decomposition.crps(CRPSTable) (`plain_atol`): both
  estimate E|X - y| - E|X - X'| / 2 with the M^2 spread from the same points;
  each is within its own absolute bound of the exact value: K20's side 3 S (4 n
  + 8 M + 32) u as above (its `crps` is the sum over the bins that the fair
  form only corrects), this side (n + 2 M + 12) u times abs_error +
  pair_distance <= 3 S.  The sum of the two.

* upper + lower == plain (`tails_atol`): max(z, t) + min(z, t) = z + t, so for
  any a, b: |max(a,t) - max(b,t)| + |min(a,t) - min(b,t)| = |a - b| (both
  differences have the sign of a - b).  Term by term the three tables hold
  means of non-negative quantities over the same valid points, each within
  (n + 2 M + 12) u of its exact value, relative: the bound is that times (upper
  + lower + plain), per term.
"""
import math

import numpy as np

U = 2.0 ** -53


def point_terms(members, truth, threshold, tail='upper'):
  """(A, B) of one point from scalars, or None where the point is invalid for
  the threshold."""
  m = len(members)
  y, t = float(truth), float(threshold)
  xs = [float(v) for v in members]
  if y != y or t != t or any(x != x for x in xs):
    return None
  clamp = (lambda z: max(z, t)) if tail == 'upper' else (lambda z: min(z, t))
  vy = clamp(y)
  a = 0.0
  for x in xs:  # the given order
    a = a + abs(clamp(x) - vy)
  v = [clamp(x) for x in sorted(xs)]
  b = 0.0
  for k in range(1, m):
    b = b + k * (m - k) * (v[k] - v[k - 1])
  return a, b


def pair_sum(members, threshold, tail='upper'):
  """sum_{i<j} |v(x_i) - v(x_j)| written out: what B is the gap form of."""
  t = float(threshold)
  clamp = (lambda z: max(z, t)) if tail == 'upper' else (lambda z: min(z, t))
  v = [clamp(float(x)) for x in members]
  return sum(abs(v[i] - v[j]) for i in range(len(v))
             for j in range(i + 1, len(v)))


def point_fields(ens, truth, threshold, tail='upper'):
  """(terms float64 [O, R, C, 2], valid bool [O, R, C]) of ens [M, O, R, C],
  truth [O, R, C] and one threshold's values, [O, R, C] or [R, C]: the rules of
  `point_terms`, over the points at once (members in a Python loop); an
  invalid point is all zeros."""
  ens = np.asarray(ens).astype(np.float64)
  y = np.asarray(truth).astype(np.float64)
  t = np.broadcast_to(np.asarray(threshold).astype(np.float64), y.shape)
  m = ens.shape[0]
  valid = ~(np.isnan(y) | np.isnan(t) | np.isnan(ens).any(axis=0))
  x = np.where(valid[None], ens, 0.0)
  y, t = np.where(valid, y, 0.0), np.where(valid, t, 0.0)
  clamp = (lambda z: np.maximum(z, t)) if tail == 'upper' else (
      lambda z: np.minimum(z, t))
  vy = clamp(y)
  a = np.zeros(y.shape)
  for i in range(m):  # the given order
    a = a + np.abs(clamp(x[i]) - vy)
  v = clamp(np.sort(x, axis=0))
  b = np.zeros(y.shape)
  for k in range(1, m):
    b = b + k * (m - k) * (v[k] - v[k - 1])
  terms = np.stack([a, b], axis=-1)
  terms[~valid] = 0.0
  return terms, valid


def dense_table(terms, valid, weights, n_member, skipna):
  """[O, 2]: (abs_error, pair_distance), the weighted means of A / M and
  B / M^2 of `point_fields` over the valid points with the dense weights [R,
  C]; every sum exactly rounded."""
  w = np.asarray(weights, dtype=np.float64)
  out = np.full((terms.shape[0], 2), np.nan)
  for o in range(terms.shape[0]):
    ok = valid[o]
    mass = math.fsum(w[ok])
    lost = math.fsum(w[~ok])
    if mass == 0 or (not skipna and lost != 0):
      continue
    out[o, 0] = math.fsum((w * terms[o, ..., 0])[ok]) / mass / n_member
    out[o, 1] = math.fsum((w * terms[o, ..., 1])[ok]) / mass / (
        n_member * n_member)
  return out


def table_rtol(n_lat, n_lon, n_member):
  assert n_lon >= 2  # (the derivation above)
  return (n_lat * n_lon + 2 * n_member + 12) * U


def fair_atol(ens, truth, n_point):
  """K20's bound of the fair CRPS of a table against the oracle's CRPS."""
  m = ens.shape[0]
  with np.errstate(invalid='ignore'):
    s = np.nanmax(np.abs(ens.astype(np.float64) -
                         truth.astype(np.float64)[None]))
  return 3 * s * (4 * n_point + 8 * m + 32) * U


def plain_atol(ens, truth, n_lat, n_lon, table):
  """|twcrps(plain table) - crps(CRPSTable)|: the two modules' bounds."""
  m = ens.shape[0]
  mine = table_rtol(n_lat, n_lon, m) * (table[..., 0] + table[..., 1])
  return fair_atol(ens, truth, n_lat * n_lon) + mine


def tails_atol(n_lat, n_lon, n_member, upper, lower, plain):
  return table_rtol(n_lat, n_lon, n_member) * (upper + lower + plain)
