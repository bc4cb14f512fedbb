"""NumPy restatement of weatherbench2_amd/conditional.py: dense, per point,
float64, nothing from the package.

One grid point with truth y and the members x_0 .. x_{M-1} in STORAGE order,
float64 after an exact widening, every operation rounded on its own (NumPy has
no fused multiply-add):

  S = x_0; S = S + x_m (m = 1 .. M-1);  mu = S / M
  d_m = x_m - mu;  Q = d_0 d_0;  Q = Q + d_m d_m;  s2 = Q / (M - 1)
  (M = 1: s2 = +0.0);  e = mu - y;  se = e e
  v = s2 (by='spread', against the edges SQUARED once in float64), mu
  ('forecast') or y ('truth');  bin = searchsorted(edges, v, side='right')
  The point is invalid iff the truth or any member is NaN.

These are the product's own formulas in the product's own order, so the point
values -- and with them the bin of every point -- are IDENTICAL on both sides,
bit for bit; the tests assert the membership through the exact `weight` counts.
What differs is the summation over the points: here the weighted sums of a cell
are EXACTLY ROUNDED (math.fsum).

The table of a cell (outer index, region) is, with the dense weights W[i, j]
and mass = sum of W over the valid points, per bin b:
  weight = sum_{valid, in b} W / mass,   term = sum_{valid, in b} W v / mass
for v = mu, y, s2, se.  skipna=False: a cell with invalid mass is NaN.
skipna=True: invalid points are left out, a cell without valid mass is NaN.

Bounds used by the tests (u = 2**-53, n = n_lat * n_lon points of a cell, B
bins, M members); all first-order in u.

* dense_table vs the product (`table_atol` = (n + B + 12) u A, with A = sum_{
  valid, in b} W |v| / mass, which `dense_table` returns beside the values; for
  `weight` A is the weight itself), for grids with n_lon >= 2.  mu and y are
  signed, so the bound is relative to the sum of the ABSOLUTE values (Higham,
  Accuracy and Stability of Numerical Algorithms, section 4.2: a recursive sum
  of k floats has error <= (k - 1) u sum |x_i|).
  - the product's sums.  The column chain of a (row, class, bin) adds at most
    n_c - 1 roundings for the n_c columns of the class (the +0.0 of a foreign
    point is exact); the class fold multiplies by 0, 1 or 2 (exact) and adds
    the n_class classes (n_class - 1); the classes partition the columns and
    none is empty, so n_c + n_class - 2 <= n_lon - 1.  The row fold rounds
    wrow * s (1) and adds n_lat rows (n_lat - 1).  Numerator: (n_lon + n_lat -
    1) u A.  The mass of a bin is sum_i wrow_i * float(count_i) with exact
    integer counts (n_lat u) and the valid mass their sum over the B bins
    (B - 1): (n_lat + B - 1) u.  One division: u.  In all (n_lon + 2 n_lat + B
    - 1) u <= (n + B + 1) u, because n - n_lon - 2 n_lat + 2 = (n_lat - 1)
    (n_lon - 2) >= 0 for n_lon >= 2.  For `weight` the numerator is a bin's
    mass (n_lat u): fewer.
  - the restatement's sums.  The products W_ij * v (u, relative to |W v|), the
    exactly rounded sum (u), the exactly rounded mass (u), the division (u):
    4 u.  The dense weights W_ij = w_lat[i] * lat_mult[i] * lon_mult[j] are the
    product's wrow[i] * mult[j] (multiplicities 0, 1, 2 are exact factors).
  Sum: (n + B + 5) u A; the neglected second-order terms are below (k u)^2 < u
  for k < 2^26: const = B + 12 leaves seven roundings for them and for the two
  sides' different (but equally exact) routes to W_ij.

* `marginal(table)` vs the oracle's EnsembleVariance, EnsembleMeanMSE and Bias
  with FLOAT64 inputs (`marginal_atol`).  Z = max(|x|, |y|) over the case.
  - the point values.  A mean of M values in any order is within M u Z of the
    exact mean (M - 1 additions relative to sum |x_m| <= M Z, then the
    division): the two sides' means differ by <= 2 M u Z.  bias = mean - y
    rounds once more on either side (|mean - y| <= 2 Z): 2 (M + 2) u Z.
    se = e e with |e| <= 2 Z: d(se) <= 2 |e| d(e) + u e^2 <= (4 M + 12) u Z^2
    a side, (8 M + 24) u Z^2 between them.  s2: d_m = x_m - mean, |d_m| <= 2 Z,
    carries the mean's error and a rounding, (M + 2) u Z; d_m^2 then (4 M + 12)
    u Z^2; the sum of M of them adds (M - 1) u * 4 M Z^2 and the division u * 4
    M Z^2 / (M - 1); divided by M - 1 and with M / (M - 1) <= 2: s2 is within 2
    (4 M + 12 + 4 M) u Z^2 = (16 M + 24) u Z^2 a side, (32 M + 48) u Z^2
    between them.
  - the averages.  Every value is bounded by V = 4 Z^2 (s2, se) or 2 Z (bias).
    The table's side: each bin within (n + B + 12) u A_b of the exact weighted
    mean of indicator x value, sum_b A_b <= V; the sum over the bins in
    `marginal` adds (B - 1) u V: (n + 2 B + 11) u V.  The oracle's side is a
    weighted mean of n values with normalised weights: the weights' mean (n u),
    their division (u), the products (u) and the mean of n terms (n u): (2 n +
    2) u V.  Together (3 n + 2 B + 13) u V <= (3 n + 2 B + 16) u V.
  atol = point term + (3 n + 2 B + 16) u V.
"""
import math

import numpy as np

U = 2.0 ** -53
TERMS = ('weight', 'forecast', 'truth', 'variance', 'squared_error')


def squared_edges(edges, by):
  e = np.asarray(edges, dtype=np.float64).reshape(-1)
  return e * e if by == 'spread' else e


def point_fields(ens, truth):
  """(mu, s2, se float64 [O, R, C], valid bool [O, R, C]) of ens [M, O, R, C]
  and truth [O, R, C]: the formulas above, members in a Python loop in storage
  order."""
  x = np.asarray(ens).astype(np.float64)
  y = np.asarray(truth).astype(np.float64)
  m = x.shape[0]
  valid = ~(np.isnan(y) | np.isnan(x).any(axis=0))
  with np.errstate(all='ignore'):
    s = x[0]
    for k in range(1, m):
      s = s + x[k]
    mu = s / m
    d = x[0] - mu
    q = d * d
    for k in range(1, m):
      d = x[k] - mu
      q = q + d * d
    s2 = q / (m - 1) if m > 1 else np.zeros_like(q)
    e = mu - y
    se = e * e
  return mu, s2, se, valid


def point_bins(ens, truth, edges, by):
  """int [O, R, C] bin of every point (0 where it is invalid)."""
  mu, s2, _, valid = point_fields(ens, truth)
  v = {'spread': s2, 'forecast': mu,
       'truth': np.asarray(truth).astype(np.float64)}[by]
  return np.searchsorted(squared_edges(edges, by), np.where(valid, v, 0.0),
                         side='right')


def dense_table(ens, truth, weights, edges, by, skipna):
  """(values, scales), each [O, 5, B]: the table of one region with the dense
  weights [R, C], every sum exactly rounded, and per element A = sum W |v| /
  mass, the scale of the bound."""
  mu, s2, se, valid = point_fields(ens, truth)
  which = point_bins(ens, truth, edges, by)
  n_bin = len(np.asarray(edges).reshape(-1)) + 1
  w = np.asarray(weights, dtype=np.float64)
  y = np.asarray(truth).astype(np.float64)
  out = np.full((y.shape[0], len(TERMS), n_bin), np.nan)
  scale = np.full(out.shape, np.nan)
  for o in range(y.shape[0]):
    ok = valid[o]
    mass = math.fsum(w[ok])
    lost = math.fsum(w[~ok])
    if mass == 0 or (not skipna and lost != 0):
      continue
    for b in range(n_bin):
      sel = ok & (which[o] == b)
      out[o, 0, b] = scale[o, 0, b] = math.fsum(w[sel]) / mass
      for k, v in enumerate((mu[o], y[o], s2[o], se[o])):
        out[o, 1 + k, b] = math.fsum((w * v)[sel]) / mass
        scale[o, 1 + k, b] = math.fsum((w * np.abs(v))[sel]) / mass
  return out, scale


def table_atol(n_lat, n_lon, n_bin, scale):
  assert n_lon >= 2  # (the derivation above)
  return (n_lat * n_lon + n_bin + 12) * U * scale


def marginal_atol(ens, truth, n_point, n_bin):
  """{'variance', 'squared_error', 'bias': atol} of `marginal(table)` against
  the oracle's metrics on float64 inputs."""
  m = ens.shape[0]
  z = max(np.nanmax(np.abs(ens.astype(np.float64))),
          np.nanmax(np.abs(truth.astype(np.float64))))
  avg = (3 * n_point + 2 * n_bin + 16) * U
  return {'variance': (32 * m + 48) * U * z * z + avg * 4 * z * z,
          'squared_error': (8 * m + 24) * U * z * z + avg * 4 * z * z,
          'bias': (2 * m + 4) * U * z + avg * 2 * z}
