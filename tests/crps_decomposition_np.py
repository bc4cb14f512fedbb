"""NumPy restatement of weatherbench2_amd/crps_decomposition.py: per-point
loops, np.sort and float64, nothing from the package.

One grid point with truth y and the members sorted x_1 <= ... <= x_M (float64
after an exact widening), bins i = 0 .. M, p_i = i / M:

  i = 0        alpha = 0                      beta = max(x_1 - y, 0)
  i = M        alpha = max(y - x_M, 0)        beta = 0
  0 < i < M    c = min(max(y, x_i), x_{i+1})  alpha = c - x_i, beta = x_{i+1} - c
  below = [y < x_1], above = [y > x_M] (strict).
  The point is invalid iff the truth or any member is NaN.

The table of a cell is the weighted mean over its valid points of alpha_i,
beta_i, below (in outlier[0]) and above (in outlier[M]) with the dense weights
W[i, j].  skipna=False: a cell with invalid mass is NaN.  skipna=True: invalid
points are left out, a cell without valid mass is NaN.

Bounds used by the tests (u = 2**-53, n = n_lat * n_lon points of a cell):

* dense_table vs the product (`table_rtol`).  Every term W_ij alpha_ij is
  non-negative, and a sum of n non-negative floats in ANY order has relative
  error <= (n - 1) u (Higham, Accuracy and Stability of Numerical Algorithms,
  section 4.2), so two orders differ by 2 n u.  The dense form rounds each
  product W_ij * alpha_ij (1 u); the product rounds wrow * s once per row (1 u;
  the column multiplicities 0, 1, 2 are exact factors): 2 u.  The valid mass in
  the denominator is such a sum too (2 n u) and each side divides once (2 u).
  The point terms themselves are the same float64 operations on both sides.
  In all (4 n + 4) u; the tests use rtol = (4 n + 8) u.

* reliability + potential == crps(table) (`identity_atol`).  Algebraically
  bin i gives g_i [(o_i - p_i)^2 + o_i (1 - o_i)] = alpha_i p_i^2 + beta_i (1
  - p_i)^2.  With 0 <= o, p <= 1 the differences o - p and 1 - o carry an
  absolute error of at most u, so each bracket is off by at most 4 u plus its
  own few roundings, each term by at most 8 u g_i o-or-1 (interior bins: g_i =
  alpha_i + beta_i; bin 0: g_0 o_0 = beta_0, every factor of g_0 comes with o_0;
  bin M: g_M (1 - o_M) = alpha_M likewise), and the M + 1 terms of each of the
  three sums add (M + 1) u times the sum of their magnitudes, which is at most
  1.25 G, G = sum_{0<i<M} (alpha_i + beta_i) + beta_0 + alpha_M.  One term is
  different: o_M = 1 - above is ROUNDED (|delta| <= u / 2), and g_M (1 - o_M) =
  alpha_M (above - delta) / above misses alpha_M by alpha_M u / (2 above).
  atol = u ((M + 17) G + alpha_M / above), the last term only where above > 0.

* crps(table, fair=True) vs the oracle's CRPS (`fair_atol`), float64 inputs.
  With S = max over the points and members of |x - y|, every per-point
  quantity is bounded by a small multiple of S: skill <= S, spread <= 2 S, the
  bin widths sum to at most 2 S + S.  The oracle averages skill (M roundings
  per point) and the rank-weighted spread (M terms with weights below M,
  normalised: (M + 2) u 2 S) over n points with the same weights ((n + 2) u);
  the table sums alpha and beta over n points (n u), folds (2 u), divides
  ((n + 2) u), and its final sums over M + 1 bins with the weights p^2, (1 -
  p)^2 and i (M - i) / (M^2 (M - 1)) <= 1 / (4 (M - 1)) add (M + 4) u each.
  Both scores are differences of such quantities (no relative bound holds for
  the result), so the bound is absolute: atol = 3 S (4 n + 8 M + 32) u.
"""
import numpy as np

U = 2.0 ** -53


def point_terms(members, truth):
  """(alpha [M + 1], beta [M + 1], below, above) of one point from scalars, or
  None for an invalid point."""
  m = len(members)
  y = float(truth)
  if y != y or any(float(x) != float(x) for x in members):
    return None
  x = np.sort(np.array([float(v) for v in members], dtype=np.float64))
  alpha, beta = np.zeros(m + 1), np.zeros(m + 1)
  beta[0] = max(x[0] - y, 0.0)
  alpha[m] = max(y - x[m - 1], 0.0)
  for i in range(1, m):
    c = min(max(y, x[i - 1]), x[i])
    alpha[i] = c - x[i - 1]
    beta[i] = x[i] - c
  return alpha, beta, y < x[0], y > x[m - 1]


def point_fields(ens, truth):
  """(terms float64 [O, R, C, 3, M + 1], valid bool [O, R, C]) of ens [M, O, R,
  C] and truth [O, R, C]: one Python step per point; term 2 holds below in bin
  0 and above in bin M; an invalid point is all zeros."""
  n_member = ens.shape[0]
  terms = np.zeros(truth.shape + (3, n_member + 1), dtype=np.float64)
  valid = np.zeros(truth.shape, dtype=bool)
  for idx in np.ndindex(*truth.shape):
    got = point_terms([ens[(m,) + idx] for m in range(n_member)], truth[idx])
    if got is None:
      continue
    alpha, beta, below, above = got
    valid[idx] = True
    terms[idx][0], terms[idx][1] = alpha, beta
    terms[idx][2, 0] += float(below)
    terms[idx][2, n_member] += float(above)
  return terms, valid


def dense_table(terms, valid, weights, skipna):
  """[O, 3, M + 1]: the weighted mean of `point_fields` over the valid points
  with the dense weights [R, C]."""
  w = np.asarray(weights, dtype=np.float64)
  total = np.einsum('orctb,rc->otb', terms, w)
  mass = np.einsum('orc,rc->o', valid.astype(np.float64), w)
  lost = np.einsum('orc,rc->o', (~valid).astype(np.float64), w)
  with np.errstate(all='ignore'):
    out = total / mass[:, None, None]
  dead = mass == 0
  if not skipna:
    dead = dead | (lost != 0)
  out[dead] = np.nan
  return out


def crps_of_table(p, fair=False):
  """The CRPS of a table [..., 3, M + 1], bin by bin."""
  m = p.shape[-1] - 1
  value = np.zeros(p.shape[:-2])
  for i in range(m + 1):
    pi = i / m
    value = value + p[..., 0, i] * pi ** 2 + p[..., 1, i] * (1 - pi) ** 2
    if fair and 0 < i < m:
      value = value - i * (m - i) * (p[..., 0, i] + p[..., 1, i]) / (
          m * m * (m - 1))
  if fair and m == 1:
    value = value * np.nan
  return value


def table_rtol(n_point):
  return (4 * n_point + 8) * U


def identity_atol(p):
  """The bound of reliability + potential == crps for a table [..., 3, M + 1]
  (NaN cells give NaN)."""
  m = p.shape[-1] - 1
  big = p[..., 0, 1:m].sum(-1) + p[..., 1, 1:m].sum(-1) + p[..., 1, 0] + (
      p[..., 0, m])
  above = p[..., 2, m]
  with np.errstate(all='ignore'):
    tail = np.where(above > 0, p[..., 0, m] / above, 0.0)
  return U * ((m + 17) * big + tail)


def fair_atol(ens, truth, n_point):
  m = ens.shape[0]
  with np.errstate(invalid='ignore'):
    s = np.nanmax(np.abs(ens - truth[None]))
  return 3 * s * (4 * n_point + 8 * m + 32) * U
