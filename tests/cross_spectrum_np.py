"""NumPy restatement of weatherbench2_amd/spectral.py: dense, float64,
`np.fft.rfft`, nothing from the package.

Per outer index o, latitude row i and member m (M members), N = n_lon, NB = N
/ 2 + 1, F_m = rfft(forecast row, norm='forward'), T = rfft(truth row,
norm='forward'), s_0 = 1, s_k = 2 otherwise (Nyquist too), C_i = cos(lat_i pi
/ 180) 2 pi R:

  power_forecast[k] = sum_m s_k C_i |F_m[k]|^2
  power_truth[k]    =       s_k C_i |T[k]|^2
  cospectrum[k]     = sum_m s_k C_i Re(F_m[k] conj T[k])
  quadrature[k]     = sum_m s_k C_i Im(F_m[k] conj T[k])

A row is invalid iff the truth row or any member row holds a non-finite value;
it enters as 0 in every term.  The table of a cell (o, region) with the dense
weights W[i, j] is sum_ij W_ij term_i / sum_{valid i, j} W_ij, the member sums
divided by M.  skipna=False: a cell with invalid mass is NaN; skipna=True: a
cell without valid mass is NaN.

Bounds (`row_bounds`), with tol the project's spectrum tolerance (2e-6 for
float32 rows, 1e-12 for float64 ones: tests/test_spectrum_gpu.py), per row:
* a power term is within tol * sum_k |term[k]|;
* cospectrum and quadrature are within 2 tol sum_m sqrt(sum_k pf_m[k] sum_k
  pt[k]): two transforms that each meet tol relative to their own power, the
  product rule on F_m conj T, on the Cauchy-Schwarz scale, summed over the
  members as the terms are.
"""
import numpy as np

EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2  # schema.py:59
TOL = {np.dtype(np.float32): 2e-6, np.dtype(np.float64): 1e-12}
TERMS = ('power_forecast', 'power_truth', 'cospectrum', 'quadrature')


def circumference(lat):
  return np.cos(np.asarray(lat, np.float64) * np.pi / 180
                ) * 2 * np.pi * EARTH_RADIUS_M


def row_sums(ens, truth, lat):
  """(sums float64 [O, R, 4, NB] -- the member sums NOT divided by M, invalid
  rows 0 --, bad bool [O, R], cross_scale [O, R] = sum_m sqrt(sum_k pf_m sum_k
  pt)) of `ens` [M, O, R, C] and `truth` [O, R, C]."""
  x = np.asarray(ens, dtype=np.float64)
  y = np.asarray(truth, dtype=np.float64)
  n_col = y.shape[-1]
  n_bin = n_col // 2 + 1
  s = np.full(n_bin, 2.0)
  s[0] = 1.0
  scale = s[None, :] * circumference(lat)[:, None]      # [R, NB]
  bad = ~(np.isfinite(y).all(axis=-1) & np.isfinite(x).all(axis=(0, -1)))
  with np.errstate(all='ignore'):
    tt = np.fft.rfft(y, axis=-1, norm='forward')        # [O, R, NB]
    ff = np.fft.rfft(x, axis=-1, norm='forward')        # [M, O, R, NB]
    pt = np.abs(tt) ** 2 * scale
    pf_m = np.abs(ff) ** 2 * scale
    cross = ff * np.conj(tt)[None] * scale
    sums = np.stack([pf_m.sum(axis=0), pt, cross.real.sum(axis=0),
                     cross.imag.sum(axis=0)], axis=-2)
    cross_scale = np.sqrt(pf_m.sum(axis=-1) * pt.sum(axis=-1)[None]
                          ).sum(axis=0)
  sums[bad] = 0.0
  cross_scale[bad] = 0.0
  return sums, bad, cross_scale


def row_bounds(sums, cross_scale, dtype):
  """float64 [O, R, 4]: the bound of every term of every row."""
  tol = TOL[np.dtype(dtype)]
  power = tol * np.abs(sums).sum(axis=-1)               # [O, R, 4]
  out = power.copy()
  out[..., 2] = out[..., 3] = 2 * tol * cross_scale
  return out


def dense_table(ens, truth, lat, weights, skipna):
  """float64 [O, 4, NB] of one region with the dense weights `weights` [R,
  C]."""
  sums, bad, _ = row_sums(ens, truth, lat)
  n_member = np.asarray(ens).shape[0]
  sums = sums.copy()
  sums[:, :, (0, 2, 3)] /= float(n_member)
  wrow = np.asarray(weights, np.float64).sum(axis=1)    # [R]
  total = np.einsum('i,oitk->otk', wrow, sums)
  valid = (wrow[None] * ~bad).sum(axis=1)               # [O]
  invalid = (wrow[None] * bad).sum(axis=1)
  with np.errstate(all='ignore'):
    out = total / valid[:, None, None]
  dead = valid == 0.0
  if not skipna:
    dead = dead | (invalid != 0.0)
  out[dead] = np.nan
  return out


def table_scale(table):
  """float64 [..., 4]: the scale a table entry's error is relative to: sum_k
  |term| for the powers, sqrt(sum pf sum pt) for the cross terms."""
  power = np.abs(table).sum(axis=-1)
  out = power.copy()
  out[..., 2] = out[..., 3] = np.sqrt(power[..., 0] * power[..., 1])
  return out
