"""The float64 reference shared by the geometry sweeps of the streaming
(test_stream_geometry_gpu.py) and the ensemble reductions
(test_ens_geometry_gpu.py), and the bit-exact references of the map kernels
and running means (test_map_geometry_gpu.py).

Per-point region weights come from oracle/metrics_np.get_lat_weights times
what oracle/regions_np's Region.apply leaves (land fraction included), never
from plan.py; every sum is a math.fsum of the float64 products, so a kernel's
sum may differ from it by its own rounding only: SUM_RTOL * sum|w x|.

The maps are elementwise in the input dtype and the library is built with
-ffp-contract=off, so NumPy's arithmetic in that dtype gives their bits; the
running sums add float64 values one time step after the other, so a float64
loop in time order gives theirs.
"""
import math

import numpy as np

from oracle import metrics_np as om
from oracle.named import DS, NA

SUM_RTOL = 1e-12


def region_weights(region, lat, lon, layout):
  """Per-point weights of `region` as a slab [n_row, n_col] of `layout`:
  latitude weights times Region.apply's weights, scattered back to the points
  the region selected (a point selected twice counts twice)."""
  n_lat, n_lon = len(lat), len(lon)
  idx = NA(np.arange(n_lat * n_lon, dtype=np.float64).reshape(n_lat, n_lon),
           ('latitude', 'longitude'))
  ds = DS({'idx': idx}, {'latitude': lat, 'longitude': lon})
  sub, w = region.apply(ds, om.get_lat_weights(lat))
  where = sub['idx'].transpose('latitude', 'longitude').data
  wfull = (w * (sub['idx'] * 0.0 + 1.0)).transpose('latitude',
                                                    'longitude').data
  out = np.zeros(n_lat * n_lon)
  np.add.at(out, where.astype(np.int64).ravel(), wfull.ravel())
  out = out.reshape(n_lat, n_lon)
  return out if layout == 'latlon' else np.ascontiguousarray(out.T)


def ref_sums(weights, slots):
  """(sums, sums of |w x|) [n_outer, n_region, K] and the regions' weight
  sums [n_region], all with math.fsum."""
  n_outer, k = slots[0].shape[0], len(slots)
  sums = np.zeros((n_outer, len(weights), k))
  mags = np.zeros_like(sums)
  wsum = np.zeros(len(weights))
  for r, w in enumerate(weights):
    m = w != 0
    wm = w[m]
    wsum[r] = math.fsum(wm.tolist())
    for j in range(k):
      for o in range(n_outer):
        p = wm * slots[j][o][m]
        sums[o, r, j] = math.fsum(p.tolist())
        mags[o, r, j] = math.fsum(np.abs(p).tolist())
  return sums, mags, wsum


def assert_sums(got, want, mags, tag):
  """`got` within SUM_RTOL * mags of `want`; NaN exactly where `want` is."""
  tol = SUM_RTOL * mags
  with np.errstate(invalid='ignore'):
    bad = (np.isnan(got) != np.isnan(want)) | (np.abs(got - want) > tol)
  if bad.any():
    o, r, k = np.argwhere(bad)[0]
    raise AssertionError(
        f'{tag}: {int(bad.sum())} sums off, first (outer {o}, region {r}, '
        f'slot {k}): got {got[o, r, k]!r} want {want[o, r, k]!r} '
        f'tol {tol[o, r, k]:.3g}')


def prove_tolerance(weights, slots, sums, mags, o, tile, sign_free):
  """A kernel that dropped the first column of tile 1 (column `tile`), or
  counted the last column twice, would fail SUM_RTOL: shown on the reference
  (global region = weights[0], outer slab `o`) for every slot of `sign_free`
  (slots whose points cannot cancel)."""
  n = weights[0].shape[1]
  perturbed = []
  if n > tile:
    w = weights[0].copy()
    w[:, tile] = 0.0
    perturbed.append(('drop column T', w))
  w = weights[0].copy()
  w[:, n - 1] *= 2.0
  perturbed.append(('last column twice', w))
  for what, w in perturbed:
    s, _, _ = ref_sums([w], [x[o:o + 1] for x in slots])
    off = np.abs(s[0, 0, sign_free] - sums[o, 0, sign_free])
    assert (off > SUM_RTOL * mags[o, 0, sign_free]).all(), (what, off)


# ---- bit-exact references of the map kernels and running means --------------
def spatial_maps(f, t):
  """(bias, mse, mae) = (d, d * d, |d|) with d = f - t, in the input dtype."""
  with np.errstate(all='ignore'):
    d = f - t
    return d, d * d, np.abs(d)


def running_sum(start, steps, skipna, count=None):
  """s = s + float64(x_t) over `steps` in time order, from `start`; a skipped
  (NaN, with skipna) value adds 0.0.  Returns (sum, count): `count` (or None)
  gains one per value kept."""
  s = np.array(start, dtype=np.float64, copy=True)
  c = None if count is None else np.array(count, dtype=np.float64, copy=True)
  for x in steps:
    x = np.asarray(x).astype(np.float64)
    keep = ~np.isnan(x) if skipna else np.ones(x.shape, bool)
    with np.errstate(invalid='ignore'):  # inf + -inf
      s = s + np.where(keep, x, 0.0)
    if c is not None:
      c = c + keep
  return s, c


def order_variants(steps, u):
  """The steps summed in a wrong order: the first group of `u` pairwise or
  reversed, the last step dropped or doubled -- the ways a kernel's time loop
  can go wrong.  Each entry is (what, steps' replacement, pairwise)."""
  out = []
  n = len(steps)
  if n >= u:
    out.append(('first group pairwise', steps, True))
  if n >= 2:
    g = min(n, u)
    out.append(('first group reversed', steps[:g][::-1] + steps[g:], False))
  out.append(('last step dropped', steps[:-1], False))
  out.append(('last step doubled', steps + steps[-1:], False))
  return out


def prove_order(start, steps, skipna, u, tag):
  """Shows on the reference alone that the data tell the time order: every
  variant of order_variants changes at least one bit of the sums."""
  want, _ = running_sum(start, steps, skipna)
  for what, alt, pairwise in order_variants(list(steps), u):
    if pairwise:
      x = [np.where(np.isnan(v) & skipna, 0.0, np.asarray(v, np.float64))
           for v in alt[:u]]
      with np.errstate(invalid='ignore'):
        group = (x[0] + x[1]) + (x[2] + x[3])
      s, _ = running_sum(start, [group], False)
      s, _ = running_sum(s, alt[u:], skipna)
    else:
      s, _ = running_sum(start, alt, skipna)
    assert not same_bits(s, want), f'{tag}: {what} changes no bit'


def same_bits(a, b):
  """Equal bit patterns wherever b is not NaN, NaN in exactly b's places."""
  a, b = np.asarray(a), np.asarray(b)
  if a.shape != b.shape or a.dtype != b.dtype:
    return False
  an, bn = np.isnan(a), np.isnan(b)
  u = {4: np.uint32, 8: np.uint64}[a.itemsize]
  return bool((an == bn).all() and (a.view(u) == b.view(u))[~bn].all())


def assert_bits(got, want, tag):
  """same_bits, with the first difference in the message (integer arrays:
  plain equality)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (
      tag, got.shape, want.shape, got.dtype, want.dtype)
  if got.dtype.kind != 'f':
    bad = got != want
  else:
    gn, wn = np.isnan(got), np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.itemsize]
    bad = (gn != wn) | (~wn & (got.view(u) != want.view(u)))
  if bad.any():
    i = int(np.argwhere(bad.ravel())[0][0])
    raise AssertionError(
        f'{tag}: {int(bad.sum())} of {bad.size} elements differ, first at '
        f'{i}: got {got.ravel()[i]!r} want {want.ravel()[i]!r}')


def seeps_map(f, y, wet, p1, dry, dtype):
  """oracle/metrics_np.SpatialSEEPS per point: the categories of forecast and
  truth (dry x < dry; light dry < x < wet; heavy x >= wet; NaN stays NaN), the
  sum over the nine cells of fc[i] * tc[j] * (0.5 * matrix[i][j]) with the
  matrix in the dtype of p1, NaN where p1 is masked (NaN).  Everything that
  the reference does in its inputs' dtype is done in `dtype` (f, y, wet and p1
  are taken in it, the dry threshold too); returns float64."""
  dtype = np.dtype(dtype)
  f, y, wet = (np.asarray(v).astype(dtype) for v in (f, y, wet))
  p = np.asarray(p1, dtype=np.float64).astype(dtype)
  dry = dtype.type(dry)

  def cats(x):
    with np.errstate(invalid='ignore'):
      conds = [x < dry, np.logical_and(x > dry, x < wet), x >= wet]
    return [np.where(np.isnan(x), np.nan, c.astype(np.float64)) for c in conds]
  one = dtype.type(1)
  with np.errstate(all='ignore'):
    matrix = [[0 * p, one / (one - p), dtype.type(4) / (one - p)],
              [one / p, 0 * p, dtype.type(3) / (one - p)],
              [one / p + dtype.type(3) / (dtype.type(2) + p),
               dtype.type(3) / (dtype.type(2) + p), 0 * p]]
    fc, tc = cats(f), cats(y)
    out = None
    for i in range(3):
      for j in range(3):
        term = (fc[i] * tc[j]) * (dtype.type(0.5) * matrix[i][j]).astype(
            np.float64)
        out = term if out is None else out + term
  return np.where(np.isnan(p), np.nan, out)
