"""The float64 reference shared by the geometry sweeps of the streaming
(test_stream_geometry_gpu.py) and the ensemble reductions
(test_ens_geometry_gpu.py).

Per-point region weights come from oracle/metrics_np.get_lat_weights times
what oracle/regions_np's Region.apply leaves (land fraction included), never
from plan.py; every sum is a math.fsum of the float64 products, so a kernel's
sum may differ from it by its own rounding only: SUM_RTOL * sum|w x|.
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
