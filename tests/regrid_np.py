"""NumPy restatement of K11 as include/wb2hip.h defines it: the CSR build from
the dense weight matrices, WB2_REGRID_NANMEAN, WB2_REGRID_LINEAR and the
gather, in the header's order of operations (latitude sum inside, longitude
sum outside, table order, float64, every multiply and add rounded on its own),
so that the kernels can be compared bit for bit in both layouts.

Fields are (..., lon, lat) here, whatever layout the device reads.  Written
from the header, not from the product's Python.
"""
import numpy as np


def csr(weights: np.ndarray, wrap: bool = False) -> tuple:
  """(ptr, idx, w, nan) of a dense (target, source) matrix: the entries with
  w != 0 in ascending source index; a band over the seam of a periodic
  longitude (`wrap`) starts behind its largest inner gap; a row with a NaN is
  uncovered and empty."""
  weights = np.asarray(weights, dtype=np.float64)
  n_source = weights.shape[1]
  ptr, idx, w, nan = [0], [], [], []
  for row in weights:
    bad = bool(np.isnan(row).any())
    nan.append(int(bad))
    if not bad:
      at = [int(i) for i in np.flatnonzero(row != 0)]
      if wrap and len(at) > 1:
        gaps = [at[i + 1] - at[i] for i in range(len(at) - 1)]
        seam = at[0] + n_source - at[-1]
        if max(gaps) > seam:
          cut = gaps.index(max(gaps)) + 1
          at = at[cut:] + at[:cut]
      idx += at
      w += [float(row[i]) for i in at]
    ptr.append(len(idx))
  return (np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int64),
          np.array(w, dtype=np.float64), np.array(nan, dtype=bool))


def dense(table: tuple, n_source: int) -> np.ndarray:
  """The dense matrix back from a table (NaN rows where uncovered)."""
  ptr, idx, w, nan = table
  out = np.zeros((len(nan), n_source))
  for k in range(len(nan)):
    if nan[k]:
      out[k] = np.nan
    for q in range(ptr[k], ptr[k + 1]):
      out[k, idx[q]] = w[q]
  return out


def taps(source_points, target_points, clamp: bool, period=None) -> tuple:
  """Two taps per target point, (i0, i1) and (t, 0): np.interp's search with
  its `period`, `left` / `right` (clamped or NaN) and node coincidence moved
  into a table."""
  xp = np.asarray(source_points, dtype=np.float64)
  x = np.asarray(target_points, dtype=np.float64)
  order = np.arange(len(xp))
  if period is not None:
    x, xp = x % period, xp % period
    order = np.argsort(xp)
    xp = xp[order]
    xp = np.concatenate([[xp[-1] - period], xp, [xp[0] + period]])
    order = np.concatenate([[order[-1]], order, [order[0]]])
  ptr = 2 * np.arange(len(x) + 1, dtype=np.int64)
  idx = np.zeros(2 * len(x), dtype=np.int64)
  w = np.zeros(2 * len(x), dtype=np.float64)
  nan = np.zeros(len(x), dtype=bool)
  for k, v in enumerate(x):
    if v < xp[0] or v > xp[-1]:
      if clamp:
        idx[2 * k:2 * k + 2] = order[0] if v < xp[0] else order[-1]
      else:
        nan[k] = True
      continue
    j = int(np.searchsorted(xp, v, side='right')) - 1
    if j == len(xp) - 1 or xp[j] == v:
      idx[2 * k:2 * k + 2] = order[j]
    else:
      idx[2 * k], idx[2 * k + 1] = order[j], order[j + 1]
      w[2 * k] = (v - xp[j]) / (xp[j + 1] - xp[j])
  return ptr, idx, w, nan


def _axis_sum(values: np.ndarray, table: tuple, axis: int) -> np.ndarray:
  """sum_k w[k] * values[idx[k]] along `axis`, per target index, started at
  0.0 and run in table order (uncovered: 0.0 here, NaN at the end)."""
  ptr, idx, w, nan = table
  moved = np.moveaxis(values, axis, -1)
  out = np.zeros(moved.shape[:-1] + (len(nan),), dtype=np.float64)
  for k in range(len(nan)):
    acc = np.zeros(moved.shape[:-1], dtype=np.float64)
    for q in range(ptr[k], ptr[k + 1]):
      acc = acc + w[q] * moved[..., idx[q]]
    out[..., k] = acc
  return np.moveaxis(out, -1, axis)


def _uncovered(shape, lon_table, lat_table) -> np.ndarray:
  return np.broadcast_to(lon_table[3][:, None] | lat_table[3][None, :], shape)


def nanmean(field: np.ndarray, lon_table: tuple, lat_table: tuple,
            with_abs: bool = False):
  """WB2_REGRID_NANMEAN on (..., lon, lat) in the dtype of `field` (float32 or
  float64).  With `with_abs`: (out, A, count), A = the same sums over |field|
  with |w| and count as float64: the terms of the bound against the
  reference."""
  dtype = field.dtype
  missing = np.isnan(field)
  f = np.where(missing, 0.0, field.astype(np.float64))
  present = np.where(missing, 0.0, 1.0)
  with np.errstate(all='ignore'):
    total = _axis_sum(_axis_sum(f, lat_table, -1), lon_table, -2)
    count = _axis_sum(_axis_sum(present, lat_table, -1), lon_table, -2)
    out = total / count
  bad = _uncovered(out.shape, lon_table, lat_table)
  out = np.where(bad, np.nan, out).astype(dtype)
  if not with_abs:
    return out
  mag = lambda tab: (tab[0], tab[1], np.abs(tab[2]), tab[3])
  with np.errstate(all='ignore'):
    a = _axis_sum(_axis_sum(np.abs(f), mag(lat_table), -1), mag(lon_table),
                  -2)
  return out, a, count


def _lerp(f0, f1, t):
  with np.errstate(all='ignore'):
    return np.where(t == 0.0, f0, f0 + t * (f1 - f0))


def _axis_lerp(values: np.ndarray, table: tuple, axis: int) -> np.ndarray:
  _, idx, w, _ = table
  moved = np.moveaxis(values, axis, -1)
  out = _lerp(moved[..., idx[0::2]], moved[..., idx[1::2]], w[0::2])
  return np.moveaxis(out, -1, axis)


def linear(field: np.ndarray, lon_table: tuple, lat_table: tuple,
           with_abs: bool = False):
  """WB2_REGRID_LINEAR on (..., lon, lat): latitude first, then longitude.
  With `with_abs`: (out, A), A = the same interpolation of |field| (weights
  1 - t and t are not negative)."""
  dtype = field.dtype
  f = field.astype(np.float64)
  out = _axis_lerp(_axis_lerp(f, lat_table, -1), lon_table, -2)
  bad = _uncovered(out.shape, lon_table, lat_table)
  out = np.where(bad, np.nan, out).astype(dtype)
  if not with_abs:
    return out
  a = _axis_lerp(_axis_lerp(np.abs(f), lat_table, -1), lon_table, -2)
  return out, a


def gather(field: np.ndarray, indices: np.ndarray, target_shape: tuple):
  """out[..., j] = raveled (lon, lat) slab at indices[j], reshaped."""
  lead = field.shape[:-2]
  flat = field.reshape(lead + (-1,))
  return np.take(flat, indices, axis=-1).reshape(lead + tuple(target_shape))


def haversine_matrix(source: dict, target: dict) -> np.ndarray:
  """[target node, source node] great-circle distances in radians, both in
  raveled (lon, lat) order: the full brute-force table."""
  def nodes(grid):
    lon, lat = np.meshgrid(np.deg2rad(np.asarray(grid['longitudes'], float)),
                           np.deg2rad(np.asarray(grid['latitudes'], float)),
                           indexing='ij')
    return lon.ravel(), lat.ravel()
  s_lon, s_lat = nodes(source)
  t_lon, t_lat = nodes(target)
  a = (np.sin((t_lat[:, None] - s_lat[None, :]) / 2) ** 2
       + np.cos(t_lat[:, None]) * np.cos(s_lat[None, :])
       * np.sin((t_lon[:, None] - s_lon[None, :]) / 2) ** 2)
  return 2 * np.arcsin(np.sqrt(a))


def tables(regridder) -> tuple:
  """(longitude table, latitude table) of a product regridder, built here from
  its dense weights (conservative) or from its grids (bilinear)."""
  src, tgt = regridder.source, regridder.target
  if hasattr(regridder, 'weights'):
    lon_w, lat_w = regridder.weights
    return csr(lon_w, wrap=bool(src.periodic)), csr(lat_w)
  return (taps(src.longitudes, tgt.longitudes, False,
               360 if src.periodic else None),
          taps(src.latitudes, tgt.latitudes, bool(src.includes_poles)))


def longest(table: tuple) -> int:
  return int(np.diff(table[0]).max())


def run(regridder, field: np.ndarray, with_abs: bool = False):
  """The restatement of `regridder.regrid_array(field)`: with `with_abs`
  (out, A, count, K), K = the longest longitude band + the longest latitude
  band (the terms of `reference_bound`)."""
  lon_table, lat_table = tables(regridder)
  if hasattr(regridder, 'weights'):
    res = nanmean(field, lon_table, lat_table, with_abs)
  else:
    res = linear(field, lon_table, lat_table, with_abs)
    if with_abs:
      res = res + (np.ones_like(res[1]),)
  if not with_abs:
    return res
  return res + (longest(lon_table) + longest(lat_table),)


def reference_bound(a: np.ndarray, count: np.ndarray, k: int, dtype,
                    ref: np.ndarray) -> np.ndarray:
  """The bound on |kernel - reference| per point.  Both sides form the same
  two nested sums of at most K products in float64, with weights that agree to
  1e-12, in a different order: with gamma = (K + 4) 2^-53 and A the same sums
  over |field| with |w|, the quotient total / count is off by at most
  4 gamma A / |count| + 1e-12 A; a float32 result adds its own rounding,
  2^-24 |ref|."""
  gamma = (k + 4) * 2.0 ** -53
  with np.errstate(all='ignore'):
    bound = 4 * gamma * a / np.abs(count) + 1e-12 * a
  if np.dtype(dtype) == np.float32:
    bound = bound + 2.0 ** -24 * np.abs(ref)
  return bound


def assert_within_reference(got, ref, a, count, k, msg=''):
  """NaN positions equal; elsewhere within `reference_bound`."""
  nan = np.isnan(ref)
  assert got.shape == ref.shape, (msg, got.shape, ref.shape)
  assert np.array_equal(np.isnan(got), nan), msg
  bound = reference_bound(a, count, k, got.dtype, ref)
  err = np.abs(got.astype(np.float64) - ref)
  ok = ~nan
  worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() \
      else 0.0
  assert (err[ok] <= bound[ok]).all(), (msg, worst)
  return worst
