"""NumPy's `quantile` / `nanquantile` with method='linear', restated on sorted
data without calling either (include/wb2hip.h, K12): what the GPU kernel and
the fixtures are compared with, bit for bit.

For the series x of one point: without `skipna` a NaN makes every quantile of
the point NaN and m = len(x); with it NaNs are dropped and m is the number of
values left (m == 0: NaN).  With s the m values in ascending order,
v = q (m - 1) in float64, lo = floor(v), hi = min(lo + 1, m - 1), t = v - lo,
a = s[lo], b = s[hi], d = b - a in the data's dtype, and the result is
float64(a) + float64(d) t where t < 0.5, float64(b) - float64(d) (1 - t) where
t >= 0.5.  Integers are float64 first."""
import numpy as np


def quantile(data, q, axis, skipna: bool) -> np.ndarray:
  """float64 [len(q), *preserved shape]; `axis` an int or a tuple of ints."""
  data = np.asarray(data)
  if data.dtype.kind != 'f':
    data = data.astype(np.float64)
  axes = (axis,) if np.ndim(axis) == 0 else tuple(axis)
  axes = tuple(a % data.ndim for a in axes)
  keep = tuple(a for a in range(data.ndim) if a not in axes)
  kept_shape = tuple(data.shape[a] for a in keep)
  x = np.transpose(data, keep + axes).reshape(kept_shape + (-1,))
  n = x.shape[-1]
  s = np.sort(x, axis=-1)  # NaN last
  n_nan = np.isnan(x).sum(axis=-1)
  m = n - n_nan if skipna else np.full(kept_shape, n)
  none = (m == 0) | ((n_nan > 0) & (not skipna))
  m1 = np.maximum(m, 1) - 1
  out = np.empty((len(q),) + kept_shape, dtype=np.float64)
  with np.errstate(all='ignore'):
    for i, qi in enumerate(np.asarray(q, dtype=np.float64)):
      v = qi * m1.astype(np.float64)
      lo = np.floor(v)
      t = v - lo
      lo = lo.astype(np.int64)
      hi = np.minimum(lo + 1, m1)
      a = np.take_along_axis(s, lo[..., None], axis=-1)[..., 0]
      b = np.take_along_axis(s, hi[..., None], axis=-1)[..., 0]
      d = b - a  # in the data's dtype
      assert d.dtype == data.dtype
      low = a.astype(np.float64) + d.astype(np.float64) * t
      high = b.astype(np.float64) - d.astype(np.float64) * (1.0 - t)
      res = np.where(t < 0.5, low, high)
      res[none] = np.nan
      out[i] = res
  return out


def assert_bit_equal(actual, expected, err_msg=''):
  """NaN in the same places and the same bytes elsewhere, +0.0 and -0.0
  counting as equal (NumPy's partition leaves that sign to chance)."""
  actual, expected = np.asarray(actual), np.asarray(expected)
  assert actual.dtype == np.float64 == expected.dtype, (
      err_msg, actual.dtype, expected.dtype)
  assert actual.shape == expected.shape, (err_msg, actual.shape,
                                          expected.shape)
  nan_a, nan_e = np.isnan(actual), np.isnan(expected)
  np.testing.assert_array_equal(nan_a, nan_e, err_msg=f'{err_msg}: NaN places')
  zero = (actual == 0) & (expected == 0)
  same = (actual.view(np.uint64) == expected.view(np.uint64)) | zero | nan_e
  if not same.all():
    at = tuple(np.argwhere(~same)[0])
    raise AssertionError(
        f'{err_msg}: {int((~same).sum())} of {same.size} differ, first at '
        f'{at}: {actual[at]!r} vs {expected[at]!r}')
