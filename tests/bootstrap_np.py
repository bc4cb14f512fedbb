"""The contract of K23 (include/wb2hip.h, weatherbench2_amd/bootstrap.py)
restated in NumPy and plain Python, loop by loop, the dense definition of a
bootstrap mean, and the bound between the two.

THE BOUND.  Let u = 2^-53 and, for one (replicate, outer index, point), let
the used steps be k = 1 .. K with counts n_k and values x_k, W = sum n_k and
A = sum n_k |x_k| / W.

The contract computes
  term_k = n_k x_k (1 + d_k),                       |d_k| <= u   (one rounding)
  S_1 = term_1,  S_k = (S_{k-1} + term_k)(1 + e_k), |e_k| <= u   (K - 1 adds)
  out = S_K / W (1 + h),                            |h| <= u     (W is exact)
so out = sum_k n_k x_k (1 + t_k) / W, where (1 + t_k) is a product of at most
1 + (K - 1) + 1 = K + 1 factors (1 + something of size <= u):
  |out - exact| <= ((1 + u)^(K + 1) - 1) A,  exact = sum n_k x_k / W.

The dense definition sums the drawn values x[idx] with ONE rounding
(`math.fsum` is exactly rounded): s = W exact (1 + a), |a| <= u, and divides by
W exactly (a `fractions.Fraction`, no rounding):
  |dense - exact| <= u |exact| <= u A.

Together, compared in exact rational arithmetic,
  |out - dense| <= (((1 + u)^(K + 1) - 1) + u) A,
which to first order is (K + 2) u A.  `bound` evaluates the exact form in
rationals (overflow and underflow do not occur at the values the tests use).
"""
import fractions
import math

import numpy as np

U = fractions.Fraction(1, 2 ** 53)


def bits(a):
  """(the bit patterns with every NaN as one pattern, the NaN mask)."""
  a = np.ascontiguousarray(a)
  if a.dtype.kind != 'f':  # counts and flags: the values themselves
    return a, np.zeros(a.shape, dtype=bool)
  nan = np.isnan(a)
  raw = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
  raw[nan] = 0
  return raw, nan


def assert_same_bits(got, want, err_msg=''):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (
      err_msg, got.dtype, want.dtype, got.shape, want.shape)
  (gb, gn), (wb, wn) = bits(got), bits(want)
  np.testing.assert_array_equal(gn, wn, err_msg=err_msg)
  np.testing.assert_array_equal(gb, wb, err_msg=err_msg)


def index_sequence(n_time, n_replicate, block_length, seed):
  """int [n_replicate, n_time]: the index sequence `block_plan` counts."""
  nb = -(-n_time // block_length)
  starts = np.random.default_rng(seed).integers(0, n_time,
                                                size=(n_replicate, nb))
  seq = np.empty((n_replicate, n_time), dtype=np.int64)
  for b in range(n_replicate):
    flat = [(int(s) + j) % n_time for s in starts[b]
            for j in range(block_length)]
    seq[b] = flat[:n_time]
  return seq


def counts_of(seq, n_time):
  return np.stack([np.bincount(row, minlength=n_time) for row in seq]
                  ).astype(np.int32)


def restated_means(x, counts, skipna=False):
  """The contract, one scalar at a time: float64 [B, n_outer, n_point] of
  x [n_outer, n_time, n_point] (float32 or float64)."""
  x = np.asarray(x)
  counts = np.asarray(counts)
  n_outer, n_time, n_point = x.shape
  out = np.empty((counts.shape[0], n_outer, n_point), dtype=np.float64)
  with np.errstate(all='ignore'):
    for b in range(counts.shape[0]):
      for o in range(n_outer):
        for p in range(n_point):
          chain, weight = None, 0
          for step in range(n_time):
            n = int(counts[b, step])
            if n == 0:
              continue
            value = np.float64(x[o, step, p])
            if skipna and value != value:
              continue
            term = np.float64(n) * value
            chain = term if chain is None else chain + term
            weight += n
          out[b, o, p] = (np.float64(0.0) / np.float64(0.0) if chain is None
                          else chain / np.float64(weight))
  return out


def dense_means(series, seq):
  """{replicate: Fraction}: fsum(series[seq[b]]) / n exactly, for one series
  (a 1-D float array) -- x[idx].mean(0) with an exactly rounded sum."""
  return [fractions.Fraction(math.fsum(float(series[i]) for i in row))
          / len(row) for row in seq]


def bound(series, count_row):
  """The exact form of the bound for one series and one replicate's counts
  (module docstring), a Fraction."""
  used = [(int(n), fractions.Fraction(float(v)))
          for n, v in zip(count_row, series) if n]
  k = len(used)
  weight = sum(n for n, _ in used)
  a = sum(n * abs(v) for n, v in used) / weight
  return (((1 + U) ** (k + 1) - 1) + U) * a


def first_order_bound(series, count_row):
  used = [(int(n), abs(float(v))) for n, v in zip(count_row, series) if n]
  return (len(used) + 2) * 2.0 ** -53 * sum(n * v for n, v in used) / sum(
      n for n, _ in used)
