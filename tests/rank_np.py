"""Plain NumPy references of the rank histogram (K6, rank_histogram.hip): no
torch, nothing of the library.

Samples are rows: `ens[..., M]` holds the members of a sample, `truth[...]` its
truth.  For the seeded tie breaking a sample is the row `values[..., M + 1]` of
the reference's concatenated array (column 0 the truth, then the members), and
`stream_index[..., M + 1]` says where in np.random.default_rng(seed)'s stream
of doubles each of its elements takes its perturbation from: the reference
draws one double per element of the whole concatenated array in C order, so
that index is the element's C-order index there.
"""
import numpy as np

# dense index ranges up to this many doubles are drawn in one call
_BULK = 1 << 23


def counts(ens, truth):
  """lo = #{x_m < t}, eq = #{x_m == t}, nn = #{x_m not NaN} per sample."""
  ens, truth = np.asarray(ens), np.asarray(truth)
  t = truth[..., None]
  with np.errstate(invalid='ignore'):
    lo = (ens < t).sum(-1)
    eq = (ens == t).sum(-1)
  nn = (~np.isnan(ens)).sum(-1)
  return lo, eq, nn


def first_rank(ens, truth):
  """The rank without random tie breaking: the truth first among equals, NaN
  above everything (a NaN truth above every non-NaN member)."""
  lo, _, nn = counts(ens, truth)
  return np.where(np.isnan(truth), nn, lo)


def bin_of(rank, n_member, n_bins):
  """Bin of a rank 0..M: rank // ((M + 1) // n_bins)."""
  if n_bins < 1 or (n_member + 1) % n_bins:
    raise ValueError(f'{n_member=} does not bin into {n_bins}')
  return np.asarray(rank) // ((n_member + 1) // n_bins)


def one_hot(bins, n_bins):
  """float64 [..., n_bins]: 1.0 at each sample's bin."""
  bins = np.asarray(bins)
  assert bins.min(initial=0) >= 0 and bins.max(initial=0) < n_bins
  out = np.zeros(bins.shape + (n_bins,), dtype=np.float64)
  np.put_along_axis(out, bins[..., None], 1.0, axis=-1)
  return out


def sum_over(hot, axis):
  """Counts: the plain float64 sum of one-hots over one axis."""
  return np.asarray(hot, dtype=np.float64).sum(axis=axis)


def mean_over(hot, axis):
  """Mean of one-hots over one axis: the sum, then a true division."""
  return sum_over(hot, axis) / np.float64(np.shape(hot)[axis])


def perturbation_size(values, dtype, size_dtype=None):
  """Half the smallest positive gap of each sample's sorted values, computed in
  the data dtype; 1 where there is no positive gap or the gaps hold a NaN (a NaN
  value, or two equal infinities).  `size_dtype` computes it in another dtype
  instead: only for showing that a data recipe can tell the two apart."""
  v = np.asarray(values, dtype=dtype)
  if size_dtype is not None:
    v = v.astype(size_dtype)
  with np.errstate(invalid='ignore', over='ignore'):
    diffs = np.diff(np.sort(v, axis=-1), axis=-1)
    inf = np.asarray(np.inf, dtype=v.dtype)
    diffs = np.where(diffs == 0, inf, diffs)
    min_diff = diffs.min(axis=-1, keepdims=True)
    size = np.where(min_diff < inf, min_diff / np.asarray(2, v.dtype),
                    np.asarray(1, v.dtype))
  assert size.dtype == v.dtype
  return size


def _uniform_at(low, high, stream_index, seed):
  """np.random.default_rng(seed).uniform(low, high) as the element at each
  stream index would receive it."""
  low = np.broadcast_to(low, stream_index.shape).astype(np.float64)
  high = np.broadcast_to(high, stream_index.shape).astype(np.float64)
  flat = [int(k) for k in stream_index.ravel()]
  base, span = min(flat), max(flat) - min(flat) + 1
  if span <= _BULK:
    # one call over the dense range, bounds scattered to their places
    rel = np.array([k - base for k in flat], dtype=np.int64)
    lo_full, hi_full = np.zeros(span), np.zeros(span)
    lo_full[rel], hi_full[rel] = low.ravel(), high.ravel()
    bg = np.random.PCG64(seed)
    bg.advance(base)
    draws = np.random.Generator(bg).uniform(lo_full, hi_full)[rel]
    return draws.reshape(stream_index.shape)
  state0 = np.random.PCG64(seed).state
  out = np.empty(len(flat), dtype=np.float64)
  for i, (k, lo, hi) in enumerate(zip(flat, low.ravel(), high.ravel())):
    bg = np.random.PCG64(0)
    bg.state = state0
    bg.advance(k)
    out[i] = np.random.Generator(bg).uniform(lo, hi)
  return out.reshape(stream_index.shape)


def numpy_rank(values, stream_index, seed, dtype, size_dtype=None):
  """(rank, perturbed): the truth's position after the reference's seeded
  perturbation -- uniform in +-size/2, size from perturbation_size, added in
  float64 -- and argsort / argmin along the sample."""
  v = np.asarray(values, dtype=dtype)
  stream_index = np.asarray(stream_index)
  assert stream_index.shape == v.shape and v.shape[-1] >= 2
  size = perturbation_size(v, dtype, size_dtype)
  draws = _uniform_at(-size / 2, size / 2, stream_index, seed)
  with np.errstate(invalid='ignore'):
    perturbed = v + draws
  assert perturbed.dtype == np.float64
  order = np.argsort(perturbed, axis=-1)
  return order.argmin(axis=-1), perturbed


def ambiguous(perturbed):
  """True where the perturbed truth (column 0) is exactly equal to a perturbed
  member, or both are NaN: NumPy's unstable argsort leaves their order open."""
  p = np.asarray(perturbed)
  t, rest = p[..., :1], p[..., 1:]
  with np.errstate(invalid='ignore'):
    return ((rest == t) | (np.isnan(rest) & np.isnan(t))).any(-1)


def perturbed_bounds(perturbed):
  """(#less, #equal): members sorted before the perturbed truth whatever the
  sort does, and members it may put on either side (NaN sorts last)."""
  p = np.asarray(perturbed)
  t, rest = p[..., :1], p[..., 1:]
  with np.errstate(invalid='ignore'):
    less = (rest < t) | (np.isnan(t) & ~np.isnan(rest))
    equal = (rest == t) | (np.isnan(rest) & np.isnan(t))
  return less.sum(-1), equal.sum(-1)
