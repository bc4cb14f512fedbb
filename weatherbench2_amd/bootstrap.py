"""Block-bootstrap confidence intervals for any score (the reference has no
counterpart).

The scores of this package are non-linear in the time mean (RMSE, ACC, FSS,
fair CRPS, skill scores, reliability terms), and the rule of every table
metric is "the time mean of the TABLES first, the score from the mean table".
The bootstrap follows it: it resamples the per-time results (what
`metric.compute_chunk` / `compute_chunk_regions` return, or what
`evaluate_chunks` keeps with `temporal_mean=False`), forms the resampled MEAN
table of every replicate and applies the score to it.  Forecast errors are
autocorrelated in init time, so the resampling is a block bootstrap.

  * `block_plan` draws the circular moving-block bootstrap as COUNTS: how often
    every time enters every replicate.  Host NumPy, reproducible from a seed.
  * `resample_means` turns per-time results and counts into the replicates'
    means: a leading `replicate` dim takes the place of the time dim.
    Device-backed variables go through K23 (csrc/resample_means.hip,
    `engine.resampled_means`), host variables through `host_resample_means`
    in NumPy -- in the same order, with the same bits.
  * `bootstrap` scores every replicate, keeps the (small) scores and returns
    the point estimate, the percentile interval, the standard error and, with
    `reference=`, the paired difference and its significance.

THE ORDER of a mean (wb2hip.h states it for K23): for replicate b, walk t = 0
.. n_time - 1 with n = counts[b, t]; a step with n == 0 is LEFT OUT (a NaN or
+-inf at a time the replicate did not draw cannot reach it); x is the value
widened to float64, with `skipna` a NaN x is left out; term = n * x; the first
used term starts the chain, every later one is S = S + term; W is the integer
sum of the used n; the mean is S / W, and 0 / 0 = NaN where nothing was used.

Layout (`operands.SeriesLayout`): a time dim with a dim after it is read where
it lies -- a contiguous tensor, a time-sliced view, a `SlabGather` and a
permuted time order differ in the slab table alone --; a time dim that is the
innermost of several costs one transposing device copy; integer and bool data
become float64 first.  Inputs are never modified.

Out of scope: BCa and studentized intervals, the stationary bootstrap, an
automatic block length, more than one resampled dim.
"""
from __future__ import annotations

import typing as t
import warnings

import numpy as np
import torch

from weatherbench2_amd import engine
from weatherbench2_amd import indexing
from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

REPLICATE = 'replicate'
TIME_DIMS = ('init_time', 'time')
# `bootstrap` holds at most this many bytes of resampled tables at once (all
# inputs of a batch, the reference's included) unless `replicates_per_batch`
# says otherwise
BATCH_BYTES = 1 << 30


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
def block_plan(n_time: int, n_replicate: int, block_length: int = 1,
               seed: int = 0) -> np.ndarray:
  """int32 [n_replicate, n_time]: the circular moving-block bootstrap as
  counts.  With nb = ceil(n_time / block_length), starts =
  `np.random.default_rng(seed).integers(0, n_time, size=(n_replicate, nb))`;
  the index sequence of a replicate is `(starts[:, :, None] +
  arange(block_length)) % n_time`, flattened and cut to its first n_time
  entries; counts[b, t] is how often t occurs in it.  Every row sums to
  n_time.  block_length=1 is the iid bootstrap."""
  n_time, n_replicate, block_length = (
      int(n_time), int(n_replicate), int(block_length))
  if n_time < 1:
    raise ValueError(f'n_time={n_time}: the bootstrap needs at least one time')
  if n_replicate < 1:
    raise ValueError(f'n_replicate={n_replicate}: the bootstrap needs at least '
                     'one replicate')
  if not 1 <= block_length <= n_time:
    raise ValueError(f'block_length={block_length} is not in 1..{n_time} '
                     '(n_time)')
  nb = -(-n_time // block_length)
  starts = np.random.default_rng(seed).integers(0, n_time,
                                                size=(n_replicate, nb))
  index = (starts[:, :, None] + np.arange(block_length)) % n_time
  index = index.reshape(n_replicate, -1)[:, :n_time]
  counts = np.zeros((n_replicate, n_time), dtype=np.int32)
  np.add.at(counts, (np.arange(n_replicate)[:, None], index), 1)
  return counts


# ---------------------------------------------------------------------------
# the two paths: [n_replicate, n_outer, n_point] float64
# ---------------------------------------------------------------------------
def host_resample_means(x: np.ndarray, counts, skipna: bool = False
                        ) -> np.ndarray:
  """`engine.resampled_means` in NumPy: float64 [n_replicate, n_outer,
  n_point] of the float32 / float64 array `x` [n_outer, n_time, n_point], one
  rank-1 update per time step, in the order of the module docstring.  (A chain
  starts at -0.0, as in the kernel: (-0.0) + term has the bits of term.)"""
  x = np.asarray(x)
  if x.ndim != 3:
    raise ValueError(f'x must be [n_outer, n_time, n_point], not {x.shape}')
  if x.dtype not in (np.float32, np.float64):
    x = x.astype(np.float64)
  n_outer, n_time, n_point = x.shape
  counts = engine.checked_counts(counts, n_time)
  n_rep = counts.shape[0]
  total = np.full((n_rep, n_outer, n_point), -0.0, dtype=np.float64)
  weight = np.zeros((n_rep, n_outer, n_point) if skipna else (n_rep, 1, 1),
                    dtype=np.int64)
  with np.errstate(all='ignore'):
    for step in range(n_time):
      rows = np.nonzero(counts[:, step])[0]
      if not rows.size:
        continue
      n = counts[rows, step][:, None, None]
      value = x[:, step, :].astype(np.float64)
      term = n.astype(np.float64) * value[None]
      if skipna:
        used = ~np.isnan(value)[None]
        total[rows] = np.where(used, total[rows] + term, total[rows])
        weight[rows] += np.where(used, n, 0)
      else:
        total[rows] += term
        weight[rows] += n
    return total / weight.astype(np.float64)


def _variable_means(da: xl.DataArray, dim: str, counts: np.ndarray,
                    skipna: bool):
  """One variable with `dim`: (data, dims) with a leading replicate dim in the
  place of `dim`, float64, where the variable lies."""
  lay = operands.SeriesLayout.of(da.dims, da.sizes, dim)
  n_outer, n_time, n_point = lay.n_outer, lay.n_series, lay.n_point
  n_rep = counts.shape[0]
  if operands.on_device(da.data):
    device = engine.require_gpu()
    if n_outer * n_point == 0:
      flat = torch.empty((n_rep, n_outer, n_point), dtype=torch.float64,
                         device=device)
    else:
      ten, table = operands.operand(da, lay.order, device,
                                    operands.float_dtype(da.dtype),
                                    lay.n_inner_dims)
      flat = engine.resampled_means(ten, table, n_outer, n_time, n_point,
                                    counts, skipna)
  else:
    flat = host_resample_means(lay.host(da), counts, skipna)
  data = lay.restore(flat, (), lead=(n_rep,))
  return data, (REPLICATE,) + tuple(d for d in da.dims if d != dim)


def _pick_dim(obj, dim: t.Optional[str]) -> str:
  dims = obj.dims if isinstance(obj, xl.DataArray) else tuple(obj.dims)
  if dim is not None:
    if dim not in dims:
      raise ValueError(f'{dim!r} missing from {tuple(dims)}')
    return dim
  have = [d for d in TIME_DIMS if d in dims]
  if len(have) != 1:
    raise ValueError(
        f'dim=None needs exactly one of {TIME_DIMS} in {tuple(dims)}: '
        'name the dim to resample over')
  return have[0]


def resample_means(obj, counts, dim: t.Optional[str] = None,
                   skipna: bool = False):
  """`obj` (a Dataset or a DataArray of per-time results) with every variable
  that has `dim` replaced by its resampled means: such a variable loses `dim`
  and gains a LEADING `replicate` dim with the coordinate arange(B), keeps its
  other dims in order with their coordinates, becomes float64 and stays on its
  device.  Variables without `dim` are returned unchanged.  `dim=None` picks
  the one of `init_time` / `time` that is present.  `counts` is an integer
  array [B, n_time] with entries >= 0 and row sums below 2^31 (`block_plan`
  makes one).  See the module docstring for the order and the layout."""
  if xl.is_xarray(obj):
    if hasattr(obj, 'data_vars'):
      return xl.like_input(resample_means(xl.from_xarray(obj), counts, dim,
                                          skipna), obj)
    name = obj.name if obj.name is not None else '_bootstrap_input'
    lite = xl.from_xarray(obj.to_dataset(name=name))
    return xl.like_input(resample_means(lite[name], counts, dim, skipna), obj)
  if isinstance(obj, xl.DataArray):
    dim = _pick_dim(obj, dim)
    counts = engine.checked_counts(counts, obj.sizes[dim])
    data, dims = _variable_means(obj, dim, counts, skipna)
    coords = xl.coords_without(obj.coords, (dim,))
    coords[REPLICATE] = np.arange(counts.shape[0], dtype=np.int64)
    return xl.DataArray(data, dims, coords, obj.name)
  ds = xl.as_dataset(obj)
  dim = _pick_dim(ds, dim)
  counts = engine.checked_counts(counts, ds.dims[dim])
  coords = xl.coords_without(ds.coords, (dim,))
  coords[REPLICATE] = np.arange(counts.shape[0], dtype=np.int64)
  out = xl.Dataset(coords=coords, attrs=ds.attrs)
  for name, da in ds.data_vars.items():
    if dim in da.dims:
      data, dims = _variable_means(da, dim, counts, skipna)
    else:
      data, dims = da.data, da.dims
    out.data_vars[name] = xl.DataArray(data, dims, coords, name)
  return out


# ---------------------------------------------------------------------------
# bootstrap()
# ---------------------------------------------------------------------------
def _identity(table):
  """score_fn=None: the resampled variables themselves (a variable without
  the time dim has no replicates and no interval)."""
  return xl.Dataset({k: v for k, v in table.data_vars.items()
                     if REPLICATE in v.dims}, table.coords, table.attrs)


def _flat_scores(result) -> dict:
  """{name: DataArray or array} of what a score function returned."""
  if xl.is_xarray(result):
    result = (xl.from_xarray(result) if hasattr(result, 'data_vars') else
              xl.DataArray(np.asarray(result.values), tuple(result.dims),
                           {k: np.asarray(result.coords[k].values)
                            for k in result.dims if k in result.coords},
                           result.name))
  if isinstance(result, xl.DataArray):
    return {result.name or 'score': result}
  if isinstance(result, xl.Dataset):
    return dict(result.data_vars)
  if isinstance(result, dict):
    out = {}
    for key, value in result.items():
      if isinstance(value, (xl.Dataset, dict)) or (
          xl.is_xarray(value) and hasattr(value, 'data_vars')):
        for name, v in _flat_scores(value).items():
          out[f'{key}_{name}'] = v
      else:
        out[key] = value
    return out
  raise TypeError('a score function returns a Dataset, a DataArray or '
                  f'{{variable: array}}, not {type(result)}')


def _score_batch(score_fn, means: t.Sequence, n_rep: int, vectorized: bool
                 ) -> dict:
  """{name: (float64 host array [n_rep, ...], dims behind replicate, coords)}
  of one batch of resampled mean tables."""
  if vectorized:
    parts = [_flat_scores(score_fn(*means))]
  else:
    parts = [_flat_scores(score_fn(*[m.isel(**{REPLICATE: b}) for m in means]))
             for b in range(n_rep)]
  out = {}
  for name, first in parts[0].items():
    if isinstance(first, xl.DataArray):
      dims, coords = tuple(first.dims), dict(first.coords)
      values = [np.asarray(p[name].values, dtype=np.float64) for p in parts]
    else:
      values = [np.asarray(torch.as_tensor(p[name]).cpu()
                           if isinstance(p[name], torch.Tensor) else p[name],
                           dtype=np.float64) for p in parts]
      shape = values[0].shape
      dims = (REPLICATE,) * bool(vectorized) + tuple(
          f'dim_{i}' for i in range(len(shape) - bool(vectorized)))
      coords = {}
    if vectorized:
      if not dims or dims[0] != REPLICATE or values[0].shape[0] != n_rep:
        raise ValueError(
            f'score {name!r} has dims {dims}: the score function does not '
            f'carry the leading {REPLICATE!r} dim; pass vectorized=False')
      value, dims = values[0], dims[1:]
    else:
      if REPLICATE in dims:
        raise ValueError(f'score {name!r} keeps a {REPLICATE!r} dim')
      value = np.stack(values, axis=0)
    coords = {k: c for k, c in coords.items() if k != REPLICATE}
    out[name] = (value, dims, coords)
  return out


def _time_labels(tables: t.Sequence, dim: str) -> int:
  """n_time; every input has the same time labels along `dim`."""
  first, n_time = None, None
  for table in tables:
    if dim not in table.dims:
      raise ValueError(f'{dim!r} missing from {tuple(table.dims)}')
    n = int(table.dims[dim])
    labels = xl.coord_values(table, dim) if dim in table.coords else None
    if n_time is None:
      n_time, first = n, labels
      continue
    same = n == n_time and (labels is None) == (first is None)
    if same and labels is not None:
      same = np.array_equal(indexing.positions(first, labels), np.arange(n))
    if not same:
      raise ValueError(f'the inputs differ in their {dim!r} labels: every '
                       'table of a bootstrap covers the same times')
  return n_time


def _bytes_per_replicate(tables: t.Sequence, dim: str) -> int:
  total = 0
  for table in tables:
    for da in table.data_vars.values():
      if dim in da.dims:
        total += 8 * int(np.prod([n for d, n in da.sizes.items() if d != dim],
                                 dtype=np.int64))
  return total


def bootstrap(tables, score_fn: t.Optional[t.Callable] = None, *,
              reference=None, n_replicate: int = 1000, block_length: int = 1,
              seed: int = 0, level: float = 0.95,
              dim: t.Optional[str] = None, skipna: bool = False,
              replicates_per_batch: t.Optional[int] = None,
              vectorized: bool = True) -> xl.Dataset:
  """Percentile confidence intervals of `score_fn(*mean tables)` from a
  circular moving-block bootstrap over the time dim `dim`.

  `tables` is one per-time Dataset (or DataArray), or a tuple of them when the
  score takes several (`twcrpss(table, reference_table)`).  `score_fn` returns
  a Dataset, a DataArray or {variable: array}; None is the identity (one
  table): the resampled mean itself is the score.  Per batch of replicates:
  one `resample_means` per input with the SAME counts, `score_fn` on the batch
  with its leading `replicate` dim (`vectorized=False` calls it replicate by
  replicate, for a function that cannot carry a leading dim), and only the
  scores are kept.  `replicates_per_batch` bounds the resampled tables held at
  once; the default holds at most BATCH_BYTES (1 GiB) of them, at least one
  replicate.  The batching changes no bit.

  The result is a Dataset with, per score variable `<name>`: `<name>` (the
  score of the un-resampled mean table: the same code path with all counts 1),
  `<name>_lower` / `<name>_upper` (NumPy 'linear' quantiles at (1 - level) / 2
  and 1 - (1 - level) / 2 over the replicates whose score is not NaN),
  `<name>_standard_error` (std over those replicates, ddof=1) and
  `<name>_valid_replicates`.  With `reference=` (tables of the same structure
  from another forecast) every replicate scores both with the SAME counts, all
  statistics are those of score(tables) - score(reference), and
  `<name>_significant` is true where lower > 0 or upper < 0.  Attributes:
  n_replicate, block_length, seed, level."""
  given = tables if isinstance(tables, (tuple, list)) else (tables,)
  refs = () if reference is None else (
      reference if isinstance(reference, (tuple, list)) else (reference,))

  def lite(obj):
    if isinstance(obj, xl.DataArray):
      return xl.Dataset({obj.name or 'score': obj}, obj.coords)
    return xl.as_dataset(obj)
  mine, theirs = [lite(x) for x in given], [lite(x) for x in refs]
  if not mine:
    raise ValueError('no tables')
  if refs and len(theirs) != len(mine):
    raise ValueError(f'reference holds {len(theirs)} tables, tables '
                     f'{len(mine)}: they must have the same structure')
  if score_fn is None:
    if len(mine) != 1:
      raise ValueError('score_fn=None (the resampled mean itself) takes one '
                       'table')
    score_fn, vectorized = _identity, True
  if not 0.0 < float(level) < 1.0:
    raise ValueError(f'level={level} is not in (0, 1)')
  dim = _pick_dim(mine[0], dim)
  n_time = _time_labels(mine + theirs, dim)
  counts = block_plan(n_time, n_replicate, block_length, seed)
  n_replicate = counts.shape[0]
  if replicates_per_batch is None:
    per = max(_bytes_per_replicate(mine + theirs, dim), 1)
    replicates_per_batch = max(1, BATCH_BYTES // per)
  batch = int(replicates_per_batch)
  if batch < 1:
    raise ValueError(f'replicates_per_batch={replicates_per_batch} is not '
                     'positive')
  batch = min(batch, n_replicate)

  def scores(part: np.ndarray) -> dict:
    n = part.shape[0]
    out = _score_batch(
        score_fn, [resample_means(x, part, dim, skipna) for x in mine], n,
        vectorized)
    if theirs:
      other = _score_batch(
          score_fn, [resample_means(x, part, dim, skipna) for x in theirs], n,
          vectorized)
      with np.errstate(all='ignore'):
        out = {k: (v - other[k][0], dims, coords)
               for k, (v, dims, coords) in out.items()}
    return out

  point = scores(np.ones((1, n_time), dtype=np.int32))
  kept = {k: np.empty((n_replicate,) + v.shape[1:], dtype=np.float64)
          for k, (v, _, _) in point.items()}
  for start in range(0, n_replicate, batch):
    part = scores(counts[start:start + batch])
    for k, (v, _, _) in part.items():
      kept[k][start:start + batch] = v

  alpha = (1.0 - float(level)) / 2.0
  coords: dict = {}
  for _, _, c in point.values():
    coords.update(c)
  out = xl.Dataset(coords=coords, attrs={
      'n_replicate': int(n_replicate), 'block_length': int(block_length),
      'seed': seed, 'level': float(level)})

  def put(name, value, dims):
    out.data_vars[name] = xl.DataArray(value, dims, coords, name)
  for name, (value, dims, _) in point.items():
    reps = kept[name]
    valid = ~np.isnan(reps)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
      warnings.simplefilter('ignore')
      lower, upper = np.nanquantile(reps, [alpha, 1.0 - alpha], axis=0,
                                    method='linear')
      error = np.nanstd(reps, axis=0, ddof=1)
    put(name, value[0], dims)
    put(f'{name}_lower', lower, dims)
    put(f'{name}_upper', upper, dims)
    put(f'{name}_standard_error', error, dims)
    put(f'{name}_valid_replicates', valid.sum(axis=0).astype(np.int64), dims)
    if theirs:
      put(f'{name}_significant', (lower > 0) | (upper < 0), dims)
  return xl.like_input(out, *given)
