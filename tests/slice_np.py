"""NumPy twins of the slicing path: `np.take` and nothing else."""
import numpy as np


def box_gather(x: np.ndarray, src_slab=None, rows=None, cols=None
               ) -> np.ndarray:
  """[n_out_slab, n_row_out, n_col_out] of a [n_slab, n_row, n_col] array:
  one take per table (None: identity)."""
  out = x
  for axis, table in enumerate((src_slab, rows, cols)):
    if table is not None:
      out = np.take(out, np.asarray(table, dtype=np.int64), axis=axis)
  return np.ascontiguousarray(out)


def run(col0: int, step: int, count: int) -> np.ndarray:
  """The columns of an affine run."""
  return col0 + step * np.arange(count, dtype=np.int64)


def take(values: np.ndarray, dims, positions: dict) -> np.ndarray:
  """`values` with every dim of `positions` cut to those positions."""
  for axis, d in enumerate(dims):
    if d in positions:
      values = np.take(values, positions[d], axis=axis)
  return values


def same_bits(a, b) -> bool:
  """Equal shape, dtype and bytes: NaN payloads and -0.0 included."""
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and (
      a.tobytes() == b.tobytes())
