"""Writes tests/golden/reference_lead_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified weatherbench2/derived_variables.py for its two
lead-time classes (PrecipitationAccumulation,
AggregatePrecipitationAccumulation) on the seeded cases of
tests/lead_cases.py, one shard per case (a committed file stays below 1 MiB;
tests/lead_cases.load_golden reads them back as one dict).

As for reference_derived_v1, "the reference" means the reference's code on the
mini-xarray of oracle/refshim/ (xarray itself is absent here; see
make_derived_vectors.py, whose set-up this generator imports).  The stand-in's
`rolling` raises NotImplementedError; this generator gives the stand-in's
DataArray one at run time, in its own process, that restates xarray's default
NumPy path for `rolling({dim: w}).sum()` (min_periods = w): the sum over the
window axis of numpy's `sliding_window_view`, NaN where the window is
incomplete or holds a NaN, integers made float64 first.  It is THIS build's
reading of xarray, not xarray's code; its independent pins are the reference's
three known-answer tests (derived_variables_test.py:134-216), whose inputs
this generator runs through the reference and records as the case `known`.
Nothing under oracle/ changes.

Per case and label the file holds
  <case>/<label>/ref (+ /dims, /coords)  the reference on the case's inputs
and <case>/seed, <case>/shape; known/<label>/{ref, expected, dims}; and
structure: the reference's class names, fields, defaults, base_variables and
core_dims of the two classes plus its full list of dictionary keys.

Only runs where the reference is at hand:
    python tests/golden/make_lead_vectors.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_derived_vectors as base  # noqa: E402  (paths, stand-in, reference)

from tests import lead_cases as lc  # noqa: E402

ref_dv = base.ref_dv
xr = base.xr


class _Rolling:
  """`DataArray.rolling({dim: w})` with `sum()` alone."""

  def __init__(self, array, dim=None, min_periods=None, center=False, **kw):
    windows = dict(dim or {}, **kw)
    assert len(windows) == 1 and min_periods is None and not center
    (self.dim, self.window), = windows.items()
    self.array = array

  def sum(self):
    da = self.array
    axis = da.dims.index(self.dim)
    data = np.asarray(da.data)
    if data.dtype.kind != 'f':
      data = data.astype(np.float64)
    w = int(self.window)
    assert w >= 1
    out = np.full(data.shape, np.nan, dtype=data.dtype)
    if w <= data.shape[axis]:
      view = np.lib.stride_tricks.sliding_window_view(data, w, axis=axis)
      with np.errstate(all='ignore'):
        total = view.sum(axis=-1)
        total[np.isnan(view).any(axis=-1)] = np.nan
      at = [slice(None)] * data.ndim
      at[axis] = slice(w - 1, None)
      out[tuple(at)] = total
    return da.copy(data=out)


xr.DataArray.rolling = lambda self, *a, **k: _Rolling(self, *a, **k)


def to_dataset(case):
  return xr.Dataset({k: (d, a) for k, (d, a) in case['vars'].items()},
                    dict(case['coords']))


def run(label, case):
  name, kwargs = lc.CLASSES[label]
  with np.errstate(all='ignore'):
    return getattr(ref_dv, name)(**kwargs).compute(to_dataset(case))


def generate() -> dict:
  out = {}
  for label, known in lc.KNOWN_ANSWERS.items():
    res = run(label, known)
    np.testing.assert_array_equal(np.asarray(res.data), known['expected'])
    out[f'known/{label}/ref'] = np.asarray(res.data)
    out[f'known/{label}/expected'] = known['expected']
    out[f'known/{label}/dims'] = np.array(list(res.dims), dtype='U32')
  for cname, build in lc.cases().items():
    case = build()
    for label in case['labels']:
      key = f'{cname}/{label}'
      res = run(label, case)
      out[f'{key}/ref'] = np.asarray(res.data)
      out[f'{key}/dims'] = np.array(list(res.dims), dtype='U32')
      out[f'{key}/coords'] = np.array(sorted(res.coords), dtype='U32')
    out[f'{cname}/seed'] = np.array(case['seed'])
    out[f'{cname}/shape'] = np.array(
        case['vars']['total_precipitation'][1].shape)
  record = lc.structure(ref_dv, ref_dv.DERIVED_VARIABLE_DICT)
  record['keys'] = list(ref_dv.DERIVED_VARIABLE_DICT)
  out['structure/structure'] = np.array(json.dumps(record, sort_keys=True))
  return out


def shards(out: dict) -> dict:
  """{shard name: its arrays}: one per case, the structure record apart."""
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(key.split('/')[0], {})[key] = value
  return by_shard


def main():
  out = generate()
  directory = os.environ.get('WB2_LEAD_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{lc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')
  for cname, build in lc.cases().items():
    for label in build()['labels']:
      a = out[f'{cname}/{label}/ref']
      print(f'{cname:20s} {label:36s} -> {a.dtype}  NaN '
            f'{np.isnan(a).sum():4d}/{a.size}  inf {np.isinf(a).sum():3d}  '
            f'zeros {(a == 0).sum():4d}  negative {(a < 0).sum():4d}')


if __name__ == '__main__':
  main()
