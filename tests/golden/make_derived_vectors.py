"""Writes tests/golden/reference_derived_v1.<shard>.npz: outputs of the
REFERENCE's own, unmodified weatherbench2/derived_variables.py on the seeded
cases of tests/derived_cases.py (one shard per case, two for the largest: a
committed file stays below 1 MiB; tests/derived_cases.load_golden reads them
back as one dict).

As for reference_vectors_v1.npz, "the reference" means the reference's code
on the mini-xarray of oracle/refshim/ (xarray itself is absent here).  That
stand-in has `integrate`, `sel`, `mean`, `where` and `copy(data=)` but no
`differentiate`; this generator adds that one method to the stand-in's
DataArray at run time as np.gradient(data, coordinate, axis, edge_order) --
which is what xarray's own `differentiate` calls, but it is THIS build's
reading of xarray, not xarray's code.  Nothing under oracle/ changes.

Per class label and case the file holds
  <case>/<label>/ref32 (+ /dims, /coords)  the reference on float32 inputs
  <case>/<label>/ref64                     ... on the same values as float64
(float64 cases: ref64 alone; the dtype of an array is part of the record),
and known/<label>/{ref, expected}: the reference on the inputs of its own
unit tests (derived_variables_test.py:85-119).  For every class and float32
case `noise / rms < 1e-4` is asserted, noise = max |ref32 - ref64| over the
finite points: the tests' tolerance is a multiple of that noise.

Only runs where the reference is at hand:
    python tests/golden/make_derived_vectors.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHIM = os.path.join(ROOT, 'oracle', 'refshim')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)
sys.path.insert(0, SHIM)  # `import xarray` -> the mini-xarray

import xarray as xr  # noqa: E402  (the stand-in)
from weatherbench2 import derived_variables as ref_dv  # noqa: E402

from tests import derived_cases as dc  # noqa: E402

assert 'wb2shim' in xr.__version__
assert ref_dv.__file__.startswith(REFERENCE)


def _differentiate(self, coord, edge_order=1):
  axis = self.dims.index(coord)
  data = np.gradient(self.data, np.asarray(self.coords[coord].data),
                     axis=axis, edge_order=edge_order)
  return self.copy(data=data)


if not hasattr(xr.DataArray, 'differentiate'):
  xr.DataArray.differentiate = _differentiate


def to_dataset(case):
  used = set()
  for dims, _ in case['vars'].values():
    used |= set(dims)
  return xr.Dataset({k: (d, a) for k, (d, a) in case['vars'].items()},
                    {k: v for k, v in case['coords'].items() if k in used})


def run(label, case):
  name, kwargs = dc.CLASSES[label]
  with np.errstate(all='ignore'):
    return getattr(ref_dv, name)(**kwargs).compute(to_dataset(case))


def generate() -> dict:
  out = {}
  for cname, build in dc.cases().items():
    case = build()
    for label in dc.CLASSES:
      key = f'{cname}/{label}'
      if case['dtype'] == 'float32':
        r32 = run(label, case)
        r64 = run(label, dc.as_float64(case))
        a32, a64 = np.asarray(r32.data), np.asarray(r64.data)
        assert r32.dims == r64.dims
        np.testing.assert_array_equal(np.isfinite(a32), np.isfinite(a64))
        ok = np.isfinite(a64)
        noise = np.abs(a32[ok].astype(np.float64) - a64[ok]).max()
        rms = np.sqrt(np.mean(a64[ok] ** 2))
        assert noise / rms < 1e-4, (key, noise / rms)
        out[f'{key}/ref32'] = a32
        ref = r32
      else:
        r64 = run(label, case)
        ref = r64
      out[f'{key}/ref64'] = np.asarray(r64.data)
      out[f'{key}/dims'] = np.array(list(ref.dims), dtype='U32')
      out[f'{key}/coords'] = np.array(sorted(ref.coords), dtype='U32')
    out[f'{cname}/seed'] = np.array(case['seed'])
    out[f'{cname}/shape'] = np.array(
        case['vars']['u_component_of_wind'][1].shape)
  for label, known in dc.KNOWN_ANSWERS.items():
    res = run(label, known)
    np.testing.assert_allclose(np.asarray(res.data), known['expected'],
                               atol=known['atol'], rtol=0)
    out[f'known/{label}/ref'] = np.asarray(res.data)
    out[f'known/{label}/expected'] = known['expected']
    out[f'known/{label}/dims'] = np.array(list(res.dims), dtype='U32')
  import json
  out['known/structure'] = np.array(json.dumps(dc.structure(ref_dv), sort_keys=True))
  return out


def shards(out: dict) -> dict:
  """{shard name: its arrays}."""
  by_shard: dict = {}
  for key, value in out.items():
    parts = key.split('/')
    if parts[0] == 'known':
      shard = 'known'
    elif parts[1] in dc.CLASSES:
      shard = dc.shard_of(parts[0], parts[1])
    else:  # seed / shape of a case
      shard = dc.shard_of(parts[0], 'wind_speed')
    by_shard.setdefault(shard, {})[key] = value
  return by_shard


def main():
  out = generate()
  directory = os.environ.get('WB2_DERIVED_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{dc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')
  for cname in dc.cases():
    for label in dc.CLASSES:
      if f'{cname}/{label}/ref32' in out:
        a32 = out[f'{cname}/{label}/ref32'].astype(np.float64)
        a64 = out[f'{cname}/{label}/ref64']
        ok = np.isfinite(a64)
        print(f'{cname:16s} {label:34s} {a32.dtype} -> '
              f'{out[f"{cname}/{label}/ref32"].dtype}  non-finite '
              f'{(~ok).sum():4d}/{ok.size}  noise/rms '
              f'{np.abs(a32[ok] - a64[ok]).max() / np.sqrt(np.mean(a64[ok] ** 2)):.2e}')


if __name__ == '__main__':
  main()
