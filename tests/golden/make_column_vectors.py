"""Writes tests/golden/reference_column_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified weatherbench2/derived_variables.py for its
level-column classes (TotalColumnWater, IntegratedWaterTransport, LapseRate,
VerticalVelocity, EddyKineticEnergy) on the seeded cases of
tests/column_cases.py, one shard per case (a committed file stays below
1 MiB; tests/column_cases.load_golden reads them back as one dict).

As for reference_derived_v1, "the reference" means the reference's code on the
mini-xarray of oracle/refshim/ (xarray itself is absent here), with
`differentiate` added to the stand-in's DataArray at run time as np.gradient
(see make_derived_vectors.py, whose set-up this generator imports).  What a
label slice selects -- `sel(level=slice(300, 1000))` -- is the stand-in's
reading too: it asks pandas' `Index.slice_indexer`, which selects NOTHING for
such bounds on a decreasing level coordinate; the `decreasing` case pins that.

Per label and case the file holds
  <case>/<label>/ref32 (+ /dims, /coords)  the reference on float32 inputs
  <case>/<label>/ref64                     ... on the same values as float64
(float64 cases: ref64 alone; the dtype of an array is part of the record), and
structure: the reference's class names, fields, defaults, base_variables and
core_dims of the five classes plus its full list of dictionary keys.

For the (case, label) pairs of column_cases.ZERO the reference's result is
identically 0.0 and the generator asserts that; for every other pair of a
float32 case it asserts a non-zero rms and `noise / rms < 1e-4`, noise =
max |ref32 - ref64| over the finite points: the tests' tolerance is a
multiple of that noise.

Only runs where the reference is at hand:
    python tests/golden/make_column_vectors.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_derived_vectors as base  # noqa: E402  (paths, stand-in, reference)

from tests import column_cases as cc  # noqa: E402

ref_dv = base.ref_dv


def run(label, case):
  name, kwargs = cc.CLASSES[label]
  with np.errstate(all='ignore'):
    return getattr(ref_dv, name)(**kwargs).compute(base.to_dataset(case))


def _noise_and_rms(a32, a64):
  ok = np.isfinite(a64)
  noise = np.abs(a32[ok].astype(np.float64) - a64[ok]).max()
  return noise, np.sqrt(np.mean(a64[ok] ** 2))


def generate() -> dict:
  out = {}
  for cname, build in cc.cases().items():
    case = build()
    for label in cc.CLASSES:
      key = f'{cname}/{label}'
      zero = (cname, label) in cc.ZERO
      if case['dtype'] == 'float32':
        r32 = run(label, case)
        r64 = run(label, cc.as_float64(case))
        a32, a64 = np.asarray(r32.data), np.asarray(r64.data)
        assert r32.dims == r64.dims
        np.testing.assert_array_equal(np.isfinite(a32), np.isfinite(a64))
        if zero:
          assert (a32 == 0).all() and (a64 == 0).all(), key
        else:
          noise, rms = _noise_and_rms(a32, a64)
          assert rms > 0 and noise / rms < 1e-4, (key, noise, rms)
        out[f'{key}/ref32'] = a32
        ref = r32
      else:
        r64 = run(label, case)
        assert not zero
        ref = r64
      out[f'{key}/ref64'] = np.asarray(r64.data)
      out[f'{key}/dims'] = np.array(list(ref.dims), dtype='U32')
      out[f'{key}/coords'] = np.array(sorted(ref.coords), dtype='U32')
    out[f'{cname}/seed'] = np.array(case['seed'])
    out[f'{cname}/shape'] = np.array(
        case['vars']['u_component_of_wind'][1].shape)
    out[f'{cname}/level'] = np.asarray(case['coords']['level'])
  record = cc.structure(ref_dv, ref_dv.DERIVED_VARIABLE_DICT)
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
  directory = os.environ.get('WB2_COLUMN_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{cc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')
  for cname in cc.cases():
    for label in cc.CLASSES:
      if f'{cname}/{label}/ref32' in out:
        a32 = out[f'{cname}/{label}/ref32']
        a64 = out[f'{cname}/{label}/ref64']
        noise, rms = _noise_and_rms(a32, a64)
        print(f'{cname:16s} {label:28s} -> {a32.dtype}  non-finite '
              f'{(~np.isfinite(a64)).sum():4d}/{a64.size}  noise/rms '
              + ('(all zeros)' if rms == 0 else f'{noise / rms:.2e}'))


if __name__ == '__main__':
  main()
