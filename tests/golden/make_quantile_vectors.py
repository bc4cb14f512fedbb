"""Writes tests/golden/reference_quantile_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified scripts/compute_quantiles.py on the seeded cases
of tests/quantile_cases.py, one shard per case and one for the known-answer
cases (a committed file stays below 1 MiB; tests/quantile_cases.load_golden
reads them back as one dict).

Which of the two routes was taken: the PREFERRED one.  Every case with a list
of quantiles runs the reference's `_evaluate_chunk_core` itself (its two
checks, `chunk.quantile(quantiles, dim=..., skipna=...)`, the rename with
--name_suffix) on the mini-xarray of oracle/refshim/ (xarray itself is absent
here; see make_derived_vectors.py).  The script reads its arguments from
absl flags and imports apache_beam / xarray_beam for its pipeline; absl.flags
and absl.app do not exist here, so this generator supplies, in its own process
only, a module `absl.flags` whose DEFINE_* return plain holders with a
`.value` (set per case below) and an empty `absl.app`; apache_beam and
xarray_beam are the import-only stand-ins that oracle/refshim/ already has.
Nothing under oracle/ changes.  The one case with a scalar q (`scalar_q`; the
script only ever passes a list) calls the stand-in's `Dataset.quantile`
directly, which is the one xarray call the reference makes.

The stand-in's quantile is `np.quantile` / `np.nanquantile` with
method='linear' over the reduced axes: it is THIS build's reading of xarray.
Its independent pin is the reference's own test
(scripts/compute_quantiles_test.py), whose inputs are recorded as the cases
`known_<k>` (RandomState(802701 + k).rand(4, 50, 6), the first three times,
dim='lat', quantiles 0.2 and 0.8, once with name_suffix='_quantile') together
with what that test compares with: `quantile` of the input followed by
`rename_vars`.

Per case and mode (keepna / skipna) the files hold
  <case>/<mode>/<variable>  (+ /dims)  the reference's output variable
  <case>/<mode>/coords, <case>/<mode>/quantile   coordinate names, the
                                       quantile coordinate
known_<k>/<mode>/expected/<variable>   the test's own expectation
and structure/structure: output dims, dtypes and coordinate names per case.

Only runs where the reference is at hand:
    python tests/golden/make_quantile_vectors.py
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHIM = os.path.join(ROOT, 'oracle', 'refshim')
REFERENCE = os.environ.get('WB2_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)
sys.path.insert(0, SHIM)  # `import xarray` -> the mini-xarray


class _Flag:
  """What a DEFINE_* of absl.flags returns, as far as the script reads it."""

  def __init__(self, name, default):
    self.name, self.value = name, default


def _flags_module():
  flags = types.ModuleType('absl.flags')

  def define(name, default=None, help=None, **kwargs):  # pylint: disable=redefined-builtin
    return _Flag(name, default)

  for kind in ('string', 'list', 'boolean', 'integer', 'float', 'enum'):
    setattr(flags, 'DEFINE_' + kind, define)
  flags.DEFINE = lambda parser, name, default, help=None, **kw: _Flag(  # pylint: disable=redefined-builtin
      name, parser.parse(default) if isinstance(default, str) else default)
  flags.ArgumentParser = type('ArgumentParser', (), {})
  flags.ArgumentSerializer = type('ArgumentSerializer', (), {})
  flags.IllegalFlagValueError = type('IllegalFlagValueError', (ValueError,), {})
  flags.mark_flags_as_required = lambda names: None
  return flags


import absl  # noqa: E402  (the import-only stand-in of oracle/refshim/)

absl.flags = sys.modules['absl.flags'] = _flags_module()
absl.app = sys.modules['absl.app'] = types.ModuleType('absl.app')

import xarray as xr  # noqa: E402  (the stand-in)

assert 'wb2shim' in xr.__version__

_spec = importlib.util.spec_from_file_location(
    'wb2_reference_compute_quantiles',
    os.path.join(REFERENCE, 'scripts', 'compute_quantiles.py'))
ref_cq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_cq)
assert ref_cq.__file__.startswith(REFERENCE)

from tests import quantile_cases as qc  # noqa: E402


def to_dataset(case):
  return xr.Dataset({k: (d, a) for k, (d, a) in case['vars'].items()},
                    dict(case['coords']))


def run(case, skipna: bool):
  dim = [case['dim']] if isinstance(case['dim'], str) else list(case['dim'])
  ds = to_dataset(case)
  import warnings
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')  # (all-NaN slices; inf - inf)
    if case['scalar']:
      return ds.quantile(case['q'], dim=dim, skipna=skipna)
    ref_cq.DIM.value = dim
    ref_cq.QUANTILES.value = [repr(float(v)) for v in case['q']]
    ref_cq.SKIPNA.value = skipna
    ref_cq.NAME_SUFFIX.value = case['name_suffix']
    return ref_cq._evaluate_chunk_core(ds)  # pylint: disable=protected-access


def record(res) -> dict:
  out = {}
  for name in res:
    da = res[name]
    out[str(name)] = np.asarray(da.data)
    out[f'{name}/dims'] = np.array(list(da.dims), dtype='U32')
  out['coords'] = np.array(sorted(res.coords), dtype='U32')
  out[qc.QUANTILE] = np.asarray(res.coords[qc.QUANTILE].data)
  return out


def structure_of(res) -> dict:
  q = np.asarray(res.coords[qc.QUANTILE].data)
  return {'vars': {str(name): {'dims': list(res[name].dims),
                               'dtype': np.asarray(res[name].data).dtype.name}
                   for name in res},
          'coords': sorted(res.coords), 'quantile_dtype': q.dtype.name,
          'quantile_ndim': q.ndim}


def generate() -> dict:
  out, structure = {}, {}
  for cname, build in qc.all_cases().items():
    case = build()
    for mode, skipna in qc.MODES.items():
      res = run(case, skipna)
      for key, value in record(res).items():
        out[f'{cname}/{mode}/{key}'] = value
      mine = structure_of(res)
      assert structure.setdefault(cname, mine) == mine, cname
      assert mine == qc.expected_structure(case), (cname, mine)
      if cname.startswith('known'):
        # what compute_quantiles_test.py compares with
        with np.errstate(all='ignore'):
          want = to_dataset(case).quantile(
              qc.KNOWN_QUANTILES, dim='lat', skipna=skipna).rename_vars(
                  {'precip': 'precip' + case['name_suffix']})
        for name in want:
          np.testing.assert_array_equal(np.asarray(res[name].data),
                                        np.asarray(want[name].data))
          out[f'{cname}/{mode}/expected/{name}'] = np.asarray(want[name].data)
    out[f'{cname}/seed'] = np.array(case['seed'])
  # the reference's two errors
  case = qc.known(0)
  ref_cq.DIM.value, ref_cq.SKIPNA.value = ['lat'], False
  ref_cq.NAME_SUFFIX.value = ''
  for bad in (['-0.1'], ['0.5', '1.5']):
    ref_cq.QUANTILES.value = bad
    try:
      ref_cq._evaluate_chunk_core(to_dataset(case))  # pylint: disable=protected-access
    except ValueError as e:
      assert 'Expected all quantiles to be in [0, 1]' in str(e)
    else:
      raise AssertionError(bad)
  out['structure/structure'] = np.array(json.dumps(structure, sort_keys=True))
  return out


def shards(out: dict) -> dict:
  """{shard name: its arrays}: one per case, one for the known-answer cases,
  the structure record apart."""
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(qc.shard_of(key), {})[key] = value
  return by_shard


def main():
  out = generate()
  directory = os.environ.get('WB2_QUANTILE_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{qc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')
  for cname in qc.all_cases():
    for mode in qc.MODES:
      for key, a in out.items():
        head = f'{cname}/{mode}/'
        if (key.startswith(head) and a.dtype == np.float64 and a.ndim
            and '/' not in key[len(head):] and key != head + qc.QUANTILE):
          print(f'{cname:16s} {mode:7s} {key[len(head):]:22s} {a.shape}  NaN '
                f'{np.isnan(a).sum():4d}/{a.size}  inf {np.isinf(a).sum():3d}  '
                f'zeros {(a == 0).sum():4d}')


if __name__ == '__main__':
  main()
