"""Writes tests/golden/reference_slice_v1.json and one
reference_slice_v1.<case>.npz per case of tests/slice_cases.py: what the
REFERENCE's scripts/slice_dataset.py makes of the seeded inputs.

What runs: the script's own, unmodified `_get_selections` and
`_maybe_make_some_dims_increasing`, on the flag values of each case, and the
selection sequence of its `main` (:253-272) restated below call for call, on
the mini-xarray of oracle/refshim/ (xarray itself is absent here).  `main`
itself does not run (zarr and Beam).  absl.flags does not exist here either:
this generator supplies, in its own process only, the same flag stand-in as
make_time_indexing_vectors.py (DEFINE_* return plain holders with a
`.value`, set per case).

What the stand-in xarray lacks and this generator supplies, in its own
process only, from pandas' own `Index`: `Dataset.drop_isel` (`Index.delete`
of the positions) and `Dataset.drop_sel` (`Index.drop` of the labels, then
`get_indexer` of what is left).  `.sel` with a slice is the stand-in's, which
asks `Index.slice_indexer`.  Nothing under oracle/ changes.  So every label
rule in the fixtures -- inclusive bounds, decreasing axes, partial date
strings, timedelta strings -- is pandas' (the version is recorded).

The `known_*` cases are the inputs and expected results of the reference's
own GetSelectionsTest and SliceDatasetTest (data only): the expected datasets
are computed here the way those tests compute them, and asserted equal to what
the sequence gives.

Only runs where the reference and pandas are at hand:
    python tests/golden/make_slice_vectors.py
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np
import pandas as pd

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

  for kind in ('string', 'list', 'boolean', 'bool', 'integer', 'float'):
    setattr(flags, 'DEFINE_' + kind, define)
  flags.DEFINE = lambda parser, name, default, help=None, **kw: _Flag(  # pylint: disable=redefined-builtin
      name, parser.parse(default) if isinstance(default, str) else default)
  flags.ArgumentParser = type('ArgumentParser', (), {})
  flags.ArgumentSerializer = type('ArgumentSerializer', (), {})
  flags.IllegalFlagValueError = type('IllegalFlagValueError', (ValueError,), {})
  flags.mark_flags_as_required = lambda names: None
  flags.mark_flags_as_mutual_exclusive = lambda names: None
  return flags


import absl  # noqa: E402  (the import-only stand-in of oracle/refshim/)

absl.flags = sys.modules['absl.flags'] = _flags_module()
absl.app = sys.modules['absl.app'] = types.ModuleType('absl.app')

import xarray as xr  # noqa: E402  (the stand-in)

assert 'wb2shim' in xr.__version__

from tests import slice_cases  # noqa: E402


def _load(name):
  spec = importlib.util.spec_from_file_location(
      'wb2_reference_' + name, os.path.join(REFERENCE, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  assert module.__file__.startswith(REFERENCE)
  return module


def _index_of(ds, dim) -> pd.Index:
  return pd.Index(ds[dim].data)


def _drop_isel(ds, indexers):
  """xarray's Dataset.drop_isel: the positions leave the axis."""
  for dim, positions in indexers.items():
    keep = pd.RangeIndex(ds.sizes[dim]).delete(positions)
    ds = ds.isel({dim: np.asarray(keep, dtype=np.int64)})
  return ds


def _drop_sel(ds, labels):
  """xarray's Dataset.drop_sel: `Index.drop` of the labels (KeyError for an
  absent one), then the positions of what is left."""
  for dim, values in labels.items():
    index = _index_of(ds, dim)
    left = index.drop(values)
    ds = ds.isel({dim: index.get_indexer(left).astype(np.int64)})
  return ds


def _to_xr(description):
  coords = {}
  for name, c in description['coords'].items():
    coords[name] = c if isinstance(c, tuple) else np.asarray(c)
  return xr.Dataset({k: v for k, v in description['vars'].items()}, coords)


def _names(value):
  return [n for n in (value or '').split(',') if n]


def run_main_sequence(script, parse, ds, options):
  """scripts/slice_dataset.py:253-272 on `ds`."""
  for flag in ('SEL', 'SEL_STRINGS', 'ISEL', 'DROP_SEL', 'DROP_SEL_STRINGS',
               'DROP_ISEL'):
    getattr(script, flag).value = parse(options.get(flag.lower(), ''))
  script.MAKE_DIMS_INCREASING.value = _names(
      options.get('make_dims_increasing'))
  script.DROP_VARIABLES.value = _names(options.get('drop_variables')) or None
  script.KEEP_VARIABLES.value = _names(options.get('keep_variables')) or None

  ds = script._maybe_make_some_dims_increasing(ds)
  if script.DROP_VARIABLES.value:
    ds = ds.drop_vars(script.DROP_VARIABLES.value)
  elif script.KEEP_VARIABLES.value:
    ds = ds[script.KEEP_VARIABLES.value]
  get = script._get_selections
  for selection in get(script.ISEL.value, force_string=False):
    ds = ds.isel(selection)
  for selection in get(script.SEL.value, force_string=False):
    ds = ds.sel(selection)
  for selection in get(script.SEL_STRINGS.value, force_string=True):
    ds = ds.sel(selection)
  for selection in get(script.DROP_ISEL.value, force_string=False):
    ds = _drop_isel(ds, selection)
  for selection in get(script.DROP_SEL.value, force_string=False):
    ds = _drop_sel(ds, selection)
  for selection in get(script.DROP_SEL_STRINGS.value, force_string=True):
    ds = _drop_sel(ds, selection)
  return ds


def _known_expected(name, ds):
  """The expected dataset as the reference's test computes it, from the
  input BEFORE the test reverses its latitude."""
  if name == 'known_simple':
    return ds.sel(time=slice('2021-02-01', '2021-04-01', 5),
                  longitude=slice(None, None, 60)).isel(
                      latitude=slice(5))[['temperature', 'geopotential']]
  return _drop_isel(ds.sel(longitude=[60, 150]),
                    {'latitude': [-1]})[['temperature', 'geopotential']]


def main():
  script = _load('slice_dataset')
  from weatherbench2 import flag_utils
  parse = flag_utils._parse_dim_value_pairs  # pylint: disable=protected-access
  meta = {'pandas': pd.__version__, 'cases': {}, 'known_selections': {},
          'parsed': {}}

  for name, (flag_values, force) in slice_cases.KNOWN_SELECTIONS.items():
    got = script._get_selections(dict(flag_values), force_string=force)
    meta['known_selections'][name] = [slice_cases.encode_selection(s)
                                      for s in got]
  # what the flag parser makes of every option string of the cases
  for name in slice_cases.CASES:
    for key, value in slice_cases.options(name).items():
      if key.endswith('variables') or key == 'make_dims_increasing':
        continue
      meta['parsed'][value] = parse(value)

  for name in slice_cases.CASES:
    options = slice_cases.options(name)
    ds = _to_xr(slice_cases.build(name))
    out = run_main_sequence(script, parse, ds, options)
    if name.startswith('known_'):
      plain = _to_xr(slice_cases.mock_truth())
      want = _known_expected(name, plain)
      assert list(want.data_vars) == list(out.data_vars)
      for k in want.data_vars:
        assert want[k].dims == out[k].dims, (name, k)
        np.testing.assert_array_equal(want[k].data, out[k].data)
      for k in ('time', 'latitude', 'longitude', 'level'):
        np.testing.assert_array_equal(want[k].data, out[k].data)
      chunks = {k: v for k, v in slice_cases.KNOWN_CHUNKS['input'].items()
                if k in out.dims}
      over = slice_cases.KNOWN_CHUNKS['overrides']
      meta.setdefault('known_chunks', {})[name] = {
          k: over[k] if k in over else min(v, out.sizes[k])
          for k, v in chunks.items()}
    arrays, dims, coord_dims = {}, {}, {}
    for k in out.data_vars:
      arrays['var/' + k] = np.asarray(out[k].data)
      dims[k] = list(out[k].dims)
    for k in out.coords:
      arrays['coord/' + k] = np.asarray(out.coords[k].data)
      coord_dims[k] = list(out.coords[k].dims)
    meta['cases'][name] = {'options': options, 'order': list(out.data_vars),
                           'dims': dims, 'coord_dims': coord_dims,
                           'sizes': {k: int(v) for k, v in out.sizes.items()}}
    path = os.path.join(HERE, f'{slice_cases.PREFIX}.{name}.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < (1 << 20), path
    print(name, dict(out.sizes), os.path.getsize(path))

  with open(os.path.join(HERE, slice_cases.PREFIX + '.json'), 'w') as f:
    json.dump(meta, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
