"""Writes tests/golden/reference_resample_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified scripts/resample_in_time.py on the seeded cases of
tests/resample_cases.py, one shard per case and one for the known-answer cases
(a committed file stays below 1 MiB; tests/resample_cases.load_golden reads
them back as one dict).

Every case runs the reference's `resample_in_time_chunk` (and through it
`resample_in_time_core`) once per variable, as its pipeline does with
split_vars=True, on the mini-xarray of oracle/refshim/ (xarray itself is
absent here; see make_derived_vectors.py), with a small key object of this
file's own that has `with_offsets`; `resample_in_time_core` is also called on
the whole dataset and must agree.  The script reads --time_dim and
--label_side from absl flags and imports apache_beam / xarray_beam for its
pipeline; absl.flags and absl.app do not exist here, so this generator
supplies, in its own process only, the same flag stand-in as
make_quantile_vectors.py (DEFINE_* return plain holders with a `.value`, set
per case below).  Nothing under oracle/ changes.

The stand-in's `resample` and `rolling` raise NotImplementedError.  This
generator gives the stand-in its own versions, in its own process only:
  * bin membership comes from pandas' own `Series.resample(period, label=,
    closed=)` grouping of the positions 0 .. n-1, which is what xarray groups
    by; the statistic of a bin is the stand-in's own mean / sum / min / max
    (skipna=) over that slice of the time dim; a bin without members (a gap)
    is NaN in every statistic, `sum` included;
  * rolling is a `sliding_window_view`, the stand-in's own reduction over the
    window axis, NaN where fewer than w samples of the window are not NaN
    (min_periods=None) and for the first w - 1 outputs.
This is THIS build's reading of xarray.  Its independent pins are pandas (the
bins, and the float64 values in tests/test_resampling_cpu.py) and the
reference's own known-answer test (scripts/resample_in_time_test.py:30-189),
whose inputs are the cases `known_*`: the ten-day 3d case with and without the
NaN, and the seven (n_times, period, nan_locations) combinations with
RandomState(802701), each as resample and as rolling.  For those the generator
asserts what that test asserts (the labels and means it spells out; resample
and rolling, after `main`'s label shift, agree at their common times, of which
at most one resample label is missing).

Per case and mode (keepna / skipna) the files hold
  <case>/<mode>/<output variable>  (+ /dims)  the reference's output
  <case>/<mode>/coords, <case>/<mode>/labels   coordinate names, the time
                                               labels of the result

Only runs where the reference is at hand:
    python tests/golden/make_resample_vectors.py
"""
import importlib.util
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

  def define_enum(name, default, enum_values, help=None, **kwargs):  # pylint: disable=redefined-builtin
    return _Flag(name, default)

  for kind in ('string', 'list', 'boolean', 'bool', 'integer', 'float'):
    setattr(flags, 'DEFINE_' + kind, define)
  flags.DEFINE_enum = define_enum
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


# ---------------------------------------------------------------------------
# resample and rolling for the stand-in (this process only)
# ---------------------------------------------------------------------------
def _variables(obj):
  """[(name, DataArray)] of a Dataset, or the DataArray itself."""
  if isinstance(obj, xr.Dataset):
    return [(k, obj[k]) for k in obj.data_vars], True
  return [(obj.name, obj)], False


def _rebuild(obj, dim, new_index, arrays):
  """`obj` with `dim` relabelled by `new_index` and the data of `arrays`."""
  variables, is_dataset = _variables(obj)

  def coords_of(da):
    out = {k: (tuple(c.dims), np.asarray(c.data)) for k, c in da.coords.items()
           if dim not in tuple(c.dims)}
    if dim in da.dims:
      out[dim] = ((dim,), np.asarray(new_index))
    return out

  made = {k: xr.DataArray(arrays[k], coords=coords_of(da), dims=da.dims,
                          name=k) for k, da in variables}
  if not is_dataset:
    return made[variables[0][0]]
  return xr.Dataset(made)


class _Resample:

  def __init__(self, obj, indexer=None, label=None, closed=None, **kw):
    (self.dim, self.freq), = dict(indexer or {}, **kw).items()
    self.obj, self.label, self.closed = obj, label, closed

  def _bins(self):
    index = pd.Index(np.asarray(self.obj[self.dim].data))
    positions = pd.Series(np.arange(len(index)), index=index)
    table = positions.resample(self.freq, label=self.label,
                               closed=self.closed).agg(['min', 'max', 'count'])
    ranges = [(int(lo), int(hi) + 1) if n else None
              for lo, hi, n in zip(table['min'], table['max'], table['count'])]
    return table.index.values, ranges

  def _reduce(self, statistic, skipna):
    labels, ranges = self._bins()
    dim, arrays = self.dim, {}
    for name, da in _variables(self.obj)[0]:
      if dim not in da.dims:
        arrays[name] = np.asarray(da.data)
        continue
      axis = da.dims.index(dim)
      rest = tuple(n for i, n in enumerate(da.shape) if i != axis)
      pieces = []
      for r in ranges:
        if r is None:
          pieces.append(np.full(rest, np.nan))
        else:
          piece = da.isel({dim: slice(*r)})
          pieces.append(np.asarray(
              getattr(piece, statistic)(dim, skipna=skipna).data))
      arrays[name] = np.stack(pieces, axis=axis)
    return _rebuild(self.obj, dim, labels, arrays)


class _Rolling:

  def __init__(self, obj, dim=None, min_periods=None, center=False, **kw):
    (self.dim, self.window), = dict(dim or {}, **kw).items()
    assert min_periods is None and not center
    self.obj = obj

  def _reduce(self, statistic, skipna):
    dim, w, arrays = self.dim, int(self.window), {}
    for name, da in _variables(self.obj)[0]:
      data = np.asarray(da.data)
      if dim not in da.dims:
        arrays[name] = data
        continue
      axis = da.dims.index(dim)
      out = np.full(data.shape, np.nan,
                    dtype=data.dtype if data.dtype.kind == 'f' else np.float64)
      if w <= data.shape[axis]:
        windows = np.lib.stride_tricks.sliding_window_view(data, w, axis=axis)
        wide = xr.DataArray(windows, dims=tuple(da.dims) + ('_window',))
        value = np.asarray(getattr(wide, statistic)('_window',
                                                    skipna=skipna).data)
        count = (~np.isnan(windows)).sum(axis=-1)
        value = np.where(count >= w, value, np.nan).astype(out.dtype)
        at = [slice(None)] * data.ndim
        at[axis] = slice(w - 1, None)
        out[tuple(at)] = value
      arrays[name] = out
    return _rebuild(self.obj, dim, np.asarray(self.obj[dim].data), arrays)


for _cls in (_Resample, _Rolling):
  for _stat in ('mean', 'min', 'max', 'sum'):
    setattr(_cls, _stat,
            lambda self, skipna=None, _stat=_stat: self._reduce(_stat, skipna))
for _cls in (xr.DataArray, xr.Dataset):
  _cls.resample = lambda self, *a, **k: _Resample(self, *a, **k)
  _cls.rolling = lambda self, *a, **k: _Rolling(self, *a, **k)

_spec = importlib.util.spec_from_file_location(
    'wb2_reference_resample_in_time',
    os.path.join(REFERENCE, 'scripts', 'resample_in_time.py'))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
assert ref.__file__.startswith(REFERENCE)

from tests import resample_cases as rc  # noqa: E402


class _Key:
  """As much of xarray_beam.Key as `resample_in_time_chunk` uses."""

  def __init__(self, offsets):
    self.offsets = dict(offsets)

  def with_offsets(self, **offsets):
    new = dict(self.offsets)
    for k, v in offsets.items():
      if v is None:
        new.pop(k, None)
      else:
        new[k] = v
    return _Key(new)


def to_dataset(case, names=None):
  return xr.Dataset({k: (d, a) for k, (d, a) in case['vars'].items()
                     if names is None or k in names}, dict(case['coords']))


def run(case, skipna: bool):
  """{output name: DataArray} in the reference's order, and the labels."""
  import warnings
  ref.TIME_DIM.value = case['time_dim']
  ref.LABEL_SIDE.value = case['label_side']
  period = pd.to_timedelta(case['period'])
  stats = case['stats']
  out = {}
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')  # (all-NaN slices)
    for name, (dims, _) in case['vars'].items():
      if case['time_dim'] not in dims or not any(
          name in stats[s] for s in rc.STATS):
        continue
      key = _Key({d: 0 for d in dims})
      new_key, res = ref.resample_in_time_chunk(
          key, to_dataset(case, [name]), case['method'], period,
          case['time_dim'], stats['mean'], stats['min'], stats['max'],
          stats['sum'], case['add_mean_suffix'], skipna=skipna)
      assert case['time_dim'] not in new_key.offsets
      for k in res.data_vars:
        assert k not in out, k
        out[str(k)] = res[k]
    # the core on the whole dataset: the same means, the others untouched
    whole = ref.resample_in_time_core(to_dataset(case), case['method'], period,
                                      'mean', skipna=skipna)
    for name, (dims, array) in case['vars'].items():
      mean_name = name + ('_mean' if case['add_mean_suffix'] else '')
      if case['time_dim'] not in dims:
        np.testing.assert_array_equal(np.asarray(whole[name].data), array)
      elif name in stats['mean']:
        np.testing.assert_array_equal(np.asarray(whole[name].data),
                                      np.asarray(out[mean_name].data))
  labels = np.asarray(whole[case['time_dim']].data)
  for da in out.values():
    np.testing.assert_array_equal(np.asarray(da[case['time_dim']].data), labels)
  return out, labels


def record(res: dict, labels) -> dict:
  out = {}
  coords = set()
  for name, da in res.items():
    out[name] = np.asarray(da.data)
    out[f'{name}/dims'] = np.array(list(da.dims), dtype='U32')
    coords.update(str(c) for c in da.coords)
  out['coords'] = np.array(sorted(coords), dtype='U32')
  out['labels'] = np.asarray(labels)
  return out


def _shifted(case, labels):
  """`main`'s label shift for rolling (:336-352)."""
  times = pd.DatetimeIndex(case['coords']['time'])
  delta_t = times[1] - times[0]
  period = pd.to_timedelta(case['period'])
  assert case['label_side'] == 'left'
  return (pd.DatetimeIndex(labels) - period + delta_t).values


def check_known(results: dict):
  """What resample_in_time_test.py:30-189 asserts."""
  for nan in ('clean', 'nan'):
    case = rc.known_ten_days(nan == 'nan', 'resample')
    temperatures = case['vars']['temperature'][1]
    res, labels = results[f'known_ten_{nan}_resample']['keepna']
    np.testing.assert_array_equal(
        labels, np.array(['2023-01-01', '2023-01-04', '2023-01-07',
                          '2023-01-10'], dtype='datetime64[ns]'))
    np.testing.assert_array_equal(
        np.asarray(res['temperature'].data),
        [np.mean(temperatures[:3]), np.mean(temperatures[3:6]),
         np.mean(temperatures[6:9]), np.mean(temperatures[9:12])])
  names = [f'known_ten_{nan}' for nan in ('clean', 'nan')] + [
      f'known_{k}' for k in range(len(rc.KNOWN_COMBINATIONS))]
  for name in names:
    case = rc.all_cases()[name + '_rolling']()
    res_a, labels_a = results[name + '_resample']['keepna']
    res_b, labels_b = results[name + '_rolling']['keepna']
    labels_b = _shifted(case, labels_b)
    common = np.intersect1d(labels_a, labels_b)
    assert len(common) >= len(labels_a) - 1, name
    a = np.asarray(res_a['temperature'].data)[np.isin(labels_a, common)]
    b = np.asarray(res_b['temperature'].data)[np.isin(labels_b, common)]
    np.testing.assert_array_equal(a, b, err_msg=name)


def generate() -> dict:
  out, results = {}, {}
  for cname, build in rc.all_cases().items():
    case = build()
    for mode, skipna in rc.MODES.items():
      res, labels = run(case, skipna)
      results.setdefault(cname, {})[mode] = (res, labels)
      for key, value in record(res, labels).items():
        out[f'{cname}/{mode}/{key}'] = value
    out[f'{cname}/seed'] = np.array(case['seed'])
  check_known(results)
  # the reference's errors
  case = rc.all_cases()['rolling_4']()
  ref.TIME_DIM.value, ref.LABEL_SIDE.value = 'time', 'left'
  for method, period, text in (('nearest', '1d', 'Unhandled method'),
                               ('rolling', '7h', 'did not evenly divide')):
    try:
      ref.resample_in_time_core(to_dataset(case), method,
                                pd.to_timedelta(period), 'mean', skipna=False)
    except ValueError as e:
      assert text in str(e), e
    else:
      raise AssertionError(method)
  ref.LABEL_SIDE.value = 'middle'
  try:
    ref.resample_in_time_core(to_dataset(case), 'resample',
                              pd.to_timedelta('1d'), 'mean', skipna=False)
  except ValueError as e:
    assert 'Unhandled' in str(e), e
  else:
    raise AssertionError('label_side')
  for bad in (['ALL', 'x'],):
    try:
      ref._get_vars(bad, ['x'])  # pylint: disable=protected-access
    except ValueError as e:
      assert 'Cannot specify both ALL and other variables' in str(e)
    else:
      raise AssertionError(bad)
  assert ref._get_vars(['ALL'], ['x', 'y']) == ['x', 'y']  # pylint: disable=protected-access
  return out


def shards(out: dict) -> dict:
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(rc.shard_of(key), {})[key] = value
  return by_shard


def main():
  out = generate()
  directory = os.environ.get('WB2_RESAMPLE_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{rc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')


if __name__ == '__main__':
  main()
