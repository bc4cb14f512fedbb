"""Writes tests/golden/reference_climatology_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified weatherbench2/utils.py:73-287 and of
scripts/compute_climatology.py's `compute_stat_chunk` on the seeded cases of
tests/climatology_cases.py, one shard per case (a committed file stays below
1 MiB; tests/climatology_cases.load_golden reads them back as one dict).

Every case runs `compute_stat_chunk` once per method ('explicit', 'fast': the
script's --method flag) and statistic ('mean', 'std') on the mini-xarray of
oracle/refshim/ (xarray itself is absent here; see make_derived_vectors.py),
with a small key object of this file's own; the utils function the script
dispatches to is also called directly and must agree.  absl.flags and
absl.app do not exist here, so this generator supplies, in its own process
only, the same flag stand-in as the other generators.  Nothing under oracle/
changes.

The stand-in lacks a weighted std, `groupby`, `rolling(...).construct`,
`resample`, `pad` and a Dataset's `roll`.  This generator gives the stand-in its own versions, in
its own process only:
  * weighted std / var: xarray/core/weighted.py's _sum_of_squares and
    _weighted_var, spelt with the stand-in's own weighted mean and reduction;
  * groupby('time.dayofyear').mean() / .std(): the groups are the sorted
    unique values of pandas' DatetimeIndex.dayofyear, the statistic of a group
    the stand-in's own mean / std over that selection of the time dim;
  * resample(time='D').mean(): bin membership from pandas' own
    `Series.resample('D')` grouping of the positions, the stand-in's own mean
    per bin, NaN for a bin without members;
  * pad(mode='wrap'): np.pad(mode='wrap') of the data and of the coordinate;
  * Dataset.roll: the stand-in's DataArray.roll (np.roll), per variable;
  * rolling(dim=W, center=True).construct('window'): a sliding_window_view of
    the NaN-padded data, window i centred on i.
All label semantics (partial-string `sel`, `.dt` fields, the outer join of
`concat`) come from pandas through the stand-in.  This is THIS build's reading
of xarray.  Its independent pins are the reference's own testMethodEquivalence
(weatherbench2/utils_test.py:24-47), whose input is recorded as the case
`known` and whose assertion is made here, and the per-point pandas
transcription in tests/test_climatology_cpu.py.

Per case the files hold
  <case>/<method>/<stat>  (+ /dims)      the reference's output
  <case>/<method>/<stat>/dayofyear, /hour  its labels (the stand-in's
                                         weighted reduction drops the
                                         day-of-year labels: `fast` only)
and `known/times`, `known/data` for the recorded input.

Only runs where the reference is at hand:
    python tests/golden/make_climatology_vectors.py
"""
import importlib.util
import os
import sys
import types
import warnings

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
# what the stand-in lacks (this process only)
# ---------------------------------------------------------------------------
def _each(obj, fn):
  """fn over the variables of a Dataset that it applies to, or a DataArray."""
  if isinstance(obj, xr.Dataset):
    return xr.Dataset({k: fn(obj[k]) for k in obj.data_vars})
  return fn(obj)


def _rebuilt(da, dim, data, labels, new_dim=None):
  """`da` with the axis `dim` replaced by `data`'s and relabelled."""
  new_dim = new_dim or dim
  coords = {k: (tuple(c.dims), np.asarray(c.data)) for k, c in da.coords.items()
            if dim not in tuple(c.dims)}
  coords[new_dim] = ((new_dim,), np.asarray(labels))
  dims = tuple(new_dim if d == dim else d for d in da.dims)
  return xr.DataArray(data, coords=coords, dims=dims, name=da.name)


def _weighted_var(self, da, dim, skipna):
  demeaned = da - da.weighted(self.weights).mean(dim=dim)
  sum_of_squares = self._reduce(demeaned**2, self.weights, dim=dim,
                                skipna=skipna)
  return sum_of_squares / self._sum_of_weights(da, dim=dim)


def _weighted_std(self, da, dim, skipna):
  return np.sqrt(self._weighted_var(da, dim, skipna))


_Weighted = type(xr.DataArray(np.zeros(1), dims=['a']).weighted(
    xr.DataArray(np.ones(1), dims=['a'])))
_Weighted._weighted_var = _weighted_var
_Weighted._weighted_std = _weighted_std
_Weighted.var = lambda self, dim=None, *, skipna=None, keep_attrs=None: (
    self._apply(self._weighted_var, dim, skipna, keep_attrs))
_Weighted.std = lambda self, dim=None, *, skipna=None, keep_attrs=None: (
    self._apply(self._weighted_std, dim, skipna, keep_attrs))


class _GroupBy:

  def __init__(self, obj, group):
    assert group == 'time.dayofyear', group
    self.obj = obj
    self.labels = np.asarray(
        pd.DatetimeIndex(np.asarray(obj['time'].data)).dayofyear)

  def _reduce(self, statistic, **kwargs):
    groups = np.unique(self.labels)

    def one(da):
      if 'time' not in da.dims:
        return da
      axis = da.dims.index('time')
      pieces = [np.asarray(getattr(da.isel(time=np.nonzero(
          self.labels == g)[0]), statistic)('time', **kwargs).data)
                for g in groups]
      return _rebuilt(da, 'time', np.stack(pieces, axis=axis), groups,
                      'dayofyear')

    return _each(self.obj, one)

  def mean(self, **kwargs):
    return self._reduce('mean', **kwargs)

  def std(self, **kwargs):
    return self._reduce('std', **kwargs)


class _Resample:

  def __init__(self, obj, indexer=None, **kw):
    (self.dim, self.freq), = dict(indexer or {}, **kw).items()
    self.obj = obj

  def mean(self, **kwargs):
    index = pd.Index(np.asarray(self.obj[self.dim].data))
    positions = pd.Series(np.arange(len(index)), index=index)
    table = positions.resample(self.freq).agg(['min', 'max', 'count'])
    ranges = [(int(lo), int(hi) + 1) if n else None
              for lo, hi, n in zip(table['min'], table['max'], table['count'])]
    dim = self.dim

    def one(da):
      if dim not in da.dims:
        return da
      axis = da.dims.index(dim)
      rest = tuple(n for i, n in enumerate(da.shape) if i != axis)
      pieces = []
      for r in ranges:
        if r is None:
          pieces.append(np.full(rest, np.nan, dtype=da.dtype
                                if da.dtype.kind == 'f' else np.float64))
        else:
          pieces.append(np.asarray(
              da.isel({dim: slice(*r)}).mean(dim, **kwargs).data))
      return _rebuilt(da, dim, np.stack(pieces, axis=axis), table.index.values)

    return _each(self.obj, one)


def _pad(self, pad_width=None, mode='constant', **kw):
  assert mode == 'wrap', mode
  (dim, width), = dict(pad_width or {}, **kw).items()
  width = (width, width) if np.ndim(width) == 0 else tuple(width)

  def one(da):
    if dim not in da.dims:
      return da
    axis = da.dims.index(dim)
    pads = [(0, 0)] * da.ndim
    pads[axis] = width
    if sum(width) == 0:
      return da
    return _rebuilt(da, dim, np.pad(np.asarray(da.data), pads, mode='wrap'),
                    np.pad(np.asarray(da[dim].data), width, mode='wrap'))

  return _each(self, one)


class _Rolling:

  def __init__(self, obj, dim=None, min_periods=None, center=False, **kw):
    (self.dim, self.window), = dict(dim or {}, **kw).items()
    assert center is True and min_periods is None
    self.obj = obj

  def construct(self, window_dim):
    dim, w = self.dim, int(self.window)
    assert w % 2 == 1

    def one(da):
      if dim not in da.dims:
        return da
      axis = da.dims.index(dim)
      data = np.asarray(da.data)
      if data.dtype.kind != 'f':
        data = data.astype(np.float64)
      pads = [(0, 0)] * data.ndim
      pads[axis] = (w // 2, w // 2)
      padded = np.pad(data, pads, mode='constant', constant_values=np.nan)
      windows = np.lib.stride_tricks.sliding_window_view(padded, w, axis=axis)
      coords = {k: (tuple(c.dims), np.asarray(c.data))
                for k, c in da.coords.items()}
      return xr.DataArray(windows, coords=coords,
                          dims=tuple(da.dims) + (window_dim,), name=da.name)

    return _each(self.obj, one)


for _cls in (xr.DataArray, xr.Dataset):
  _cls.groupby = lambda self, group, **k: _GroupBy(self, group)
  _cls.resample = lambda self, *a, **k: _Resample(self, *a, **k)
  _cls.rolling = lambda self, *a, **k: _Rolling(self, *a, **k)
  _cls.pad = _pad
# (the stand-in rolls a DataArray with np.roll; a Dataset variable by variable)
xr.Dataset.roll = lambda self, shifts=None, **kw: _each(
    self, lambda da: da.roll(shifts, **kw))


def _load(name, path):
  spec = importlib.util.spec_from_file_location(name, path)
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  assert module.__file__.startswith(REFERENCE)
  return module


from weatherbench2 import utils  # noqa: E402  (the reference's)

assert utils.__file__.startswith(REFERENCE)
script = _load('wb2_reference_compute_climatology',
               os.path.join(REFERENCE, 'scripts', 'compute_climatology.py'))

from tests import climatology_cases as cc  # noqa: E402


class _Key:
  """As much of xarray_beam.Key as `compute_stat_chunk` uses."""

  def __init__(self, offsets, vars=None):  # pylint: disable=redefined-builtin
    self.offsets, self.vars = dict(offsets), vars

  def with_offsets(self, **offsets):
    new = dict(self.offsets)
    for k, v in offsets.items():
      if v is None:
        new.pop(k, None)
      else:
        new[k] = v
    return _Key(new, self.vars)

  def replace(self, vars=None):  # pylint: disable=redefined-builtin
    return _Key(self.offsets, vars)


def to_dataset(case):
  return xr.Dataset({'x': (case['dims'], case['data'])},
                    {'time': case['times']})


def run(case, method: str, stat: str):
  script.METHOD.value = method
  ds = to_dataset(case)
  kwargs = dict(window_size=case['window_size'],
                clim_years=case['clim_years'])
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')
    key, res = script.compute_stat_chunk(
        _Key({d: 0 for d in case['dims']}, {'x'}), ds,
        frequency=case['frequency'], statistic=stat,
        hour_interval=case['hour_interval'], **kwargs)
    assert 'time' not in key.offsets and key.offsets['dayofyear'] == 0
    name = 'x' if stat == 'mean' else f'x_{stat}'
    assert key.vars == {name} and list(res.data_vars) == [name]
    if case['frequency'] == 'hourly':
      fn = (utils.compute_hourly_stat if method == 'explicit'
            else utils.compute_hourly_stat_fast)
      direct = fn(ds, hour_interval=case['hour_interval'], stat_fn=stat,
                  **kwargs)
    else:
      fn = (utils.compute_daily_stat if method == 'explicit'
            else utils.compute_daily_stat_fast)
      direct = fn(ds, stat_fn=stat, **kwargs)
  np.testing.assert_array_equal(np.asarray(direct['x'].data),
                                np.asarray(res[name].data))
  return res[name]


def record(out, prefix, da):
  out[prefix] = np.asarray(da.data)
  out[prefix + '/dims'] = np.array(list(da.dims), dtype='U32')
  # (the explicit outputs come out of the stand-in's weighted reduction with
  # positions 0 .. n-1 for labels; only the labels of `fast` are recorded)
  if '/fast/' in prefix:
    out[prefix + '/dayofyear'] = np.asarray(da['dayofyear'].data)
  if 'hour' in da.dims:
    out[prefix + '/hour'] = np.asarray(da['hour'].data)


def known_case():
  """The input of utils_test.py:24-47 (testMethodEquivalence)."""
  from weatherbench2 import schema
  truth = schema.mock_truth_data(
      variables_3d=[], variables_2d=['2m_temperature'],
      time_start='2022-01-01', time_stop='2023-01-01')
  truth = truth + 1 * truth.time.dt.dayofyear
  da = truth['2m_temperature']
  case = cc._case(np.asarray(da['time'].data), np.asarray(da.data),  # pylint: disable=protected-access
                  tuple(da.dims), hour_interval=24, window_size=61)
  return case


def generate() -> dict:
  out = {}
  cases = {k: c for k, c in cc.expanded_cases().items() if c['reference']}
  cases['known'] = known_case()
  out['known/times'] = cases['known']['times']
  out['known/data'] = cases['known']['data']
  out['known/dims'] = np.array(list(cases['known']['dims']), dtype='U32')
  for cname, case in cases.items():
    for method in cc.METHODS:
      for stat in cc.STATS:
        record(out, f'{cname}/{method}/{stat}', run(case, method, stat))
  # what testMethodEquivalence asserts (xr.testing.assert_allclose: rtol 1e-5)
  np.testing.assert_allclose(out['known/explicit/mean'],
                             out['known/fast/mean'], rtol=1e-5)
  # the reference's errors
  case = cc.common_years()
  for bad in ('median',):
    try:
      script.compute_stat_chunk(_Key({}, {'x'}), to_dataset(case),
                                frequency='hourly', window_size=3,
                                clim_years=slice(None, None), statistic=bad,
                                hour_interval=24)
    except NotImplementedError as e:
      assert 'not implemented' in str(e)
    else:
      raise AssertionError(bad)
  try:
    script.compute_stat_chunk(_Key({}, {'x'}), to_dataset(case),
                              frequency='weekly', window_size=3,
                              clim_years=slice(None, None))
  except NotImplementedError as e:
    assert 'not implemented' in str(e)
  else:
    raise AssertionError('frequency')
  out['weights/61'] = np.asarray(utils.create_window_weights(61).data)
  out['weights/3'] = np.asarray(utils.create_window_weights(3).data)
  out['weights/7'] = np.asarray(utils.create_window_weights(7).data)
  return out


def main():
  out = generate()
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(cc.shard_of(key), {})[key] = value
  directory = os.environ.get('WB2_CLIMATOLOGY_OUT') or HERE
  for shard, arrays in by_shard.items():
    path = os.path.join(directory, f'{cc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')


if __name__ == '__main__':
  main()
