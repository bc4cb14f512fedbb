"""Writes tests/golden/reference_time_indexing_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified scripts/expand_climatology.py,
scripts/index_on_valid_time.py and
scripts/compute_probabilistic_climatological_forecasts.py on the seeded cases
of tests/time_indexing_cases.py, one shard per case and one for the sampler
(a committed file stays below 1 MiB; tests/time_indexing_cases.load_golden
reads them back as one dict).

The scripts read their options from absl flags and import apache_beam /
xarray_beam for their pipelines; absl.flags and absl.app do not exist here, so
this generator supplies, in its own process only, the same flag stand-in as
make_resample_vectors.py (DEFINE_* return plain holders with a `.value`, set
per case below; `flags.ValidationError` is an exception class of this file).
They run on the mini-xarray of oracle/refshim/ (xarray itself is absent here;
see make_derived_vectors.py).  What the stand-in lacks and this generator
supplies, in its own process only: a key class with `with_offsets` (installed
as `xarray_beam.Key`, so the scripts' isinstance checks hold),
`xarray_beam.split_chunks` and `split_variables` for chunks that are already
of the target size, and `xarray.zeros_like`.  Nothing under oracle/ changes.

What runs:
  * `_get_sampled_init_times`, `_get_ensemble_size`,
    `_check_input_spacing_and_time_flags` and `_check_times_in_dataset`: the
    live functions, under pandas;
  * the per-chunk functions `select_climatology`, `index_on_valid_time`,
    `slice_along_timedelta_axis_if_index_on_timedelta`, `iter_padding_chunks`
    and `_emit_sampled_weather`, and `get_forecast_offset_and_spacing`: the
    live functions on chunks this file cuts the way the pipelines do (one init
    time x one lead time per chunk; one truth time per chunk), their outputs
    written where their keys' offsets say.  Every cell of an output must be
    written exactly once.
What does not run: the three `main`s (zarr and Beam).  What they do around the
per-chunk functions -- the time axes, the templates' dims, the sampled times
per lead, the index information per destination -- is restated here from
their text, in `expand`, `index` and `ensemble` below; it is pinned by the
`known_*` cases, whose inputs and answers are those of the reference's own
tests (expand_climatology_test.py, index_on_valid_time_test.py,
compute_probabilistic_climatological_forecasts_test.py) and which this
generator asserts.  So the `<name>/dims` entries, the time axes and the lead
labels of the fixtures are this restatement, not reference output; only the
values and the offsets they are written at come from the reference's
functions.  The `index_grid_*` cases are NOT something `main` of
index_on_valid_time.py would run: their two variables have the init-time dim
on different axes, which its `get_axis` refuses (it unpacks a one-element
set); here every variable goes through the per-chunk functions on its own, as
`split_vars=True` sends it, with a template of its own.

Only runs where the reference is at hand:
    python tests/golden/make_time_indexing_vectors.py
`--live-sampler N SEED PATH` instead writes N random sampler draws (arguments
and the live function's answers) to PATH, for tests/test_time_indexing_cpu.py.
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
  """What a DEFINE_* of absl.flags returns, as far as the scripts read it."""

  def __init__(self, name, default):
    self.name, self.value = name, default


class ValidationError(Exception):
  """absl.flags.ValidationError."""


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
  flags.ValidationError = ValidationError
  flags.mark_flags_as_required = lambda names: None
  flags.mark_flag_as_required = lambda names: None
  return flags


import absl  # noqa: E402  (the import-only stand-in of oracle/refshim/)

absl.flags = sys.modules['absl.flags'] = _flags_module()
absl.app = sys.modules['absl.app'] = types.ModuleType('absl.app')

import xarray as xr  # noqa: E402  (the stand-in)
import xarray_beam  # noqa: E402  (the stand-in)

assert 'wb2shim' in xr.__version__


class _Key(xarray_beam.Key):
  """As much of xarray_beam.Key as the per-chunk functions use."""

  def with_offsets(self, **offsets):
    new = dict(self.offsets)
    for k, v in offsets.items():
      if v is None:
        new.pop(k, None)
      else:
        new[k] = v
    return _Key(new, self.vars)


def _split_chunks(key, dataset, target_chunks):
  for dim, n in target_chunks.items():
    assert dataset.sizes[dim] <= n, (dim, dataset.sizes[dim], n)
  yield key, dataset


def _split_variables(key, dataset):
  for name in dataset.data_vars:
    yield _Key(key.offsets, {name}), dataset[[name]]


def _zeros_like(dataset):
  return dataset.copy(data={k: np.zeros_like(np.asarray(v.data))
                            for k, v in dataset.data_vars.items()})


xarray_beam.Key = _Key
xarray_beam.split_chunks = _split_chunks
xarray_beam.split_variables = _split_variables
if not hasattr(xr, 'zeros_like'):
  xr.zeros_like = _zeros_like


def _load(name):
  spec = importlib.util.spec_from_file_location(
      'wb2_reference_' + name, os.path.join(REFERENCE, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  assert module.__file__.startswith(REFERENCE)
  return module


ref_expand = _load('expand_climatology')
ref_index = _load('index_on_valid_time')
ref_ens = _load('compute_probabilistic_climatological_forecasts')

from tests import time_indexing_cases as tc  # noqa: E402

DELTA = 'prediction_timedelta'


def to_dataset(case, names=None, rename=None):
  rename = rename or {}
  return xr.Dataset(
      {k: (tuple(rename.get(x, x) for x in d), a)
       for k, (d, a) in case['vars'].items() if names is None or k in names},
      {rename.get(k, k): v for k, v in case['coords'].items()})


class _Once:
  """An output array whose every cell must be written exactly once."""

  def __init__(self):
    self.data, self.count, self.dims = None, None, None

  def write(self, dims, shape, at: dict, block):
    block = np.asarray(block)
    if self.data is None:
      self.dims = tuple(dims)
      self.data = np.zeros(shape, dtype=block.dtype)
      self.count = np.zeros(shape, dtype=np.int32)
    assert tuple(dims) == self.dims, (dims, self.dims)
    assert block.dtype == self.data.dtype, (block.dtype, self.data.dtype)
    where = tuple(slice(at.get(d, 0), at.get(d, 0) + n)
                  for d, n in zip(dims, block.shape))
    self.data[where] = block
    self.count[where] += 1

  def result(self):
    assert self.count is not None and (self.count == 1).all(), (
        'cells written', np.unique(self.count))
    return self.data


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def sampled(kwargs: dict) -> np.ndarray:
  kwargs = dict(kwargs)
  times = pd.DatetimeIndex(kwargs.pop('output_times'))
  out = ref_ens._get_sampled_init_times(times, **kwargs)  # pylint: disable=protected-access
  assert out.dtype == np.dtype('datetime64[ns]'), out.dtype
  return out


# ---------------------------------------------------------------------------
# expand_climatology: `select_climatology` per variable and time chunk
# ---------------------------------------------------------------------------
def expand(case, chunk: int = 7) -> dict:
  climatology = to_dataset(case)
  times = pd.DatetimeIndex(case['times'])
  time_dims = ['hour', 'dayofyear'] if 'hour' in climatology.coords else [
      'dayofyear']
  out = {}
  for name, (dims, _) in case['vars'].items():
    if not any(d in dims for d in time_dims):
      continue
    pieces, first_dims = [], None
    for start in range(0, len(times), chunk):
      (key, sliced), = ref_expand.select_climatology(
          (name, slice(start, start + chunk)), climatology, times, {})
      assert key.offsets == {'time': start} and key.vars == {name}
      da = sliced[name]
      assert 'hour' not in sliced.coords and 'dayofyear' not in sliced.coords
      first_dims = first_dims or tuple(da.dims)
      assert tuple(da.dims) == first_dims
      np.testing.assert_array_equal(np.asarray(da['time'].data),
                                    times[start:start + chunk].values)
      pieces.append(np.asarray(da.data))
    out[name] = np.concatenate(pieces, axis=first_dims.index('time'))
    out[f'{name}/dims'] = np.array(first_dims, dtype='U32')
  out['time'] = times.values
  return out


# ---------------------------------------------------------------------------
# index_on_valid_time: one (init, lead) chunk at a time, then the padding
# ---------------------------------------------------------------------------
def index(case) -> dict:
  mode = case['mode']
  ref_index.DESIRED_TIME_DIMS.value = mode
  source = to_dataset(case, rename={'time': 'init'})
  by_delta = mode == ref_index.VALID_AND_DELTA
  other, dropped = (DELTA, 'init') if by_delta else ('init', DELTA)
  inits = np.asarray(source['init'].data)
  leads = np.asarray(source[DELTA].data)
  offset, spacing = ref_index.get_forecast_offset_and_spacing(inits, leads)
  new_deltas = leads[offset::spacing] if by_delta else leads
  new_times = np.unique(inits[:, None] + new_deltas[None, :])
  other_labels = new_deltas if by_delta else inits
  out = {}
  for name, (dims, array) in case['vars'].items():
    in_dims = tuple('init' if d == 'time' else d for d in dims)
    # the template's dims: valid time where the dropped dim stood
    out_dims = tuple('time' if d == dropped else d for d in in_dims)
    sizes = dict(zip(in_dims, array.shape))
    sizes.update({'time': len(new_times), other: len(other_labels)})
    shape = tuple(sizes[d] for d in out_dims)
    cells = _Once()
    one = source[[name]]
    for i in range(len(inits)):
      for j in range(len(leads)):
        key = _Key({d: 0 for d in in_dims}, {name}).with_offsets(
            **{'init': i, DELTA: j})
        chunk = one.isel({'init': [i], DELTA: [j]})
        for key2, chunk2 in (
            ref_index.slice_along_timedelta_axis_if_index_on_timedelta(
                key, chunk, forecast_offset=offset,
                forecast_spacing=spacing)):
          key3, new = ref_index.index_on_valid_time(
              key2, chunk2, dropped_dim=dropped, forecast_spacing=spacing)
          assert dropped not in key3.offsets
          da = new[name]
          # (the chunk's own dim order may differ from the template's: the
          # zarr writer goes by name)
          da = da.transpose(*out_dims)
          at = dict(key3.offsets)
          assert np.asarray(da['time'].data)[0] == new_times[at['time']]
          assert np.asarray(da[other].data)[0] == other_labels[at[other]]
          cells.write(out_dims, shape, at, da.data)
    template = xr.Dataset(
        {name: (out_dims, np.zeros(shape, dtype=np.float32))},
        {'time': new_times, other: other_labels})
    for key, chunk in ref_index.iter_padding_chunks(
        None, template, {'init': 1, DELTA: 1}, pd.Index(
            inits if by_delta else leads), other_index_dim=other,
        dropped_dim=dropped):
      da = chunk[name].transpose(*out_dims)
      assert np.isnan(np.asarray(da.data)).all()
      cells.write(out_dims, shape, dict(key.offsets), da.data)
    out[name] = cells.result()
    assert out[name].dtype == np.float32
    out[f'{name}/dims'] = np.array(out_dims, dtype='U32')
  out['time'] = new_times
  out['other'] = other_labels
  out['offset_and_spacing'] = np.array([offset, spacing])
  return out


# ---------------------------------------------------------------------------
# the sampled ensemble: `_emit_sampled_weather` per truth time
# ---------------------------------------------------------------------------
def ensemble(case) -> dict:
  kw = dict(case['kwargs'])
  time_dim = kw.get('time_dim', 'time')
  realization = kw.get('realization_name', 'realization')
  ref_ens.TIME_DIM.value = time_dim
  ref_ens.REALIZATION_NAME.value = realization
  ref_ens.ADD_SOURCE_TIME.value = bool(kw.get('add_source_time', False))
  ref_ens.TIMEDELTA_SPACING.value = kw['timedelta_spacing']
  ref_ens.INITIAL_TIME_SPACING.value = kw['initial_time_spacing']
  ref_ens.INITIAL_TIME_EDGE_BEHAVIOR.value = kw.get(
      'initial_time_edge_behavior', 'WRAP_YEAR')
  ref_ens.SAMPLE_HOLD_DAYS.value = kw.get('sample_hold_days', 0)
  truth = to_dataset(case)
  ref_ens._check_input_spacing_and_time_flags(truth)  # pylint: disable=protected-access
  leave_out = kw.get('leave_out_if_in_climatology', False)
  n_member = ref_ens._get_ensemble_size(  # pylint: disable=protected-access
      kw['ensemble_size'], kw['climatology_start_year'],
      kw['climatology_end_year'], kw['day_window_size'], leave_out)
  inits = pd.date_range(kw['initial_time_start'], kw['initial_time_end'],
                        freq=kw['initial_time_spacing'])
  deltas = pd.timedelta_range('0 days', kw['forecast_duration'],
                              freq=kw['timedelta_spacing'])
  sampled_times = ref_ens._get_sampled_init_times(  # pylint: disable=protected-access
      output_times=inits,
      climatology_start_year=kw['climatology_start_year'],
      climatology_end_year=kw['climatology_end_year'],
      day_window_size=kw['day_window_size'], ensemble_size=n_member,
      with_replacement=kw.get('with_replacement', True),
      initial_time_edge_behavior=kw.get('initial_time_edge_behavior',
                                        'WRAP_YEAR'),
      sample_hold_days=kw.get('sample_hold_days', 0),
      leave_out_if_in_climatology=leave_out,
      num_years_to_exclude=kw.get('num_years_to_exclude', 0),
      seed=kw['seed'])
  assert sampled_times.shape == (n_member, len(inits))
  flat = sampled_times.ravel()  # [realization][init]
  needed = np.unique(np.stack([flat + td.to_numpy() for td in deltas]))
  ref_ens._check_times_in_dataset(needed, truth)  # pylint: disable=protected-access
  # the index information of every destination, keyed by its truth time
  by_time: dict = {}
  for d, td in enumerate(deltas):
    for r in range(n_member):
      for i in range(len(inits)):
        source = sampled_times[r, i] + td.to_numpy()
        by_time.setdefault(source, []).append({
            'timedelta_value': td, time_dim: i, realization: r, DELTA: d,
            'output_init_time_value': inits.values[i],
            'sampled_time_value': source})
  truth_times = np.asarray(truth[time_dim].data)
  position = {t: k for k, t in enumerate(truth_times)}
  cells: dict = {}
  for source in needed:
    k = position[source]
    chunk = truth.isel({time_dim: [k]})
    key = _Key({time_dim: k})
    for new_key, new in ref_ens._emit_sampled_weather(  # pylint: disable=protected-access
        0, {'dataset_in_chunks': [(key, chunk)],
            'time_key_and_index_info': by_time[source]}):
      for name in new.data_vars:
        da = new[name]
        assert tuple(da.dims)[:2] == (realization, DELTA), da.dims
        # the template's dims (`main`: the time dim dropped, then time, lead
        # and realization put in front); a chunk keeps its time dim where the
        # truth has it, and the zarr writer goes by name
        dims = (realization, DELTA, time_dim) + tuple(
            x for x in da.dims if x not in (realization, DELTA, time_dim))
        da = da.transpose(*dims)
        sizes = dict(zip(dims, da.shape))
        sizes.update({realization: n_member, DELTA: len(deltas),
                      time_dim: len(inits)})
        cells.setdefault(name, _Once()).write(
            dims, tuple(sizes[x] for x in dims), dict(new_key.offsets),
            da.data)
  out = {}
  for name, once in cells.items():
    out[name] = once.result()
    out[f'{name}/dims'] = np.array(once.dims, dtype='U32')
  out['time'] = inits.values
  out[DELTA] = deltas.values
  out['sampled'] = sampled_times
  return out


# ---------------------------------------------------------------------------
# what the reference's own tests assert
# ---------------------------------------------------------------------------
def check_known(out: dict):
  for name, answer in tc.KNOWN_INDEX_ANSWERS.items():
    np.testing.assert_array_equal(out[f'index/{name}/foo'],
                                  np.array(answer, dtype=np.float32))
  nan = np.nan
  np.testing.assert_array_equal(
      out['index/known_index_zero_init/foo'],
      np.array([[1, 2, 3, 4, 5, nan, nan, nan, nan, nan, nan],
                [nan, nan, 6, 7, 8, 9, 10, nan, nan, nan, nan],
                [nan, nan, nan, nan, 11, 12, 13, 14, 15, nan, nan],
                [nan, nan, nan, nan, nan, nan, 16, 17, 18, 19, 20]],
               dtype=np.float32))
  assert out['index/known_index_offset_init/foo'].shape == (4, 10)
  for name in tc.KNOWN_ENSEMBLE:
    case = tc.ensemble_cases()[f'known_ens_{name}']()
    prefix = f'ensemble/known_ens_{name}/'
    temperature = out[prefix + 'temperature']
    dims = out[prefix + 'temperature/dims'].tolist()
    axis = dims.index(DELTA)
    np.testing.assert_allclose(np.diff(temperature, axis=axis), 1)
    assert (temperature.var(axis=dims.index('realization')) > 0).all()
    if case['kwargs'].get('add_source_time'):
      source = out[prefix + 'source_time']
      step = np.diff(out[prefix + DELTA])[0]
      assert (np.diff(source, axis=axis) == step).all()
  years = out['sampler/known_leave_out_1/sampled'].astype(
      'datetime64[Y]').astype(int) + 1970
  assert 2005 not in years and 2006 not in years
  assert set(np.unique(years)) <= set(range(2000, 2005)) | set(range(2007,
                                                                     2011))
  years = out['sampler/known_leave_out_0/sampled'].astype(
      'datetime64[Y]').astype(int) + 1970
  assert 2005 not in years and 2006 in years


def generate() -> dict:
  out = {}
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    for name, build in tc.sampler_cases().items():
      out[f'sampler/{name}/sampled'] = sampled(build())
    for family, cases, run in (('expand', tc.expand_cases(), expand),
                               ('index', tc.index_cases(), index),
                               ('ensemble', tc.ensemble_cases(), ensemble)):
      for name, build in cases.items():
        for key, value in run(build()).items():
          out[f'{family}/{name}/{key}'] = value
  check_known(out)
  return out


def live_sampler(n: int, seed: int, path: str) -> None:
  """N random draws of the sampler's arguments with the live answers."""
  rng = np.random.default_rng(seed)
  out = {}
  edges = (ref_ens.WRAP_YEAR, ref_ens.NO_EDGE, ref_ens.REFLECT_RANGE)
  k = 0
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    while k < n:
      start = np.datetime64('2015-01-01T00', 'ns') + int(
          rng.integers(0, 9000)) * tc.HOUR * 6
      step = int(rng.choice([6, 12, 24, 48]))
      times = tc.time_axis(str(start), step, int(rng.integers(1, 14)))
      first = int(rng.integers(2008, 2018))
      kwargs = dict(
          climatology_start_year=first,
          climatology_end_year=first + int(rng.integers(0, 12)),
          day_window_size=int(rng.choice([1, 2, 5, 10, 15, 400])),
          ensemble_size=int(rng.choice([-1, 1, 3, 7])),
          with_replacement=bool(rng.integers(2)),
          sample_hold_days=int(rng.choice([0, 0, 2, 4])),
          initial_time_edge_behavior=str(rng.choice(edges)),
          leave_out_if_in_climatology=bool(rng.integers(2)),
          num_years_to_exclude=int(rng.integers(0, 3)),
          seed=int(rng.integers(0, 10**6)))
      try:
        answer = sampled(dict(kwargs, output_times=times))
      except (ValueError, ValidationError, KeyError):
        # (an error case; KeyError: a sample hold with one output time)
        answer = np.zeros((0, 0), dtype='datetime64[ns]')
      out[f'{k}/times'] = times
      out[f'{k}/answer'] = answer
      for name, value in kwargs.items():
        out[f'{k}/kw/{name}'] = np.array(value)
      k += 1
  np.savez(path, **out)


def shards(out: dict) -> dict:
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(tc.shard_of(key), {})[key] = value
  return by_shard


def main():
  if len(sys.argv) > 1 and sys.argv[1] == '--live-sampler':
    live_sampler(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    return
  out = generate()
  directory = os.environ.get('WB2_TIME_INDEXING_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{tc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')


if __name__ == '__main__':
  main()
