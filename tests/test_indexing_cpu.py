"""weatherbench2_amd/indexing.py against pandas and against loops written out
by hand: the calendar, label positions and the slab table of a vectorised
selection, and the two entry points that build the same table from it."""
import datetime
import itertools

import numpy as np
import pandas as pd
import pytest

from weatherbench2_amd import evaluation
from weatherbench2_amd import indexing
from weatherbench2_amd import time_indexing as ti
from weatherbench2_amd import xarray_lite as xl

STAMPS = ('1969-12-31T23:00', '1900-03-01T07', '2020-02-29T05:30',
          '2020-12-31T05', '2024-12-31T23:59:59')


# ---------------------------------------------------------------------------
# calendar
# ---------------------------------------------------------------------------
def _check_calendar(times, stamps_ns):
  year, doy, hour, day = indexing.calendar(times)
  idx = pd.DatetimeIndex(np.asarray(stamps_ns).ravel())
  shape = np.shape(times)
  for got, want in ((year, idx.year), (doy, idx.dayofyear), (hour, idx.hour),
                    (day, np.asarray(stamps_ns).ravel().astype(
                        'datetime64[D]').astype(np.int64))):
    assert got.dtype == np.int64 and got.shape == shape
    np.testing.assert_array_equal(got.ravel(), np.asarray(want))


@pytest.mark.parametrize('unit', ['s', 'h', 'ns'])
def test_calendar_equals_pandas_in_every_unit_and_shape(unit):
  # (a coarser unit truncates the stamp: pandas sees the truncated one too)
  flat = np.array(STAMPS, dtype='datetime64[ns]').astype(f'datetime64[{unit}]')
  _check_calendar(flat, flat.astype('datetime64[ns]'))
  lead = np.array([0, 30], dtype='timedelta64[h]')
  grid = flat[:, None] + lead[None, :]  # (init, lead)
  assert grid.shape == (5, 2)
  _check_calendar(grid, grid.astype('datetime64[ns]'))


@pytest.mark.parametrize('make', [
    lambda s: pd.Timestamp(s).to_pydatetime(), pd.Timestamp],
                         ids=['datetime', 'Timestamp'])
def test_calendar_of_object_arrays(make):
  ns = np.array(STAMPS, dtype='datetime64[ns]')
  objects = np.empty(len(STAMPS), dtype=object)
  for i, s in enumerate(STAMPS):
    objects[i] = make(s)
  assert isinstance(objects[0], datetime.datetime)
  _check_calendar(objects, ns)
  _check_calendar(objects.reshape(5, 1), ns.reshape(5, 1))
  _check_calendar(np.array(STAMPS), ns)  # ISO strings


def test_calendar_nat_and_integers():
  with pytest.raises(ValueError, match='NaT'):
    indexing.calendar(np.array(['2020-01-01', 'NaT'], dtype='datetime64[D]'))
  with pytest.raises(ValueError, match='NaT'):
    indexing.calendar(np.array([['2020-01-01T00', 'NaT']],
                               dtype='datetime64[ns]'))
  # integers have a meaning under the conversion (and under DatetimeIndex,
  # which the callers used before): nanoseconds since 1970.  Kept.
  ints = np.array([-1, 0, 86400 * 10**9 * 366 + 3600 * 10**9])
  _check_calendar(ints, ints.astype('datetime64[ns]'))
  assert [a.tolist() for a in indexing.calendar(ints)] == [
      [1969, 1970, 1971], [365, 1, 2], [23, 0, 1], [-1, 0, 366]]


# ---------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------
def _ns(a):
  a = np.asarray(a)
  if a.dtype.kind in 'Mm':
    unit = 'datetime64[ns]' if a.dtype.kind == 'M' else 'timedelta64[ns]'
    return a.astype(unit).astype(np.int64)
  return a


def _brute(have, want):
  """The double loop; the FIRST match wins."""
  have, want = _ns(have), _ns(want)
  out = np.full(want.shape, -1, dtype=np.int64)
  flat = out.reshape(-1)
  for j, w in enumerate(want.reshape(-1).tolist()):
    for i, h in enumerate(have.tolist()):
      if h == w:
        flat[j] = i
        break
  return out


def _check_positions(have, want):
  got = indexing.positions(have, want)
  assert got.dtype == np.int64 and got.shape == np.shape(want)
  np.testing.assert_array_equal(got, _brute(have, want))
  return got


def test_positions_of_small_integer_labels_take_the_table_and_its_memo():
  rs = np.random.RandomState(0)
  for have in (rs.permutation(np.arange(1, 367)), np.arange(24),
               rs.permutation(np.arange(0, 24, 6)).astype(np.int32)):
    want = rs.choice(have, size=(3, 5))
    indexing._LABEL_LUTS.clear()
    first = _check_positions(have, want)
    assert indexing._LABEL_LUTS[id(have)][0] is have
    table = indexing._LABEL_LUTS[id(have)][1]
    assert table is not None
    again = _check_positions(have, want)  # (the memo is hit)
    assert indexing._LABEL_LUTS[id(have)][1] is table
    np.testing.assert_array_equal(first, again)
    _check_positions(have, np.array([-5, -1, 0, 24, 366, 367, 4096, 10**6]))
    _check_positions(have, np.array([0, 6, 255], dtype=np.uint8))


def test_the_memo_is_bounded_and_skips_what_has_no_table():
  indexing._LABEL_LUTS.clear()
  keep = [np.arange(3) + i for i in range(70)]
  for have in keep:
    _check_positions(have, np.array([2, 3, 99]))
  assert 0 < len(indexing._LABEL_LUTS) <= 64
  indexing._LABEL_LUTS.clear()
  _check_positions(np.array([3, 1, 10**9]), np.array([1, 2, 10**9]))
  _check_positions(np.array([3, -1, 7]), np.array([-1, 7, 0]))
  _check_positions(np.arange(5000), np.array([4999, 5000]))  # (too long)
  assert all(lut is None for _, lut in indexing._LABEL_LUTS.values())


def test_positions_of_floats_times_and_strings():
  _check_positions(np.array([850.0, 500.0, 1000.0, 50.0]),
                   np.array([[500.0, 50.0], [1000.0, 700.0]]))
  _check_positions(np.array([850, 500, 1000]), np.array([500.0, 850.5]))
  have = (np.datetime64('1969-12-31T18', 'h')
          + np.array([6, 0, 12, 30]).astype('timedelta64[h]'))
  want = (np.datetime64('1969-12-31T18', 'ns')
          + np.array([[0, 6], [30, 7]]).astype('timedelta64[h]'))
  assert have.dtype != want.dtype
  np.testing.assert_array_equal(_check_positions(have, want),
                                [[1, 0], [3, -1]])
  np.testing.assert_array_equal(
      _check_positions(np.array([0, 21600, 43200], dtype='timedelta64[s]'),
                       np.array([12, 6, 1], dtype='timedelta64[h]')),
      [2, 1, -1])
  np.testing.assert_array_equal(
      _check_positions(np.array(['tropics', 'global', 'europe']),
                       np.array([['global', 'asia'], ['europe', 'tropics']])),
      [[1, -1], [2, 0]])


def test_positions_of_empty_sides():
  for have, want in ((np.zeros(0, np.int64), np.array([[1, 2]])),
                     (np.zeros(0), np.array([1.0])),
                     (np.zeros(0, 'datetime64[ns]'),
                      np.array(['2020-01-01'], dtype='datetime64[D]')),
                     (np.zeros(0, '<U3'), np.array(['a', 'b']))):
    np.testing.assert_array_equal(_check_positions(have, want),
                                  np.full(want.shape, -1))
  for have in (np.arange(4), np.array([1.5, 2.5]), np.array(['a']),
               np.array(['2020-01-01'], dtype='datetime64[D]')):
    assert _check_positions(have, have[:0]).shape == (0,)
    assert _check_positions(have, have[:0].reshape(0, 3)).shape == (0, 3)


def test_absent_labels_are_minus_one_and_a_keyerror_of_the_wrapper():
  have = np.array([1, 2, 3, 365])
  want = np.array([[1, 366], [365, 2]])
  np.testing.assert_array_equal(indexing.positions(have, want),
                                [[0, -1], [3, 1]])
  with pytest.raises(KeyError, match='dayofyear label .*366.* not found'):
    indexing.sel_positions(have, want, 'dayofyear label {label!r} not found')
  np.testing.assert_array_equal(
      indexing.sel_positions(have, want[:, :1], '{label}'), [[0], [3]])
  with pytest.raises(KeyError, match='level 700.0'):
    indexing.sel_positions(np.array([500.0, 850.0]), np.array([850.0, 700.0]),
                           'level {label}')
  with pytest.raises(KeyError, match='asia'):
    indexing.sel_positions(np.array(['global']), np.array(['asia']), '{label}')


def test_a_duplicated_label_gives_its_first_position():
  """Outside the reference's contract (pandas raises on a non-unique index);
  pinned so that every kind of label answers alike."""
  for have, want in (
      (np.array([7, 3, 7, 3, 1]), np.array([3, 7, 1, 2])),    # (no table)
      (np.array([0.5, 0.25, 0.5]), np.array([0.5, 0.25])),
      (np.array(['2020-01-02', '2020-01-01', '2020-01-02'],
                dtype='datetime64[D]'),
       np.array(['2020-01-02T00'], dtype='datetime64[ns]')),
      (np.array(['a', 'b', 'a', 'b']), np.array(['b', 'a', 'c']))):
    _check_positions(have, want)
  np.testing.assert_array_equal(
      indexing.positions(np.array([7, 3, 7, 3, 1]), np.array([3, 7, 1, 2])),
      [1, 0, 4, -1])
  np.testing.assert_array_equal(
      indexing.positions(np.array(['a', 'b', 'a', 'b']), np.array(['b', 'a'])),
      [1, 0])


# ---------------------------------------------------------------------------
# the slab table
# ---------------------------------------------------------------------------
def _slab_table_by_hand(in_dims, sizes, out_dims, re_, n_inner):
  in_outer = in_dims[:len(in_dims) - n_inner]
  out_outer = out_dims[:len(out_dims) - n_inner]
  new_sizes = dict(zip(re_.new_dims, re_.table.shape))
  shape = [new_sizes[d] if d in new_sizes else sizes[d] for d in out_outer]
  out = np.zeros(shape, dtype=np.int64)
  for at in itertools.product(*[range(n) for n in shape]):
    here = dict(zip(out_outer, at))
    entry = int(re_.table[tuple(here[d] for d in re_.new_dims)])
    if entry < 0:
      out[at] = -1
      continue
    where = {}
    for d in reversed(re_.src_dims):  # C order over the grid of src_dims
      entry, where[d] = divmod(entry, sizes[d])
    slab = 0
    for d in in_outer:
      slab = slab * sizes[d] + (where[d] if d in where else here[d])
    out[at] = slab
  return out


def _check_slab_table(in_dims, sizes, re_, n_inner=2):
  out_dims = indexing.in_place_dims(in_dims, re_.src_dims, re_.new_dims)
  got = indexing.slab_table(in_dims, sizes, out_dims, re_, n_inner)
  want = _slab_table_by_hand(in_dims, sizes, out_dims, re_, n_inner)
  assert got.dtype == np.int64 and got.shape == want.shape
  np.testing.assert_array_equal(got, want)
  return out_dims, got


SIZES = {'time': 4, 'level': 2, 'hour': 3, 'dayofyear': 4, 'number': 2,
         'latitude': 2, 'longitude': 3}


def test_one_dim_becomes_two_the_persistence_shape():
  table = np.array([[0, 1, 3], [1, -1, 3]])  # (lead, init) -> time
  re_ = indexing.Reindex(('time',), ('lead', 'init'), table)
  dims, got = _check_slab_table(
      ('number', 'time', 'level', 'latitude', 'longitude'), SIZES, re_)
  assert dims == ('number', 'lead', 'init', 'level', 'latitude', 'longitude')
  assert got.shape == (2, 2, 3, 2)
  assert got[1, 0, 2, 1] == (1 * 4 + 3) * 2 + 1 and (got[:, 1, 1] == -1).all()
  # the new dims given in another order than they stand in the output
  swapped = indexing.Reindex(('time',), ('init', 'lead'), table.T)
  out_dims = ('lead', 'init', 'level', 'latitude', 'longitude')
  in_dims = ('time', 'level', 'latitude', 'longitude')
  np.testing.assert_array_equal(
      indexing.slab_table(in_dims, SIZES, out_dims, swapped, 2),
      _slab_table_by_hand(in_dims, SIZES, out_dims, swapped, 2))
  np.testing.assert_array_equal(
      indexing.slab_table(in_dims, SIZES, out_dims, swapped, 2),
      indexing.slab_table(in_dims, SIZES, out_dims,
                          indexing.Reindex(('time',), ('lead', 'init'), table),
                          2))


def test_two_dims_become_one_adjacent_or_not():
  hour, doy = np.array([0, 2, 1, 2, 0]), np.array([3, 0, 0, 2, 1])
  table = np.ravel_multi_index([hour, doy], (3, 4))
  table[2] = -1
  re_ = indexing.Reindex(('hour', 'dayofyear'), ('time',), table)
  dims, got = _check_slab_table(
      ('hour', 'dayofyear', 'latitude', 'longitude'), SIZES, re_)
  assert dims == ('time', 'latitude', 'longitude') and got.shape == (5,)
  dims, got = _check_slab_table(
      ('hour', 'level', 'dayofyear', 'latitude', 'longitude'), SIZES, re_)
  assert dims == ('time', 'level', 'latitude', 'longitude')
  assert got[3, 1] == (2 * 2 + 1) * 4 + 2
  dims, _ = _check_slab_table(
      ('number', 'dayofyear', 'level', 'hour', 'latitude', 'longitude'), SIZES,
      indexing.Reindex(('dayofyear', 'hour'), ('time',),
                       np.ravel_multi_index([doy, hour], (4, 3))))
  assert dims == ('number', 'time', 'level', 'latitude', 'longitude')
  # a slab of another depth: everything behind the selection, or one dim
  for n_inner in (0, 1, 3):
    _check_slab_table(('hour', 'level', 'dayofyear', 'number', 'latitude',
                       'longitude')[:3 + n_inner], SIZES, re_, n_inner)


def test_an_empty_table():
  re_ = indexing.Reindex(('hour', 'dayofyear'), ('time',),
                         np.zeros(0, np.int64))
  _, got = _check_slab_table(
      ('hour', 'level', 'dayofyear', 'latitude', 'longitude'), SIZES, re_)
  assert got.shape == (0, 2)
  re_ = indexing.Reindex(('time',), ('lead', 'init'), np.zeros((3, 0), np.int64))
  _, got = _check_slab_table(('time', 'level', 'latitude', 'longitude'), SIZES,
                             re_)
  assert got.shape == (3, 0, 2)


def test_common_tail_and_compose():
  re_ = indexing.Reindex(('time',), ('lead', 'init'), np.zeros((1, 1), int))
  tail = indexing.common_tail
  assert tail(('time', 'level', 'latitude', 'longitude'),
              ('lead', 'init', 'level', 'latitude', 'longitude'), re_) == 3
  assert tail(('level', 'time', 'latitude', 'longitude'),
              ('level', 'lead', 'init', 'latitude', 'longitude'), re_) == 2
  assert tail(('latitude', 'longitude', 'time'),
              ('latitude', 'longitude', 'lead', 'init'), re_) == 0
  same = indexing.Reindex(('time',), ('time',), np.zeros(1, int))
  assert tail(('level', 'time'), ('level', 'time'), same) == 0
  prior = np.array([5, -1, 2, 0])
  table = np.array([[3, 1], [-1, 2]])
  got = indexing.compose(table, prior)
  np.testing.assert_array_equal(got, [[0, -1], [-1, 2]])
  for at in itertools.product(range(2), range(2)):
    assert got[at] == (-1 if table[at] < 0 else prior[table[at]])


def _source(dims, with_gather=False):
  shape = tuple(SIZES[d] for d in dims)
  values = np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
  data, prior = values, None
  if with_gather:  # the same array, read through an earlier gather with a hole
    n_outer = int(np.prod(shape[:-2]))
    prior = np.random.RandomState(1).permutation(n_outer)
    base = np.zeros((n_outer,) + shape[-2:])
    base[prior] = values.reshape((n_outer,) + shape[-2:])
    prior[5] = -1
    data = xl.SlabGather(base, prior.reshape(shape[:-2]))
    values = values.copy()
    values.reshape((n_outer,) + shape[-2:])[5] = np.nan
  coords = {d: np.arange(SIZES[d]) for d in dims}
  return xl.Dataset({'x': xl.DataArray(data, dims)}, coords), values, prior


@pytest.mark.parametrize('with_gather', [False, True])
def test_gather_dataset_a_hole_in_one_selector_and_an_earlier_gather(
    with_gather):
  """evaluation._gather_dataset builds its table from the shared planner: two
  selectors over dims that are not adjacent, a hole in one of them only, and
  the composition over an index that has a hole of its own."""
  dims = ('hour', 'level', 'dayofyear', 'latitude', 'longitude')
  source, values, prior = _source(dims, with_gather)
  hour, doy = np.array([0, 2, -1, 2, 0]), np.array([3, 0, 0, 2, 1])
  out = evaluation._gather_dataset(
      source, ['x'], {'dayofyear': doy, 'hour': hour}, ('time',), (5,),
      {'time': np.arange(5)})
  assert out['x'].dims == ('time', 'level', 'latitude', 'longitude')
  index = out['x'].data.index
  assert index.shape == (5, 2)
  want = np.full((5, 2, 2, 3), np.nan)
  for i, lev in itertools.product(range(5), range(2)):
    slab = -1 if hour[i] < 0 else (hour[i] * 2 + lev) * 4 + doy[i]
    if slab >= 0:
      want[i, lev] = values[hour[i], lev, doy[i]]
      if prior is not None:
        slab = prior[slab]
    assert index[i, lev] == slab
  assert (index[2] == -1).all()
  if with_gather:
    assert (index == -1).sum() == 3  # (the two of the selector, one of prior)
  np.testing.assert_array_equal(np.asarray(out['x'].values), want)


def test_gather_dataset_one_dim_becomes_two():
  source, values, _ = _source(('number', 'time', 'latitude', 'longitude'))
  where = np.array([[0, 1, 3], [1, -1, 3]])
  out = evaluation._gather_dataset(
      source, ['x'], {'time': where}, ('lead', 'init'), where.shape,
      {'lead': np.arange(2), 'init': np.arange(3)})
  assert out['x'].dims == ('number', 'lead', 'init', 'latitude', 'longitude')
  want = values[:, np.maximum(where, 0)]
  want[:, where < 0] = np.nan
  np.testing.assert_array_equal(np.asarray(out['x'].values), want)


# ---------------------------------------------------------------------------
# expand_climatology(materialize=False) and climatology_like_forecast
# ---------------------------------------------------------------------------
def _climatology(n_doy=366):
  rs = np.random.RandomState(3)
  dims = ('hour', 'dayofyear', 'latitude', 'longitude')
  return xl.Dataset(
      {k: xl.DataArray(rs.normal(size=(2, n_doy, 2, 3)).astype(np.float32),
                       dims) for k in ('z', 't2m')},
      {'hour': np.array([0, 12]), 'dayofyear': np.arange(1, n_doy + 1),
       'latitude': np.array([-45.0, 45.0]),
       'longitude': np.array([0.0, 120.0, 240.0])})


def _forecast(times):
  return xl.Dataset(
      {k: xl.DataArray(np.zeros((len(times), 2, 3), np.float32),
                       ('time', 'latitude', 'longitude')) for k in ('z', 't2m')},
      {'time': times, 'latitude': np.array([-45.0, 45.0]),
       'longitude': np.array([0.0, 120.0, 240.0])})


def test_the_two_climatology_entry_points_build_one_table():
  times = (np.datetime64('2020-12-30T00', 'ns')
           + np.arange(8) * np.timedelta64(12, 'h'))
  doy = indexing.calendar(times)[1]
  assert 366 in doy and 1 in doy and times[-1] == np.datetime64('2021-01-02T12')
  clim = _climatology()
  lazy = ti.expand_climatology(clim, times, materialize=False)
  like = evaluation.climatology_like_forecast(_forecast(times), clim, 'time')
  hour = np.arange(8) % 2
  for name in ('z', 't2m'):
    a, b = lazy[name].data, like[name].data
    assert isinstance(a, xl.SlabGather) and isinstance(b, xl.SlabGather)
    assert lazy[name].dims == like[name].dims == (
        'time', 'latitude', 'longitude')
    np.testing.assert_array_equal(a.index, b.index)
    np.testing.assert_array_equal(a.index, hour * 366 + doy - 1)
    np.testing.assert_array_equal(np.asarray(lazy[name].values),
                                  np.asarray(like[name].values))
  short = _climatology(365)
  with pytest.raises(KeyError, match='dayofyear'):
    ti.expand_climatology(short, times, materialize=False)
  with pytest.raises(KeyError, match='dayofyear'):
    evaluation.climatology_like_forecast(_forecast(times), short, 'time')
