"""The pure parts of the operand layer (weatherbench2_amd/operands.py and the
two coordinate helpers of xarray_lite): no GPU."""
import numpy as np
import pytest
import torch

from weatherbench2_amd import operands
from weatherbench2_amd import xarray_lite as xl

SIZES = {'m': 2, 's': 23, 'a': 3, 'b': 8}

# (dims, reduced) -> (order, first, shape, n_outer, n_series, n_point,
#                     n_inner_dims, copied)
TABLE = {
    'first': (('s', 'm', 'a', 'b'), 's',
              (('s', 'm', 'a', 'b'), 0, (23, 2, 3, 8), 1, 23, 48, 3, False)),
    'middle': (('m', 's', 'a', 'b'), 's',
               (('m', 's', 'a', 'b'), 1, (2, 23, 3, 8), 2, 23, 24, 2, False)),
    'innermost': (('m', 'a', 'b', 's'), 's',
                  (('s', 'm', 'a', 'b'), 0, (23, 2, 3, 8), 1, 23, 48, 3, True)),
    'innermost of two': (('a', 's'), 's',
                         (('s', 'a'), 0, (23, 3), 1, 23, 3, 1, True)),
    'lone': (('s',), 's', (('s',), 0, (23,), 1, 23, 1, 0, False)),
    'one name in a list': (('m', 's', 'a', 'b'), ['s'],
                           (('m', 's', 'a', 'b'), 1, (2, 23, 3, 8), 2, 23, 24,
                            2, False)),
    'two adjacent': (('m', 's', 'a', 'b'), ['s', 'a'],
                     (('m', 's', 'a', 'b'), 1, (2, 23, 3, 8), 2, 69, 8, 1,
                      False)),
    'two adjacent, named backwards': (
        ('m', 's', 'a', 'b'), ['a', 's'],
        (('s', 'a', 'm', 'b'), 0, (23, 3, 2, 8), 1, 69, 16, 2, True)),
    'two adjacent at the end': (('m', 's', 'a', 'b'), ['a', 'b'],
                                (('a', 'b', 'm', 's'), 0, (3, 8, 2, 23), 1,
                                 24, 46, 2, True)),
    'two apart': (('m', 's', 'a', 'b'), ['m', 'a'],
                  (('m', 'a', 's', 'b'), 0, (2, 3, 23, 8), 1, 6, 184, 2,
                   True)),
    'all': (('m', 's', 'a', 'b'), ['m', 's', 'a', 'b'],
            (('m', 's', 'a', 'b'), 0, (2, 23, 3, 8), 1, 1104, 1, 0, False)),
}


def _layout(name):
  dims, reduced, _ = TABLE[name]
  return operands.SeriesLayout.of(dims, SIZES, reduced)


@pytest.mark.parametrize('name', list(TABLE))
def test_layout_table(name):
  lay = _layout(name)
  assert (lay.order, lay.first, lay.shape, lay.n_outer, lay.n_series,
          lay.n_point, lay.n_inner_dims, lay.copied) == TABLE[name][2]
  assert lay.dims == TABLE[name][0]
  for v in (lay.first, lay.n_outer, lay.n_series, lay.n_point) + lay.shape:
    assert type(v) is int


def test_an_empty_extent_gives_zero_not_an_error():
  lay = operands.SeriesLayout.of(('m', 's', 'a'), {'m': 2, 's': 0, 'a': 3},
                                 's')
  assert (lay.n_outer, lay.n_series, lay.n_point) == (2, 0, 3)


def _array(name, dtype=np.float64):
  dims = TABLE[name][0]
  shape = tuple(SIZES[d] for d in dims)
  return xl.DataArray(np.arange(int(np.prod(shape)), dtype=dtype).reshape(
      shape), dims)


@pytest.mark.parametrize('as_tensor', [False, True])
@pytest.mark.parametrize('name', ['first', 'middle', 'innermost',
                                  'innermost of two', 'lone'])
def test_host_then_restore_is_the_identity(name, as_tensor):
  da = _array(name)
  lay = _layout(name)
  flat = lay.host(da)
  assert flat.shape == (lay.n_outer, lay.n_series, lay.n_point)
  assert flat.dtype == np.float64
  # the series axis at `first` (the table test pins it), the rest in order
  assert np.array_equal(flat, np.moveaxis(
      da.data, da.dims.index('s'), lay.first).reshape(flat.shape))
  a = torch.from_numpy(flat.copy()) if as_tensor else flat
  back = lay.restore(a, (lay.n_series,))
  assert tuple(back.shape) == da.shape
  assert np.array_equal(np.asarray(back), da.data)
  assert isinstance(back, torch.Tensor) == as_tensor


@pytest.mark.parametrize('name', ['first', 'middle', 'innermost', 'lone'])
def test_restore_with_another_extent(name):
  """K13: the bins stand where the time stood."""
  da = _array(name)
  lay = _layout(name)
  axis = da.dims.index('s')
  flat = lay.host(da)[:, 3:8]  # five "bins": steps 3..7
  back = lay.restore(np.ascontiguousarray(flat), (5,))
  assert np.array_equal(back, np.take(da.data, range(3, 8), axis=axis))


@pytest.mark.parametrize('as_tensor', [False, True])
@pytest.mark.parametrize('name', ['first', 'middle', 'innermost', 'lone'])
def test_restore_splits_cycle_and_position(name, as_tensor):
  """K14 / K15: [n_outer, n_cycle * n_pos, n_point] -> the `hour` plane in
  front, the position where the time stood; without hours, plane 0 of it."""
  lay = _layout(name)
  dims = TABLE[name][0]
  axis = dims.index('s')
  n_cycle, n_pos = 2, 4
  rest = tuple(SIZES[d] for d in dims if d != 's')
  # value = 1000 * cycle + 100 * position + the index of the other dims
  other = np.arange(int(np.prod(rest, dtype=np.int64))).reshape(rest)
  want = (1000 * np.arange(n_cycle).reshape((-1,) + (1,) * len(dims))
          + 100 * np.expand_dims(
              np.arange(n_pos).reshape((-1,) + (1,) * len(rest)), 0)
          + other[None, None])  # [cycle, position, rest..]
  want = np.moveaxis(want, 1, 1 + axis)
  # the kernel's flat plane of the same values
  flat = np.moveaxis(want, 1 + axis, 1)  # [cycle, position, rest in dims]
  keep = [d for d in dims if d != 's']
  outer = [d for d in lay.order[:lay.first]]
  inner = [d for d in lay.order[lay.first + 1:]]
  perm = ([2 + keep.index(d) for d in outer] + [0, 1]
          + [2 + keep.index(d) for d in inner])
  flat = np.ascontiguousarray(np.transpose(flat, perm)).reshape(
      lay.n_outer, n_cycle * n_pos, lay.n_point)
  a = torch.from_numpy(flat) if as_tensor else flat
  got = lay.restore(a, (n_cycle, n_pos))
  assert np.array_equal(np.asarray(got), want)
  single = lay.restore(a[:, :n_pos], (1, n_pos))[0]  # no `hour` plane
  assert np.array_equal(np.asarray(single), want[0])


def test_restore_of_a_quantile_keeps_the_leading_axis():
  lay = _layout('two apart')  # order (m, a, s, b): the kept dims are s, b
  flat = np.arange(2 * 1 * 184).reshape(2, 1, 184)
  got = lay.restore(flat, (), (2,))
  assert got.shape == (2, 23, 8)
  assert np.array_equal(got, flat.reshape(2, 23, 8))
  lay = _layout('two adjacent')  # in place: kept m before, b after
  flat = np.arange(3 * 2 * 8).reshape(3, 2, 8)
  assert np.array_equal(lay.restore(flat, (), (3,)), flat.reshape(3, 2, 8))


def test_host_casts_what_is_not_float():
  da = _array('middle', np.int32)
  lay = _layout('middle')
  assert lay.host(da).dtype == np.float64
  assert lay.host(_array('middle', np.float32)).dtype == np.float32
  assert np.array_equal(lay.host(da), da.data.reshape(2, 23, 24))


# -- stride_table --------------------------------------------------------------
def test_stride_table_of_whole_block_views():
  full = torch.arange(2 * 23 * 3 * 8, dtype=torch.float32).reshape(2, 23, 3, 8)
  view = full[:, 1::2]
  assert operands.stride_table(view, 2).tolist() == [
      0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20,
      23, 25, 27, 29, 31, 33, 35, 37, 39, 41, 43]
  # one inner dim: rows of 8 are the blocks
  assert operands.stride_table(full[:, ::11, 1:], 1).tolist() == [
      0, 1, 33, 34, 66, 67, 69, 70, 102, 103, 135, 136]
  # no inner dim: a table of elements
  assert operands.stride_table(full[0, 0, :, ::4], 0).tolist() == [
      0, 4, 8, 12, 16, 20]
  # a transposed outer part is still whole blocks
  assert operands.stride_table(full.permute(1, 0, 2, 3)[:2], 2).tolist() == [
      0, 23, 1, 24]


def test_stride_table_ignores_the_stride_of_size_one_dims():
  full = torch.zeros(4, 5, 6)
  view = full[:, 2:3]  # [4, 1, 6]: the stride of the middle dim is moot
  assert operands.stride_table(view, 2).tolist() == [0, 5, 10, 15]
  assert operands.stride_table(full[1:2, ::2], 1).tolist() == [0, 2, 4]


def test_stride_table_refuses_broken_blocks():
  full = torch.zeros(4, 6, 8)
  assert operands.stride_table(full[:, :, ::2], 1) is None  # strided inside
  assert operands.stride_table(full[:, :, 1:], 2) is None  # partial block
  assert operands.stride_table(full[:, 1:, :], 2) is None  # 48 % 40 != 0
  # overlapping blocks: an outer stride of half a block (torch has no
  # negative strides to offer; the `s < 0` test guards foreign tensors)
  half = torch.as_strided(full, (3, 6, 8), (24, 8, 1))
  assert operands.stride_table(half, 2) is None
  assert operands.stride_table(full[:, :, :0], 1) is None  # nothing inside


def test_dtypes():
  assert operands.float_dtype(np.float32, torch.float32) == torch.float32
  assert operands.float_dtype(np.float32, np.float64) == torch.float64
  assert operands.float_dtype(np.dtype('int16')) == torch.float64
  assert operands.float_dtype(torch.int64) == torch.float64
  assert operands.torch_dtype(np.float32) == torch.float32
  assert operands.torch_dtype(np.dtype('int16')) == torch.int16
  assert operands.torch_dtype(torch.bool) == torch.bool
  assert operands.numpy_dtype(torch.float64) == np.float64
  assert operands.numpy_dtype('uint8') == np.uint8


def test_on_device_of_host_data():
  assert not operands.on_device(np.zeros(3))
  assert not operands.on_device(torch.zeros(3))
  assert not operands.on_device(xl.SlabGather(np.zeros((2, 3, 4)),
                                              np.array([1, 0])))


# -- the coordinate helpers ----------------------------------------------------
def test_coords_without():
  along_time = xl.DataArray(np.zeros(4), ('time',))
  along_level = xl.DataArray(np.zeros(2), ('level',))
  scalar_named_time = xl.DataArray(np.asarray(7.0), ())
  coords = {'time': np.arange(4), 'level': np.arange(2), 'valid': along_time,
            'height': along_level, 'label': 'x'}
  assert list(xl.coords_without(coords, ('time',))) == ['level', 'height',
                                                         'label']
  assert list(xl.coords_without(coords, ['level', 'time'])) == ['label']
  assert xl.coords_without(coords, ()) == coords
  assert xl.coords_without(coords, ('time',))['height'] is along_level
  # a DataArray named after a dim goes even where it does not lie along it
  assert xl.coords_without({'time': scalar_named_time, 'level': along_level},
                           ('time',)) == {'level': along_level}
  # and one that lies along a dim goes whatever its name
  assert xl.coords_without({'level': along_time}, ('time',)) == {}


def test_coord_values():
  ds = xl.Dataset(coords={'time': np.arange(4),
                          'valid': xl.DataArray(np.arange(4.0), ('time',)),
                          'levels': [500, 850]})
  assert xl.coord_values(ds, 'time').tolist() == [0, 1, 2, 3]
  got = xl.coord_values(ds, 'valid')
  assert isinstance(got, np.ndarray) and got.tolist() == [0.0, 1.0, 2.0, 3.0]
  assert xl.coord_values(ds, 'levels').tolist() == [500, 850]
  da = xl.DataArray(np.zeros(4), ('time',), {'time': np.arange(4) * 2})
  assert xl.coord_values(da, 'time').tolist() == [0, 2, 4, 6]
  with pytest.raises(KeyError):
    xl.coord_values(ds, 'level')
