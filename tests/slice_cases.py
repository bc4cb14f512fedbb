"""Seeded inputs and options of the dataset-slicing cases, shared by
tests/golden/make_slice_vectors.py (which records what the reference's
scripts/slice_dataset.py makes of them) and the CPU and GPU tests.

An input is a plain description -- {'coords': {name: values or (dims,
values)}, 'vars': {name: (dims, values)}} -- that `to_lite` turns into an
`xarray_lite.Dataset` and the generator into the stand-in xarray's.  The
fixtures hold the expected outputs only: tests/golden/reference_slice_v1.json
(options, dims, variable order, known answers) and one
reference_slice_v1.<case>.npz per case (values and coordinates).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PREFIX = 'reference_slice_v1'

LAYOUTS = {'latlon': ('latitude', 'longitude'),
           'lonlat': ('longitude', 'latitude')}


def _special(values: np.ndarray) -> np.ndarray:
  """A NaN with a payload, -0.0 and an infinity among the values: a slice is
  a bit copy."""
  flat = values.reshape(-1)
  if flat.dtype == np.float32:
    flat[1:2].view(np.uint32)[0] = 0x7fc00123
  elif flat.dtype == np.float64:
    flat[1:2].view(np.uint64)[0] = 0x7ff8000000000456
  if flat.dtype.kind == 'f':
    flat[2], flat[3] = -0.0, np.inf
  return values


def mock_truth(reversed_lat: bool = False, seed: int = 0) -> dict:
  """The input of the reference's SliceDatasetTest: schema.mock_truth_data at
  30 degrees, daily over 2021, three 3-D float32 variables (time, level,
  longitude, latitude), random values, geopotential + 10."""
  rs = np.random.RandomState(seed)
  coords = {
      'time': np.arange('2021-01-01', '2022-01-01',
                        dtype='datetime64[D]').astype('datetime64[ns]'),
      'latitude': np.linspace(-90, 90, 7),
      'longitude': np.linspace(0, 360, 12, endpoint=False),
      'level': np.array([500, 700, 850]),
  }
  dims = ('time', 'level', 'longitude', 'latitude')
  shape = tuple(coords[d].size for d in dims)
  data = {k: rs.rand(*shape).astype(np.float32)
          for k in ('temperature', 'geopotential', 'should_drop')}
  data['geopotential'] = data['geopotential'] + np.float32(10)
  if reversed_lat:
    coords['latitude'] = coords['latitude'][::-1].copy()
    data = {k: np.ascontiguousarray(v[..., ::-1]) for k, v in data.items()}
  return {'coords': coords, 'vars': {k: (dims, v) for k, v in data.items()}}


def grid(layout: str = 'latlon', lat_decreasing: bool = False,
         seed: int = 1) -> dict:
  """48 six-hourly times across a new year, 3 levels, 7 x 12 points in either
  layout; float32, float64 and int32 variables, one without `level`, and a
  coordinate `day_index` that lies along `time` without being its index."""
  rs = np.random.RandomState(seed)
  lat = np.linspace(-90, 90, 7)
  coords = {
      'time': (np.datetime64('2020-12-24T00', 'ns')
               + np.arange(48) * np.timedelta64(6, 'h')),
      'level': np.array([500, 700, 850]),
      'latitude': lat[::-1].copy() if lat_decreasing else lat,
      'longitude': np.linspace(0, 360, 12, endpoint=False),
  }
  coords['day_index'] = (('time',), np.arange(48) // 4)
  dims = ('time', 'level') + LAYOUTS[layout]
  shape = tuple(np.asarray(coords[d]).size for d in dims)
  flat = ('time',) + LAYOUTS[layout]
  return {'coords': coords, 'vars': {
      't': (dims, _special(rs.randn(*shape).astype(np.float32))),
      'z': (dims, _special(rs.randn(*shape) * 1e3)),
      'n': (dims, rs.randint(-2**31, 2**31 - 1, shape).astype(np.int32)),
      'sp': (flat, _special(rs.randn(shape[0], *shape[2:]).astype(np.float32))),
  }}


def leads(seed: int = 2) -> dict:
  """A forecast: 8 six-hourly init times, 81 six-hourly leads (0 to 20 days),
  3 x 4 points, and a variable without time or lead."""
  rs = np.random.RandomState(seed)
  coords = {
      'time': (np.datetime64('2020-01-01T00', 'ns')
               + np.arange(8) * np.timedelta64(6, 'h')),
      'prediction_timedelta': (np.arange(81) * np.timedelta64(6, 'h')
                               ).astype('timedelta64[ns]'),
      'latitude': np.array([-30.0, 0.0, 30.0]),
      'longitude': np.array([0.0, 90.0, 180.0, 270.0]),
  }
  dims = ('time', 'prediction_timedelta', 'latitude', 'longitude')
  shape = tuple(coords[d].size for d in dims)
  return {'coords': coords, 'vars': {
      't2m': (dims, _special(rs.randn(*shape).astype(np.float32))),
      'bias': (dims[2:], rs.randn(*shape[2:])),
  }}


BUILDERS = {'mock_truth': mock_truth, 'grid': grid, 'leads': leads}

_KNOWN_CHUNKS = {'time': 40, 'longitude': 6, 'latitude': 5, 'level': 3}

# name -> (builder, its arguments, options of slice_dataset [, extras])
CASES = {
    # scripts/slice_dataset_test.py: test_simple_slicing
    'known_simple': ('mock_truth', {'reversed_lat': True}, {
        'sel': 'time_start=2021-02-01,time_stop=2021-04-01,time_step=5,'
               'longitude_step=60',
        'isel': 'latitude_stop=5', 'drop_variables': 'should_drop',
        'make_dims_increasing': 'latitude'}),
    # ... test_slicing_with_lists_and_dropping
    'known_lists': ('mock_truth', {}, {
        'sel': 'longitude_list=60+150', 'drop_isel': 'latitude_list=-1',
        'drop_variables': 'should_drop'}),
}
_GRID_CASES = {
    'box': (False, {'sel': 'latitude_start=-33.33,latitude_stop=33.33,'
                           'longitude_start=0,longitude_stop=180'}),
    'box_decreasing': (True, {'sel': 'latitude_start=33.33,'
                                     'latitude_stop=-33.33,longitude_step=4'}),
    'empty_decreasing': (True, {'sel': 'latitude_start=-33.33,'
                                       'latitude_stop=33.33'}),
    'empty_time': (False, {'sel_strings': 'time_start=2022'}),
    'increasing': (True, {'make_dims_increasing': 'latitude'}),
    'increasing_box': (True, {
        'make_dims_increasing': 'latitude',
        'sel': 'latitude_start=-45.5,latitude_stop=61,longitude_start=45',
        'isel': 'longitude_step=4'}),
    'year': (False, {'sel_strings': 'time_start=2021'}),
    'month': (False, {'sel_strings': 'time_stop=2020-12,time_step=3'}),
    'day': (False, {'sel_strings': 'time_start=2020-12-31,'
                                   'time_stop=2021-01-01'}),
    'hour': (False, {'sel_strings': 'time_start=2020-12-31T06,'
                                    'time_stop=2021-01-01T12,time_step=2'}),
    'isel_lists': (False, {'isel': 'time_list=3+-1+3+0,'
                                   'longitude_list=11+0+5+0,level_list=2+0'}),
    'lat_list': (True, {'isel': 'latitude_list=6+2+2+-7'}),
    'drops': (False, {'drop_isel': 'time_list=0+-1+5',
                      'drop_sel': 'level_list=700,longitude_list=30+330',
                      'drop_sel_strings': 'time_list=2020-12-26+2021-01-01'}),
    'keep': (False, {'keep_variables': 'z,t', 'isel': 'longitude_step=4'}),
    'levels': (False, {'sel': 'level_list=850+500'}),
    'time_only': (False, {'isel': 'time_start=2,time_stop=40,time_step=7'}),
    'everything': (True, {
        'make_dims_increasing': 'latitude', 'drop_variables': 'n,day_index',
        'isel': 'level_list=2+1', 'sel': 'longitude_start=15,longitude_stop=300',
        'sel_strings': 'time_start=2020-12-25,time_stop=2021-01-02,time_step=3',
        'drop_isel': 'longitude_list=0', 'drop_sel': 'latitude_list=0'}),
}
for _layout in LAYOUTS:
  for _name, (_dec, _options) in _GRID_CASES.items():
    CASES[f'{_layout}_{_name}'] = (
        'grid', {'layout': _layout, 'lat_decreasing': _dec}, _options)
CASES.update({
    'lead_days': ('leads', {}, {
        'sel_strings': 'prediction_timedelta_start=1 day,'
                       'prediction_timedelta_stop=15 days'}),
    'lead_days_step': ('leads', {}, {
        'sel': 'prediction_timedelta_stop=15 days,prediction_timedelta_step=4',
        'isel': 'time_start=1'}),
    'lead_hours': ('leads', {}, {
        'sel_strings': 'prediction_timedelta_start=6h,'
                       'prediction_timedelta_stop=36h'}),
})

# inputs of the reference's GetSelectionsTest: (flag values, force_string)
KNOWN_SELECTIONS = {
    'valid_selections': ({'A_start': '1 day', 'A_stop': '10 days', 'A_step': 2,
                          'B_stop': 2.2, 'C_step': 3,
                          'D_list': 'planes+trains+automobiles'}, False),
    'valid_selections_is_sel_or_dropsel': (
        {'A_start': '1 day', 'A_stop': '10 days', 'A_step': 2, 'B_stop': 2020,
         'D_list': 'planes+trains+automobiles'}, True),
    'valid_index_selections': (
        {'A_list': '9+-1+0', 'B_list': '-1+-2+02', 'X_start': 0, 'X_stop': 10,
         'X_step': 2, 'Y_stop': 4, 'Z_start': 1, 'W_step': 2}, False),
}
# the reference test's chunks: input, the output_chunks flag
KNOWN_CHUNKS = {'input': _KNOWN_CHUNKS, 'overrides': {'level': 1}}


def build(name: str) -> dict:
  builder, kwargs, _ = CASES[name]
  return BUILDERS[builder](**kwargs)


def options(name: str) -> dict:
  return dict(CASES[name][2])


def encode_selection(selection: dict) -> dict:
  """{dim: slice | list} as JSON: {'dim':, 'slice': [start, stop, step]} or
  {'dim':, 'list': [...]}."""
  (dim, s), = selection.items()
  if isinstance(s, slice):
    return {'dim': dim, 'slice': [s.start, s.stop, s.step]}
  return {'dim': dim, 'list': list(s)}


def to_lite(description: dict, device=None):
  """The `xarray_lite.Dataset` of a description; with `device` the variables
  are torch tensors there."""
  from weatherbench2_amd import xarray_lite as xl
  coords = {}
  for name, c in description['coords'].items():
    coords[name] = (xl.DataArray(np.asarray(c[1]), c[0], {}, name)
                    if isinstance(c, tuple) else np.asarray(c))
  ds = xl.Dataset(coords=coords)
  for name, (dims, values) in description['vars'].items():
    if device is not None:
      import torch
      values = torch.from_numpy(values.copy()).to(device)
    ds.data_vars[name] = xl.DataArray(values, dims, ds.coords, name)
  return ds


_META = None


def meta() -> dict:
  global _META
  if _META is None:
    with open(os.path.join(GOLDEN, PREFIX + '.json')) as f:
      _META = json.load(f)
  return _META


def load(name: str) -> dict:
  """The recorded output of a case: {'order': variable names, 'dims': {name:
  dims}, 'vars': {name: values}, 'coords': {name: values}, 'coord_dims':
  {name: dims}}."""
  case = meta()['cases'][name]
  with np.load(os.path.join(GOLDEN, f'{PREFIX}.{name}.npz')) as z:
    arrays = {k: z[k] for k in z.files}
  return {'order': case['order'], 'dims': case['dims'],
          'coord_dims': case['coord_dims'],
          'vars': {k: arrays['var/' + k] for k in case['order']},
          'coords': {k: arrays['coord/' + k] for k in case['coord_dims']}}
