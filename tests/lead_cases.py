"""Seeded cases of the lead-time fixtures: shared by the generator
(tests/golden/make_lead_vectors.py, which runs the reference on them) and by
the tests (which rebuild the same inputs from the seed).

A case is {'coords': {name: 1-D array}, 'vars': {name: (dims, array)},
'labels': the labels of CLASSES that run on it}.  `total_precipitation` is
cumulative along the lead axis with steps of a few millimetres (in metres) and
small negative steps mixed in -- many of them at some points, so that the
clamp acts on the 24-hour sums too; the raw 6- and 12-hour accumulations are
non-negative noise.
"""
import numpy as np

from tests import derived_cases as dc

REQUIRED = dc.REQUIRED
LEAD = 'prediction_timedelta'

# label -> (class name, constructor arguments); the first four are the keys of
# the reference's dictionary, with its arguments
CLASSES = {
    'total_precipitation_6hr': (
        'PrecipitationAccumulation',
        dict(total_precipitation_name='total_precipitation',
             accumulation_hours=6, lead_time_name=LEAD)),
    'total_precipitation_24hr': (
        'PrecipitationAccumulation',
        dict(total_precipitation_name='total_precipitation',
             accumulation_hours=24, lead_time_name=LEAD)),
    'total_precipitation_24hr_from_6hr': (
        'AggregatePrecipitationAccumulation',
        dict(accumulation_hours=24, lead_time_name=LEAD)),
    'total_precipitation_24hr_from_12hr': (
        'AggregatePrecipitationAccumulation',
        dict(accumulation_hours=24, lead_time_name=LEAD,
             raw_accumulation_name='total_precipitation_12hr',
             raw_accumulation_hours=12)),
    'tp6_unclamped': (
        'PrecipitationAccumulation',
        dict(total_precipitation_name='total_precipitation',
             accumulation_hours=6, set_negative_to_zero=False)),
    'tp24_unclamped': (
        'PrecipitationAccumulation',
        dict(total_precipitation_name='total_precipitation',
             accumulation_hours=24, set_negative_to_zero=False)),
}
DICT_KEYS = tuple(CLASSES)[:4]
CLASS_NAMES = ('PrecipitationAccumulation',
               'AggregatePrecipitationAccumulation')

# The reference's names, for where the reference itself is not at hand
REFERENCE_FIELDS = {
    'PrecipitationAccumulation': {
        'total_precipitation_name': REQUIRED, 'accumulation_hours': REQUIRED,
        'lead_time_name': 'prediction_timedelta',
        'set_negative_to_zero': True},
    'AggregatePrecipitationAccumulation': {
        'accumulation_hours': REQUIRED,
        'raw_accumulation_name': 'total_precipitation_6hr',
        'raw_accumulation_hours': 6,
        'lead_time_name': 'prediction_timedelta'},
}
# The 22 keys of the reference's dictionary, in its order
REFERENCE_KEYS = (
    'wind_speed', '10m_wind_speed', 'divergence', 'vorticity',
    'vertical_velocity', 'eddy_kinetic_energy', 'geostrophic_wind_speed',
    'u_component_of_geostrophic_wind', 'v_component_of_geostrophic_wind',
    'ageostrophic_wind_speed', 'u_component_of_ageostrophic_wind',
    'v_component_of_ageostrophic_wind', 'lapse_rate', 'total_column_vapor',
    'total_column_liquid', 'total_column_ice', 'integrated_vapor_transport',
    'relative_humidity') + DICT_KEYS

PRECIPITATION = ('total_precipitation_6hr', 'total_precipitation_24hr',
                 'tp6_unclamped', 'tp24_unclamped')


def _fields(rs, dims, sizes, dtype):
  shape = tuple(sizes[d] for d in dims)
  axis = dims.index(LEAD)
  other = tuple(1 if d == LEAD else sizes[d] for d in dims)
  # per point: one step in ten, or nine in ten, is a small negative one
  p_negative = np.where(rs.random_sample(other) < 0.25, 0.9, 0.1)
  steps = rs.gamma(0.5, 4e-3, size=shape)
  steps = np.where(rs.random_sample(shape) < p_negative,
                   -2e-5 * rs.random_sample(shape), steps)
  out = {
      'total_precipitation': np.cumsum(steps, axis=axis),
      'total_precipitation_6hr': rs.gamma(0.5, 4e-3, size=shape),
      'total_precipitation_12hr': rs.gamma(0.5, 8e-3, size=shape),
  }
  if np.dtype(dtype).kind in 'iu':  # tenths of a millimetre, as integers
    return {k: (dims, np.round(a * 1e4).astype(dtype))
            for k, a in out.items()}
  return {k: (dims, a.astype(dtype)) for k, a in out.items()}


def _poke(variables, rs, values, count):
  """`values` written at `count` single (lead, point) places of each field."""
  for _, a in variables.values():
    for k in range(count):
      at = tuple(rs.randint(0, n) for n in a.shape)
      a[at] = values[k % len(values)]


def _case(seed, dims, sizes, dtype, step_hours, labels, poke=()):
  rs = np.random.RandomState(seed)
  coords = {
      'time': np.arange(sizes.get('time', 0)) * np.timedelta64(12, 'h')
              + np.datetime64('2020-01-01T00', 'ns'),
      'realization': np.arange(sizes.get('realization', 0)),
      LEAD: (np.arange(sizes[LEAD]) * np.timedelta64(step_hours, 'h')
             ).astype('timedelta64[ns]'),
      'latitude': np.linspace(-90, 90, sizes['latitude']),
      'longitude': np.arange(sizes['longitude']) * (360.0
                                                    / sizes['longitude']),
  }
  variables = _fields(rs, dims, sizes, dtype)
  if poke:
    _poke(variables, rs, poke, 12)
  return {'coords': {k: v for k, v in coords.items() if k in dims},
          'vars': variables, 'seed': seed, 'dtype': np.dtype(dtype).name,
          'labels': tuple(labels)}


def cases() -> dict:
  """{case name: builder}."""
  all_labels = tuple(CLASSES)
  return {
      # 6-hourly leads, the four dictionary entries: windows 1, 4, 4, 2
      'latlon_time': lambda: _case(
          31, ('time', LEAD, 'latitude', 'longitude'),
          {'time': 2, LEAD: 13, 'latitude': 9, 'longitude': 16}, np.float32, 6,
          all_labels),
      'lonlat_member_nan': lambda: _case(
          32, ('realization', LEAD, 'longitude', 'latitude'),
          {'realization': 3, LEAD: 11, 'longitude': 12, 'latitude': 7},
          np.float32, 6, all_labels, poke=(np.nan,)),
      'latlon_inf_f64': lambda: _case(
          33, ('time', LEAD, 'latitude', 'longitude'),
          {'time': 2, LEAD: 11, 'latitude': 7, 'longitude': 12}, np.float64, 6,
          all_labels, poke=(np.inf, -np.inf, np.nan)),
      # hourly leads, the lead axis first: windows 6 and 24
      'hourly_lead_first': lambda: _case(
          34, (LEAD, 'latitude', 'longitude'),
          {LEAD: 31, 'latitude': 7, 'longitude': 12}, np.float32, 1,
          PRECIPITATION),
      'hourly_f64': lambda: _case(
          35, ('realization', LEAD, 'latitude', 'longitude'),
          {'realization': 2, LEAD: 29, 'latitude': 5, 'longitude': 8},
          np.float64, 1, PRECIPITATION),
      # the lead axis last, integer input (float64 results)
      'lead_last_int': lambda: _case(
          36, ('latitude', 'longitude', LEAD),
          {'latitude': 7, 'longitude': 12, LEAD: 13}, np.int32, 6,
          all_labels),
      'lead_last_f32': lambda: _case(
          37, ('time', 'latitude', 'longitude', LEAD),
          {'time': 2, 'latitude': 5, 'longitude': 8, LEAD: 9}, np.float32, 6,
          all_labels, poke=(np.nan,)),
  }


# The reference's three known-answer tests (derived_variables_test.py:121-216)
# as data: integer-valued, so every sum is exact
_LEAD_0_36 = np.arange(0, 36 + 1, 6, dtype='timedelta64[h]')
_LEAD_6_36 = np.arange(6, 36 + 1, 6, dtype='timedelta64[h]')
_NAN = np.nan
KNOWN_ANSWERS = {
    'total_precipitation_6hr': {
        'vars': {'total_precipitation': (
            (LEAD,), np.array([0, 5, 15, 14, 20, 30, 30]))},
        'coords': {LEAD: _LEAD_0_36},
        'expected': np.array([_NAN, 5, 10, 0, 6, 10, 0])},
    'total_precipitation_24hr': {
        'vars': {'total_precipitation': (
            (LEAD,), np.array([0, 5, 15, 14, 20, 30, 30]))},
        'coords': {LEAD: _LEAD_0_36},
        'expected': np.array([_NAN, _NAN, _NAN, _NAN, 20, 25, 15])},
    'total_precipitation_24hr_from_6hr': {
        'vars': {'total_precipitation_6hr': (
            (LEAD,), np.array([5, 0, 2, 1, 0, 10]))},
        'coords': {LEAD: _LEAD_6_36},
        'expected': np.array([_NAN, _NAN, _NAN, 8, 3, 13])},
}


def fields_of(label: str) -> tuple:
  """(class name, every constructor field with its value) of a label."""
  name, kwargs = CLASSES[label]
  return name, {**REFERENCE_FIELDS[name], **kwargs}


def input_name(label: str) -> str:
  name, fields = fields_of(label)
  return fields['total_precipitation_name' if name == CLASS_NAMES[0]
                else 'raw_accumulation_name']


# One shard per case, each below the 1 MiB limit of a committed file.
GOLDEN_STEM = 'reference_lead_v1'


def golden_paths(directory: str) -> list:
  import glob
  import os
  return sorted(glob.glob(os.path.join(directory, GOLDEN_STEM + '.*.npz')))


def load_golden(directory: str) -> dict:
  """Every array of every shard, by its key."""
  out = {}
  for path in golden_paths(directory):
    with np.load(path) as z:
      for k in z.files:
        assert k not in out, k
        out[k] = z[k]
  return out


def structure(module, dictionary: dict) -> dict:
  """Class names, dataclass fields with defaults, base_variables, core_dims
  per label of `module`, and whether `dictionary` holds an equal object under
  the label: the reference's module and DERIVED_VARIABLE_DICT in the
  generator, the product's module and LEAD_VARIABLE_DICT in the tests."""
  import dataclasses
  labels = {}
  for label, (name, kwargs) in CLASSES.items():
    cls = getattr(module, name)
    obj = cls(**kwargs)
    labels[label] = {
        'class': name,
        'fields': {f.name: (REQUIRED if f.default is dataclasses.MISSING
                            else f.default) for f in dataclasses.fields(cls)},
        'field_order': [f.name for f in dataclasses.fields(cls)],
        'base_variables': list(obj.base_variables),
        'core_dims': [[list(d) for d in obj.core_dims[0]],
                      list(obj.core_dims[1])],
        'in_dict': obj == dictionary.get(label),
    }
  return {'labels': labels}
