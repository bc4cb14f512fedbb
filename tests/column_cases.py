"""Seeded cases of the level-column fixtures: shared by the generator
(tests/golden/make_column_vectors.py, which runs the reference on them) and by
the tests (which rebuild the same inputs from the seed).

The cases are those of tests/derived_cases.py with two cloud-water fields
added (drawn from a RandomState of their own, so that the existing draws stay
where they are), the 13 ERA5 pressure levels with an int64 and with a float32
level coordinate, and a decreasing level coordinate.
"""
import numpy as np

from tests import derived_cases as dc

REQUIRED = dc.REQUIRED

# label -> (class name, constructor arguments); the first seven are the keys
# of the reference's dictionary
CLASSES = {
    'vertical_velocity': ('VerticalVelocity', {}),
    'eddy_kinetic_energy': ('EddyKineticEnergy', {}),
    'lapse_rate': ('LapseRate', {}),
    'total_column_vapor': ('TotalColumnWater',
                           dict(water_species_name='specific_humidity')),
    'total_column_liquid': (
        'TotalColumnWater',
        dict(water_species_name='specific_cloud_liquid_water_content')),
    'total_column_ice': (
        'TotalColumnWater',
        dict(water_species_name='specific_cloud_ice_water_content')),
    'integrated_vapor_transport': ('IntegratedWaterTransport', {}),
    'ivt_500_850': ('IntegratedWaterTransport',
                    dict(level_min=500, level_max=850)),
    'ivt_open': ('IntegratedWaterTransport',
                 dict(level_min=None, level_max=None)),
}
DICT_KEYS = tuple(CLASSES)[:7]
CLASS_NAMES = ('TotalColumnWater', 'IntegratedWaterTransport', 'LapseRate',
               'VerticalVelocity', 'EddyKineticEnergy')

# The reference's names, for where the reference itself is not at hand
REFERENCE_FIELDS = {
    'VerticalVelocity': {'u_name': 'u_component_of_wind',
                         'v_name': 'v_component_of_wind'},
    'EddyKineticEnergy': {'u_name': 'u_component_of_wind',
                          'v_name': 'v_component_of_wind'},
    'LapseRate': {'temperature_name': 'temperature',
                  'geopotential_name': 'geopotential'},
    'TotalColumnWater': {'water_species_name': 'specific_humidity'},
    'IntegratedWaterTransport': {'u_name': 'u_component_of_wind',
                                 'v_name': 'v_component_of_wind',
                                 'water_species_name': 'specific_humidity',
                                 'level_min': 300, 'level_max': 1000},
}
# results without a `level` dim
INTEGRALS = tuple(k for k in CLASSES
                  if k not in ('vertical_velocity', 'lapse_rate'))

# (case, label) pairs where the reference's result is identically 0.0, so that
# a relative tolerance means nothing: one selected level on the two-level
# case, an empty selection on the decreasing one.  The generator asserts the
# zeros; the tests demand exact zeros.
ZERO = (('lonlat_nan', 'ivt_500_850'),
        ('decreasing', 'integrated_vapor_transport'),
        ('decreasing', 'ivt_500_850'))

ERA5_LEVELS = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
_ERA5 = dict(time=1, level=13, latitude=19, longitude=36)
_FIVE = dict(time=1, level=5, latitude=19, longitude=36)


def _cloud_water(case: dict, nan_patches: bool) -> dict:
  """`case` with the two cloud-water fields, in the dims of the humidity."""
  rs = np.random.RandomState(1000 + case['seed'])
  dims, q = case['vars']['specific_humidity']
  extra = {}
  for name, top in (('specific_cloud_liquid_water_content', 3e-4),
                    ('specific_cloud_ice_water_content', 1e-4)):
    a = (1e-6 + top * rs.random_sample(q.shape)).astype(q.dtype)
    if nan_patches:
      for _ in range(3):
        at = tuple(slice(s, s + 2) for s in
                   (rs.randint(0, max(1, n - 1)) for n in a.shape))
        a[at] = np.nan
    extra[name] = (dims, a)
  return dict(case, vars={**case['vars'], **extra})


def _level_case(seed, sizes, level, dtype=np.float32):
  """A lat-lon case on the pole-and-equator grid with the given level
  coordinate (its dtype is part of the case)."""
  rs = np.random.RandomState(seed)
  level = np.asarray(level)
  assert len(level) == sizes['level']
  coords = {
      'time': np.arange(sizes['time']) * np.timedelta64(6, 'h')
              + np.datetime64('2020-01-01T00', 'ns'),
      'level': level,
      'latitude': np.linspace(-90, 90, sizes['latitude']),
      'longitude': np.arange(sizes['longitude']) * (360.0
                                                    / sizes['longitude']),
  }
  case = {'coords': coords,
          'vars': dc._fields(rs, dc.LATLON, sizes, level, dtype, False),
          'seed': seed, 'dtype': np.dtype(dtype).name}
  return _cloud_water(case, False)


def cases() -> dict:
  """{case name: builder}.  float32 cases carry ref32 and ref64, the float64
  case ref64 alone."""
  out = {name: (lambda build=build, name=name: _cloud_water(
      build(), name == 'lonlat_nan')) for name, build in dc.cases().items()}
  out['era5_levels'] = lambda: _level_case(
      21, _ERA5, np.array(ERA5_LEVELS, dtype=np.int64))
  out['era5_levels_f32'] = lambda: _level_case(
      22, _ERA5, np.array(ERA5_LEVELS, dtype=np.float32))
  out['decreasing'] = lambda: _level_case(
      23, _FIVE, np.array([1000, 850, 700, 500, 300], dtype=np.int64))
  return out


as_float64 = dc.as_float64


def fields_of(label: str) -> tuple:
  """(class name, every constructor field with its value) of a label."""
  name, kwargs = CLASSES[label]
  return name, {**REFERENCE_FIELDS[name], **kwargs}


# One shard per case, each below the 1 MiB limit of a committed file.
GOLDEN_STEM = 'reference_column_v1'


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
  generator, the product's module and COLUMN_VARIABLE_DICT in the tests."""
  import dataclasses
  labels = {}
  for label, (name, kwargs) in CLASSES.items():
    cls = getattr(module, name)
    obj = cls(**kwargs)
    labels[label] = {
        'class': name,
        'fields': {f.name: (REQUIRED if f.default is dataclasses.MISSING
                            else f.default) for f in dataclasses.fields(cls)},
        'base_variables': list(obj.base_variables),
        'core_dims': [[list(d) for d in obj.core_dims[0]],
                      list(obj.core_dims[1])],
        'in_dict': obj == dictionary.get(label),
    }
  return {'labels': labels}
