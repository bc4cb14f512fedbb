"""Seeded cases of the derived-variable fixtures: shared by the generator
(tests/golden/make_derived_vectors.py, which runs the reference on them) and
by the tests (which rebuild the same inputs from the seed).

A case is {'coords': {name: 1-D array}, 'vars': {name: (dims, array)}}.  The
fields are shaped like the real ones (winds of ~10 m/s, geopotential that
falls with pressure plus ~1e3 m2/s2 of weather, 200-300 K, 1e-3..1e-2 kg/kg)
so that the reference's own float32 result is well conditioned.
"""
import numpy as np

# label -> (class name, constructor arguments)
CLASSES = {
    'wind_speed': ('WindSpeed', dict(u_name='u_component_of_wind',
                                     v_name='v_component_of_wind')),
    '10m_wind_speed': ('WindSpeed', dict(u_name='10m_u_component_of_wind',
                                         v_name='10m_v_component_of_wind')),
    'relative_humidity': ('RelativeHumidity', {}),
    'divergence': ('WindDivergence', {}),
    'vorticity': ('WindVorticity', {}),
    'geostrophic_wind_speed': ('GeostrophicWindSpeed', {}),
    'u_component_of_geostrophic_wind': ('UComponentOfGeostrophicWind', {}),
    'v_component_of_geostrophic_wind': ('VComponentOfGeostrophicWind', {}),
    'ageostrophic_wind_speed': ('AgeostrophicWindSpeed', {}),
    'u_component_of_ageostrophic_wind': ('UComponentOfAgeostrophicWind', {}),
    'v_component_of_ageostrophic_wind': ('VComponentOfAgeostrophicWind', {}),
}
GEOSTROPHIC = [k for k in CLASSES if 'geostrophic' in k]

# The reference's names (weatherbench2/derived_variables.py): what the module
# must offer where the reference itself is not at hand.  Class -> dataclass
# fields with defaults (REQUIRED = no default).
REQUIRED = '<required>'
REFERENCE_FIELDS = {
    'WindSpeed': {'u_name': REQUIRED, 'v_name': REQUIRED},
    'RelativeHumidity': {'temperature_name': 'temperature',
                         'specific_humidity_name': 'specific_humidity',
                         'pressure_name': 'level'},
    'WindDivergence': {'u_name': 'u_component_of_wind',
                       'v_name': 'v_component_of_wind'},
    'WindVorticity': {'u_name': 'u_component_of_wind',
                      'v_name': 'v_component_of_wind'},
    'GeostrophicWindSpeed': {'geopotential_name': 'geopotential'},
    'UComponentOfGeostrophicWind': {'geopotential_name': 'geopotential'},
    'VComponentOfGeostrophicWind': {'geopotential_name': 'geopotential'},
    'AgeostrophicWindSpeed': {'u_name': 'u_component_of_wind',
                              'v_name': 'v_component_of_wind',
                              'geopotential_name': 'geopotential'},
    'UComponentOfAgeostrophicWind': {'u_name': 'u_component_of_wind',
                                     'v_name': 'v_component_of_wind',
                                     'geopotential_name': 'geopotential'},
    'VComponentOfAgeostrophicWind': {'u_name': 'u_component_of_wind',
                                     'v_name': 'v_component_of_wind',
                                     'geopotential_name': 'geopotential'},
}
# keys of the reference's DERIVED_VARIABLE_DICT that this build leaves out
# (DESIGN.md section 7): the level-column family and the accumulations
LEFT_OUT_KEYS = (
    'vertical_velocity', 'eddy_kinetic_energy', 'lapse_rate',
    'total_column_vapor', 'total_column_liquid', 'total_column_ice',
    'integrated_vapor_transport', 'total_precipitation_6hr',
    'total_precipitation_24hr', 'total_precipitation_24hr_from_6hr',
    'total_precipitation_24hr_from_12hr')
REFERENCE_KEYS = tuple(CLASSES) + LEFT_OUT_KEYS


def _fields(rs, dims, sizes, level, dtype, nan_patches):
  shape = tuple(sizes[d] for d in dims)
  lev_shape = [sizes[d] if d == 'level' else 1 for d in dims]
  lev = np.asarray(level, dtype=np.float64).reshape(lev_shape)
  surface_dims = tuple(d for d in dims if d != 'level')
  surface_shape = tuple(sizes[d] for d in surface_dims)
  out = {
      'u_component_of_wind': (dims, 10.0 * rs.standard_normal(shape)),
      'v_component_of_wind': (dims, 8.0 * rs.standard_normal(shape)),
      # ~ R T ln(p0 / p) g-scaled: monotonically falling with pressure
      'geopotential': (dims, 7.0e4 * np.log(1050.0 / lev)
                       + 1.0e3 * rs.standard_normal(shape)),
      'temperature': (dims, 215.0 + 0.09 * lev
                      + 5.0 * rs.standard_normal(shape)),
      'specific_humidity': (dims, 1e-3 + 9e-3 * rs.random_sample(shape)),
      '10m_u_component_of_wind': (surface_dims,
                                  6.0 * rs.standard_normal(surface_shape)),
      '10m_v_component_of_wind': (surface_dims,
                                  6.0 * rs.standard_normal(surface_shape)),
  }
  out = {k: (d, a.astype(dtype)) for k, (d, a) in out.items()}
  if nan_patches:
    for k, (d, a) in out.items():
      for _ in range(3):
        at = tuple(slice(s, s + 2) for s in
                   (rs.randint(0, max(1, n - 1)) for n in a.shape))
        a[at] = np.nan
  return out


def _grid_case(seed, dims, sizes, latitude, dtype, nan_patches=False):
  rs = np.random.RandomState(seed)
  level = np.array([300, 500, 700, 850, 1000][:sizes['level']])
  coords = {
      'time': np.arange(sizes['time']) * np.timedelta64(6, 'h')
              + np.datetime64('2020-01-01T00', 'ns'),
      'level': level,
      'latitude': np.asarray(latitude, dtype=np.float64),
      'longitude': np.arange(sizes['longitude']) * (360.0
                                                    / sizes['longitude']),
  }
  assert len(coords['latitude']) == sizes['latitude']
  return {'coords': coords,
          'vars': _fields(rs, dims, sizes, level, dtype, nan_patches),
          'seed': seed, 'dtype': np.dtype(dtype).name}


LONLAT = ('time', 'level', 'longitude', 'latitude')
LATLON = ('time', 'level', 'latitude', 'longitude')
_POLES = dict(time=2, level=5, longitude=36, latitude=19)
_MID = dict(time=1, level=3, latitude=24, longitude=40)
_POLES_SMALL = dict(time=1, level=2, longitude=36, latitude=19)


def cases() -> dict:
  """{case name: builder}.  float32 cases carry ref32 and ref64, the float64
  case ref64 alone."""
  return {
      # lon-lat, latitudes -90 ... 90 in steps of 10: poles AND equator
      'lonlat_poles': lambda: _grid_case(
          11, LONLAT, _POLES, np.linspace(-90, 90, 19), np.float32),
      # lat-lon, neither pole nor equator; linspace: not uniform in float64
      'latlon_linspace': lambda: _grid_case(
          12, LATLON, _MID, np.linspace(-88, 88, 24), np.float32),
      'lonlat_nan': lambda: _grid_case(
          13, LONLAT, _POLES_SMALL, np.linspace(-90, 90, 19), np.float32,
          nan_patches=True),
      'latlon_f64': lambda: _grid_case(
          14, LATLON, _MID, np.linspace(-88, 88, 24), np.float64),
  }


# The reference's known answers (derived_variables_test.py:85-119) as data
KNOWN_ANSWERS = {
    'wind_speed': {
        'vars': {'u_component_of_wind': (('dim_0',),
                                         np.array([0, 3, np.nan])),
                 'v_component_of_wind': (('dim_0',), np.array([0, -4, 1]))},
        'coords': {},
        'expected': np.array([0, 5, np.nan]), 'atol': 1e-8},
    'relative_humidity': {
        'vars': {'temperature': (('level',), np.array([240, 280, 295, 310])),
                 'specific_humidity': (('level',),
                                       np.array([1e-3, 1e-2, 2e-2, 4e-2]))},
        'coords': {'level': np.array([50, 200, 500, 850])},
        # from metpy.calc.relative_humidity_from_specific_humidity
        'expected': np.array([0.2116, 0.3115, 0.5937, 0.8462]), 'atol': 1e-4},
}


def fields_of(label: str) -> tuple:
  """(class name, every constructor field with its value) of a label."""
  name, kwargs = CLASSES[label]
  return name, {**REFERENCE_FIELDS[name], **kwargs}


def as_float64(case: dict) -> dict:
  """The same values as float64 (what `ref64` of a float32 case is run on)."""
  return dict(case, vars={k: (d, a.astype(np.float64))
                          for k, (d, a) in case['vars'].items()})


# No committed file may exceed 1 MiB and float64 fields of noise do not
# compress: the fixture is written as one shard per case, the pole-and-equator
# case as two (the geostrophic family apart).
GOLDEN_STEM = 'reference_derived_v1'


def shard_of(case_name: str, label: str) -> str:
  if case_name == 'lonlat_poles':
    return f'{case_name}.{"geo" if label in GEOSTROPHIC else "wind"}'
  return case_name


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


def structure(module) -> dict:
  """Class names, dataclass fields with defaults, base_variables, core_dims
  per label and the dictionary keys of `module`: the reference's module in
  the generator, the product's in the tests."""
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
        'in_dict': obj == module.DERIVED_VARIABLE_DICT.get(label),
    }
  return {'labels': labels, 'keys': list(module.DERIVED_VARIABLE_DICT)}
