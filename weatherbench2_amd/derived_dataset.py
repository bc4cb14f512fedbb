"""The dataset-level derived-variables driver: `main` of
scripts/compute_derived_variables.py (:146-221) without IO.

The script removes and renames variables of the source dataset, checks that
every derived variable is new and has its base variables, and assigns
`dv.compute(dataset)` for each.  Its two rechunking branches do not exist
here: a dataset holds its whole lead axis, so the precipitation accumulations
are computed like every other variable.
"""
from __future__ import annotations

import typing as t

from weatherbench2_amd import derived_variables as dvs
from weatherbench2_amd import xarray_lite as xl

# the script's _DEFAULT_DERIVED_VARIABLES
DEFAULT_DERIVED_VARIABLES = (
    'wind_speed', '10m_wind_speed', 'divergence', 'vorticity',
    'vertical_velocity', 'eddy_kinetic_energy', 'geostrophic_wind_speed',
    'ageostrophic_wind_speed', 'lapse_rate', 'total_column_vapor',
    'integrated_vapor_transport', 'relative_humidity',
    'total_precipitation_6hr', 'total_precipitation_24hr')


def resolve(names: t.Sequence[str], known: t.Optional[t.Mapping] = None
            ) -> dict:
  """{output name: derived variable} of the script's loop (:147-161): a
  `total_precipitation_*_from_*` name loses its `_from_` suffix, and the
  shortened name must not be listed itself."""
  known = dvs.REFERENCE_DERIVED_VARIABLES if known is None else known
  names = list(names)
  out = {}
  for variable_name in names:
    dv = known[variable_name]
    if (variable_name.startswith('total_precipitation_')
        and '_from_' in variable_name):
      variable_name = variable_name.split('_from_')[0]
      assert variable_name not in names, (
          'Duplicate variable name after removing suffix.')
    out[variable_name] = dv
  return out


def _rename(ds: xl.Dataset, names: t.Mapping[str, str]) -> xl.Dataset:
  """`Dataset.rename`: variables, coordinates and dims."""
  missing = [k for k in names if k not in ds.data_vars and k not in ds.coords
             and k not in ds.dims]
  if missing:
    raise ValueError(f'cannot rename {missing[0]!r} because it is not a '
                     'variable or dimension in this dataset')
  new = lambda k: names.get(k, k)
  coords = {}
  for k, c in ds.coords.items():
    if isinstance(c, xl.DataArray):
      c = xl.DataArray(c.data, tuple(new(d) for d in c.dims), {}, new(k))
    coords[new(k)] = c
  out = xl.Dataset(coords=coords, attrs=ds.attrs)
  for k, v in ds.data_vars.items():
    out.data_vars[new(k)] = xl.DataArray(
        v.data, tuple(new(d) for d in v.dims), out.coords, new(k))
  return out


def compute_derived_variables(
    ds, derived_variables: t.Sequence[str] = DEFAULT_DERIVED_VARIABLES,
    preexisting_variables_to_remove: t.Sequence[str] = (),
    rename_raw_tp_name: bool = False,
    raw_tp_name: str = 'total_precipitation',
    rename_variables: t.Optional[t.Mapping[str, str]] = None,
    known: t.Optional[t.Mapping] = None):
  """`ds` with every derived variable of `derived_variables` (names resolved
  in `REFERENCE_DERIVED_VARIABLES`, or in `known`) added behind its own
  variables, in the order given.  First the variables of
  `preexisting_variables_to_remove` leave if they are there, `raw_tp_name`
  becomes 'total_precipitation' with `rename_raw_tp_name`, and
  `rename_variables` is applied.  A derived variable that already exists and
  one whose base variables are missing are ValueErrors, raised before
  anything is computed.  The new variables carry no attributes."""
  like = ds
  ds = xl.as_dataset(ds)
  derived = resolve(derived_variables, known)
  remove = set(preexisting_variables_to_remove)
  # (an xarray Dataset's keys are its variables AND its coordinates: a name to
  # remove, an existing name and a base variable -- RelativeHumidity's `level`
  # -- may each be a coordinate)
  source = xl.Dataset(
      coords={k: c for k, c in ds.coords.items() if k not in remove},
      attrs=ds.attrs)
  for k, v in ds.data_vars.items():
    if k not in remove:
      source.data_vars[k] = xl.DataArray(v.data, v.dims, source.coords, k)
  if rename_raw_tp_name:
    source = _rename(source, {raw_tp_name: 'total_precipitation'})
  if rename_variables:
    source = _rename(source, dict(rename_variables))
  have = set(source.data_vars) | set(source.coords)
  for var_name, dv in derived.items():
    if var_name in have:
      raise ValueError(
          f'cannot compute {var_name!r} because it already exists in the source'
          ' dataset. Consider including it in '
          'preexisting_variables_to_remove.')
    if not set(dv.base_variables) <= have:
      raise ValueError(
          f'cannot compute {var_name!r} because its base variables '
          f'{dv.base_variables} are not found in the source dataset:\n'
          f'{source}')
  out = source.copy()
  # (every variable is computed from the SOURCE, as `Dataset.assign` does)
  for var_name, dv in derived.items():
    value = dv.compute(source)
    out[var_name] = xl.DataArray(value.data, value.dims, value.coords,
                                 var_name)
  return xl.like_input(out, like)
