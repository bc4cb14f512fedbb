"""Writes tests/golden/reference_seeps_climatology_v1.<case>.npz: outputs of
the REFERENCE's own, unmodified scripts/compute_climatology.py
(`compute_seeps_chunk`, `compute_stat_chunk(statistic='quantile')`,
`SEEPSThreshold.compute`, `Quantile.compute`) on the seeded cases of
tests/seeps_climatology_cases.py, one shard per case (a committed file stays
below 1 MiB; tests/seeps_climatology_cases.load_golden reads them back as one
dict).

It runs on the mini-xarray of oracle/refshim/ with everything that
make_climatology_vectors.py gives the stand-in in its own process (that module
is imported for it: the flag stand-in, weighted std, groupby, resample, pad,
rolling(...).construct, and the loaded reference modules).  What the stand-in
still lacks is added here, again in this process only:
  * weighted(...).quantile(q, dim): xarray/core/weighted.py's
    `_weighted_quantile` with method 'linear' and skipna=None (NaNs dropped
    for floats): per 1-D series, drop NaN samples and samples of weight 0 (no
    sample left: NaN); sort by value; normalise the weights to sum 1; cum =
    [0, cumsum(w)]; n = 1 / S w^2 (Kish's effective sample size); h = (n - 1)
    q + 1; u = max((h - 1) / n, min(h / n, cum)); v = u n - h + 1; result =
    S data diff(v).  The `quantile` dim comes first; a scalar q gives a scalar
    `quantile` coordinate.
This is THIS build's reading of xarray.  Its independent pins are the
reference's own testSEEPSThreshold (scripts/compute_climatology_test.py:23-41),
whose input is recorded as the case `known` and whose assertion is made here,
and the pins of tests/test_seeps_climatology_cpu.py (equal weights against
NumPy's linear quantile, W = 3 against the plain quantile over the years).
Nothing under oracle/ changes.

Per case the files hold
  <case>/seeps_threshold, /seeps_dry_fraction, /quantile  (+ /dims)
and `known/data`, `known/seeps_threshold`, `known/seeps_dry_fraction`,
`known/quantile`.

Only runs where the reference is at hand:
    python tests/golden/make_seeps_climatology_vectors.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_climatology_vectors as base  # noqa: E402

xr, script, utils = base.xr, base.script, base.utils

from tests import seeps_climatology_cases as sc  # noqa: E402


# ---------------------------------------------------------------------------
# what the stand-in still lacks (this process only)
# ---------------------------------------------------------------------------
def _weighted_quantile_1d(data, weights, q, skipna):
  is_nan = np.isnan(data)
  if skipna:
    data, weights = data[~is_nan], weights[~is_nan]
  elif is_nan.any():
    return np.full(q.size, np.nan)
  nonzero = weights != 0
  data, weights = data[nonzero], weights[nonzero]
  if data.size == 0:
    return np.full(q.size, np.nan)
  sorter = np.argsort(data)
  data, weights = data[sorter], weights[sorter]
  weights = weights / weights.sum()
  weights_cum = np.append(0, weights.cumsum())
  q = np.atleast_2d(q).T
  n = 1 / (weights ** 2).sum()
  h = (n - 1) * q + 1
  u = np.maximum((h - 1) / n, np.minimum(h / n, weights_cum))
  v = u * n - h + 1
  w = np.diff(v)
  return (data * w).sum(axis=1)


def _weighted_quantile(self, da, q, dim, skipna):
  scalar = np.ndim(q) == 0
  qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
  if np.any((qs < 0) | (qs > 1)):
    raise ValueError('q values must be between 0 and 1')
  dims = list(da.dims) if dim is None or dim is ... else (
      [dim] if isinstance(dim, str) else list(dim))
  dims = [d for d in dims if d in da.dims]
  if skipna is None:
    skipna = da.dtype.kind in 'cfO'
  keep = tuple(d for d in da.dims if d not in dims)
  moved = da.transpose(*keep, *dims)
  values = np.asarray(moved.data)
  # the weights, broadcast against the variable
  w = np.asarray(self.weights.data, dtype=np.float64)
  shape = [moved.shape[moved.dims.index(d)] if d in self.weights.dims else 1
           for d in moved.dims]
  order = [self.weights.dims.index(d) for d in moved.dims
           if d in self.weights.dims]
  assert len(order) == self.weights.ndim, 'weights dims must be in the data'
  w = np.broadcast_to(np.transpose(w, order).reshape(shape), values.shape)
  lead = values.shape[:len(keep)]
  flat = values.reshape(int(np.prod(lead, dtype=np.int64)), -1)
  wflat = w.reshape(flat.shape)
  out = np.stack([_weighted_quantile_1d(flat[i], wflat[i], qs, skipna)
                  for i in range(flat.shape[0])], axis=-1) if flat.shape[0] \
      else np.zeros((qs.size, 0))
  out = out.reshape((qs.size,) + lead)
  coords = {k: (tuple(c.dims), np.asarray(c.data))
            for k, c in da.coords.items()
            if not set(c.dims) & set(dims)}
  if scalar:
    coords['quantile'] = ((), np.asarray(qs[0]))
    return xr.DataArray(out[0], coords=coords, dims=keep, name=da.name)
  coords['quantile'] = (('quantile',), qs)
  return xr.DataArray(out, coords=coords, dims=('quantile',) + keep,
                      name=da.name)


def _quantile(self, q, *, dim=None, keep_attrs=None, skipna=None):
  self._check_dim(dim)
  return self._apply(
      lambda da, dim, skipna: self._weighted_quantile(da, q, dim, skipna),
      dim, skipna, keep_attrs)


base._Weighted._weighted_quantile = _weighted_quantile  # pylint: disable=protected-access
base._Weighted.quantile = _quantile  # pylint: disable=protected-access


def to_dataset(case):
  return xr.Dataset({sc.VAR: (case['dims'], case['data'])},
                    {'time': case['times']})


def run(case):
  script.METHOD.value = 'explicit'
  ds = to_dataset(case)
  kwargs = dict(frequency=case['frequency'], window_size=case['window_size'],
                clim_years=case['clim_years'],
                hour_interval=case['hour_interval'])
  key = base._Key({d: 0 for d in case['dims']}, {sc.VAR})  # pylint: disable=protected-access
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')
    seeps_key, seeps = script.compute_seeps_chunk(
        key, ds, seeps_threshold_mm={sc.VAR: sc.DRY_MM}, **kwargs)
    quant_key, quant = script.compute_stat_chunk(
        key, ds, statistic='quantile', quantiles=list(case['quantiles']),
        **kwargs)
  names = [f'{sc.VAR}_seeps_threshold', f'{sc.VAR}_seeps_dry_fraction']
  assert seeps_key.vars == set(names) and sorted(seeps.data_vars) == sorted(
      names)
  assert quant_key.vars == {f'{sc.VAR}_quantile'}
  assert list(quant.data_vars) == [f'{sc.VAR}_quantile']
  return seeps[names[0]], seeps[names[1]], quant[f'{sc.VAR}_quantile']


def record(out, prefix, da):
  out[prefix] = np.asarray(da.data)
  out[prefix + '/dims'] = np.array(list(da.dims), dtype='U32')


def known(out):
  """scripts/compute_climatology_test.py:23-41, asserted as it asserts."""
  data = sc.known_input()
  name = 'total_precipitation_6hr'
  dataset = xr.Dataset({name: xr.DataArray(data)})
  result = script.SEEPSThreshold(0.25, name).compute(dataset, dim=...)
  out['known/data'] = data
  out['known/seeps_dry_fraction'] = np.asarray(
      result[name + '_seeps_dry_fraction'].data)
  out['known/seeps_threshold'] = np.asarray(
      result[name + '_seeps_threshold'].data)
  np.testing.assert_allclose(out['known/seeps_dry_fraction'], 1 / 5,
                             rtol=1e-5)
  np.testing.assert_allclose(out['known/seeps_threshold'], 4 / 1000,
                             rtol=1e-5)
  q = script.Quantile([0.25, 0.5]).compute(dataset, dim=...)
  out['known/quantile'] = np.asarray(q[name].data)
  np.testing.assert_allclose(out['known/quantile'],
                             np.quantile(data, [0.25, 0.5]))


def generate() -> dict:
  out = {}
  known(out)
  for cname, case in sc.reference_cases().items():
    thr, dry, quant = run(case)
    record(out, f'{cname}/seeps_threshold', thr)
    record(out, f'{cname}/seeps_dry_fraction', dry)
    record(out, f'{cname}/quantile', quant)
  return out


def main():
  out = generate()
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(sc.shard_of(key), {})[key] = value
  directory = os.environ.get('WB2_SEEPS_CLIMATOLOGY_OUT') or HERE
  for shard, arrays in by_shard.items():
    path = os.path.join(directory, f'{sc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')


if __name__ == '__main__':
  main()
