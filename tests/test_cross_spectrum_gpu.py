"""Scale-dependent verification on the device (-m gpu): K25
(csrc/cross_spectrum.hip) against the dense restatement
(tests/cross_spectrum_np.py) within the bounds stated there, its tie to K4f,
the operands read in place, the invalid rows, the fold and the public path,
at the smallest shapes at which the kernel can go wrong."""
import numpy as np
import pytest
import torch

from tests import cross_spectrum_cases as cases
from tests import cross_spectrum_np as snp
from tests import helpers
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import derived_variables as dv
from weatherbench2_amd import engine
from weatherbench2_amd import spectral
from weatherbench2_amd import xarray_lite as xl

pytestmark = pytest.mark.gpu

g = helpers.to_gpu_dataset
NAME = cases.NAME
WAVE = spectral.WAVENUMBER
_ID = lambda v: getattr(v, '__name__', None) or str(v)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_dataset(ds: xl.Dataset) -> xl.Dataset:
  """The same Dataset with its variables in HBM."""
  return xl.Dataset({k: xl.DataArray(_dev(v.values), v.dims)
                     for k, v in ds.items()}, ds.coords, ds.attrs)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64) if a.dtype == np.float64 else a


def _rows(ens, truth, lat):
  """(sums, cnt) host arrays of `engine.cross_spectrum_rows` on contiguous [M,
  O, R, C] members and [O, R, C] truth."""
  n_member, n_outer, n_row, n_col = ens.shape
  sums, cnt = engine.cross_spectrum_rows(
      _dev(ens), n_outer * n_row * n_col, n_member, None, _dev(truth), None,
      n_outer, n_row, n_col, snp.circumference(lat))
  assert sums.dtype == torch.float64 and cnt.dtype == torch.int32
  assert tuple(sums.shape) == (n_outer, n_row, 4, n_col // 2 + 1)
  assert tuple(cnt.shape) == (n_outer, n_row, 2)
  return sums.cpu().numpy(), cnt.cpu().numpy()


def _assert_rows(ens, truth, lat, msg):
  """The device rows within the stated bounds of the restatement, row by row;
  prints the worst share of the bound per term."""
  sums, cnt = _rows(ens, truth, lat)
  want, bad, cross_scale = snp.row_sums(ens, truth, lat)
  bound = snp.row_bounds(want, cross_scale, ens.dtype)
  err = np.abs(sums - want).max(axis=-1)                 # [O, R, 4]
  share = err / np.maximum(bound, 1e-300)
  print(msg, 'worst share of the bound per term',
        share.reshape(-1, 4).max(axis=0))
  assert (err <= bound).all(), (msg, share.reshape(-1, 4).max(axis=0))
  np.testing.assert_array_equal(cnt[..., 1], bad.astype(np.int32))
  np.testing.assert_array_equal(cnt[..., 0], (~bad).astype(np.int32))
  return sums, cnt


# ---------------------------------------------------------------------------
# 1. rows against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
@pytest.mark.parametrize('n_lon', [64, 96, 240, 1440])
def test_rows_are_within_the_bounds_of_the_restatement(n_lon, dtype):
  lat, _ = cases.grid(5, n_lon)  # the poles included
  for n_member in (1, 3):
    ens, truth = cases.arrays(n_member, 2, 5, n_lon, dtype, seed=n_lon)
    _assert_rows(ens, truth, lat, (n_lon, dtype.__name__, n_member))


@pytest.mark.parametrize('n_lon,dtype', [(3600, np.float64), (2560, np.float32)],
                         ids=_ID)
def test_the_long_rows_keep_their_sums_in_memory(n_lon, dtype):
  """3600 float64: the largest slabs, 2 waves per group.  Both lengths keep
  the member sums in the lane's own output elements (no registers left)."""
  lat, _ = cases.grid(3, n_lon)
  ens, truth = cases.arrays(2, 1, 3, n_lon, dtype, seed=7)
  _assert_rows(ens, truth, lat, (n_lon, dtype.__name__, 2))
  if n_lon == 3600:
    assert engine.cross_spectrum_geometry(torch.float64, 3600)[
        'waves_per_group'] == 2


def test_more_rows_than_the_launch_has_waves():
  """8 580 rows of 64 points (2.2 MB): more than 2048 workgroups of 4 waves,
  so waves take a second row; compared on every row."""
  n_lat, n_outer = 33, 260
  geo = engine.cross_spectrum_geometry(torch.float32, 64)
  assert n_lat * n_outer > geo['max_grid_outer'] * geo['waves_per_group']
  lat, _ = cases.grid(n_lat, 64)
  ens, truth = cases.arrays(1, n_outer, n_lat, 64, np.float32, seed=3)
  _assert_rows(ens, truth, lat, 'rows beyond the grid')


# ---------------------------------------------------------------------------
# 2. operands in place
# ---------------------------------------------------------------------------
def test_operands_are_read_where_they_lie():
  rs = np.random.RandomState(5)
  lat, lon = cases.grid(5, 64)
  coords = {'realization': np.arange(3),
            'time': np.array(['2020-01-01', '2020-01-02'], 'datetime64[ns]'),
            'prediction_timedelta': np.arange(6) * np.timedelta64(1, 'D'),
            'latitude': lat, 'longitude': lon}
  full = (rs.normal(size=(3, 2, 6, 5, 64)) + 3).astype(np.float32)
  tru = (rs.normal(size=(2, 5, 64)) + 3).astype(np.float32)
  dims = ('realization', 'time', 'prediction_timedelta', 'latitude',
          'longitude')
  lead = slice(1, 5)
  sub = dict(coords, prediction_timedelta=coords['prediction_timedelta'][lead])
  truth = xl.Dataset({'x': xl.DataArray(_dev(tru), dims[1:2] + dims[3:])},
                     sub)
  metric = spectral.CrossSpectrumTable()
  seen = []
  old = engine.cross_spectrum_rows

  def run(data, var_dims=dims):
    forecast = xl.Dataset({'x': xl.DataArray(data, var_dims)}, sub)
    engine.cross_spectrum_rows = lambda *a: (seen.append(a), old(*a))[1]
    try:
      return metric.compute_chunk(forecast, truth)
    finally:
      engine.cross_spectrum_rows = old

  def same(got, want):
    assert got['x'].dims == want['x'].dims
    np.testing.assert_array_equal(_bits(got['x'].values),
                                  _bits(want['x'].values))
  want = run(_dev(full[:, :, lead]))
  assert seen[-1][0].is_contiguous() and seen[-1][3] is None
  assert want['x'].dims == ('time', 'prediction_timedelta', 'term', WAVE)
  assert np.isfinite(want['x'].values).all()
  # a lead-sliced VIEW of the resident forecast
  view = _dev(full)[:, :, lead]
  assert not view.is_contiguous()
  same(run(view), want)
  assert seen[-1][0] is view and seen[-1][3] is not None
  # a SlabGather over a shuffled base, members at one stride
  order = np.random.RandomState(1).permutation(2 * 4)
  index = (np.arange(3)[:, None, None] * 8 + order.reshape(2, 4)[None])
  base = np.zeros((24, 5, 64), np.float32)
  base[index.reshape(-1)] = full[:, :, lead].reshape(-1, 5, 64)
  base_dev = _dev(base)
  same(run(xl.SlabGather(base_dev, index)), want)
  assert seen[-1][0] is base_dev and seen[-1][3] is not None
  # the ensemble dim not outermost: a contiguous (time, realization, lead)
  inner = np.ascontiguousarray(np.moveaxis(full[:, :, lead], 0, 1))
  same(run(_dev(inner), ('time', 'realization') + dims[2:]), want)
  assert seen[-1][1] == 4 * 5 * 64  # (the members are one lead block apart)
  # a permuted outer order: a (lead, realization, time) tensor seen as
  # (realization, time, lead) -- a view with whole slabs
  stored = _dev(np.ascontiguousarray(
      np.transpose(full[:, :, lead], (2, 0, 1, 3, 4))))
  turned = stored.permute(1, 2, 0, 3, 4)
  assert not turned.is_contiguous()
  same(run(turned), want)
  assert seen[-1][0] is turned and seen[-1][3] is not None
  # (lon, lat): one transposing copy, the same table
  got = run(_dev(np.swapaxes(full[:, :, lead], -1, -2)),
            dims[:3] + ('longitude', 'latitude'))
  same(got, want)
  # rows off the alignment of the kernel's loads: one contiguous copy
  buf = _dev(np.concatenate([[0.0], full[:, :, lead].reshape(-1)]
                            ).astype(np.float32))
  odd = buf[1:].view(3, 2, 4, 5, 64)
  assert odd.data_ptr() % 8 == 4
  same(run(odd), want)


# ---------------------------------------------------------------------------
# 3. invalid rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_rows_with_a_non_finite_value_are_zero_and_counted(dtype):
  n_lat, n_lon, n_member = 7, 96, 3
  lat, _ = cases.grid(n_lat, n_lon)
  ens, truth = cases.arrays(n_member, 2, n_lat, n_lon, dtype, seed=11)
  truth[0, 1, 0] = np.nan            # the first value a wave loads
  ens[-1, 0, 3, n_lon - 1] = np.nan  # the last member only, the last value
  ens[1, 1, 2, 17] = np.inf
  truth[1, 5, 40] = -np.inf
  sums, cnt = _assert_rows(ens, truth, lat, ('invalid', dtype.__name__))
  bad = np.zeros((2, n_lat), bool)
  bad[0, [1, 3]] = bad[1, [2, 5]] = True
  np.testing.assert_array_equal(cnt[..., 1].astype(bool), bad)
  # +0.0 in all four terms, bit for bit
  assert not _bits(sums[bad]).any()
  assert (sums[~bad][:, :2].sum(axis=-1) > 0).all()


def test_invalid_rows_in_the_public_path():
  n_lat, n_lon = 19, 64
  lat, lon = cases.grid(n_lat, n_lon)
  ens, truth = cases.arrays(3, 2, n_lat, n_lon, np.float32, seed=13)
  truth[0, 0, 5] = np.nan       # the south pole of time 0: not in the tropics
  ens[-1, 1, 9, 0] = np.nan     # the equator of time 1
  forecast, tru = cases.datasets(ens, truth)
  oregions = dict(cases.oracle_regions())
  from oracle import regions_np as oreg
  oregions['equator'] = oreg.SliceRegion(lat_slice=slice(-1, 1))
  regions = cases.product_regions(oregions)
  metric = spectral.CrossSpectrumTable()
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  for skipna in (False, True):
    got = metric.compute_chunk(f_dev, t_dev, skipna=skipna, regions=regions)
    dead = np.isnan(got[NAME].values).all(axis=(-1, -2))   # [region, time]
    some = np.isnan(got[NAME].values).any(axis=(-1, -2))
    np.testing.assert_array_equal(dead, some)
    names = list(regions)
    # the equator row is the whole region: NaN either way at time 1
    assert dead[names.index('equator')].tolist() == [False, True]
    # the pole's NaN does not reach the tropics
    assert dead[names.index('tropics')].tolist() == [False, not skipna]
    assert dead[names.index('global')].tolist() == [not skipna, not skipna]
    assert dead[names.index('southern-hemisphere')].tolist() == [
        not skipna, False]
    tol = snp.TOL[np.dtype(np.float32)]
    for r, (name, region) in enumerate(oregions.items()):
      w = _oracle_region_weights(region, lat, lon)
      want = snp.dense_table(ens, truth, lat, w, skipna)
      scale = snp.table_scale(np.nan_to_num(want))[..., None]
      err = np.abs(np.nan_to_num(got[NAME].values[r]) - np.nan_to_num(want))
      bound = scale * tol * np.array([1, 1, 2, 2])[:, None]
      assert (err <= bound).all(), (name, skipna)


# ---------------------------------------------------------------------------
# 4. the tie to K4f
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_lon,dtype', [
    (64, np.float32), (64, np.float64), (240, np.float32), (240, np.float64),
    (1440, np.float32), (1440, np.float64), (3600, np.float64)], ids=_ID)
def test_the_powers_are_those_of_the_zonal_spectrum_kernel(n_lon, dtype):
  """The transforms share their code and should share their bits; only the
  contraction of x x + y y could differ, by at most 4 u.  Measured when this
  was written: bit for bit in all seven cases (the printed line says which
  it is now)."""
  lat, _ = cases.grid(5, n_lon)
  ens, truth = cases.arrays(1, 2, 5, n_lon, dtype, seed=n_lon + 1)
  sums, _ = _rows(ens, truth, lat)
  circ = _dev(snp.circumference(lat))
  rel = 2.0 ** -22 if dtype is np.float32 else 2.0 ** -51
  equal = True
  for slot, x in ((0, ens[0]), (1, truth)):
    want = engine.zonal_spectrum(_dev(x), circ, 5).cpu().numpy()
    got = sums[:, :, slot]
    assert (np.abs(got - want) <= rel * np.abs(want)).all(), (
        slot, float((np.abs(got - want) / np.abs(want)).max()))
    equal = equal and np.array_equal(_bits(got), _bits(want))
  print(n_lon, dtype.__name__, 'bit for bit' if equal else 'NOT bit-equal')


# ---------------------------------------------------------------------------
# 5. identities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_a_forecast_equal_to_the_truth(dtype):
  lat, _ = cases.grid(5, 240)
  _, truth = cases.arrays(1, 2, 5, 240, dtype, seed=21)
  sums, _ = _rows(truth[None], truth, lat)
  pf, pt, co, qu = (sums[:, :, s] for s in range(4))
  u = 2.0 ** -24 if dtype is np.float32 else 2.0 ** -53
  np.testing.assert_array_equal(_bits(pf), _bits(pt))
  assert (np.abs(co - pf) <= 4 * u * pf).all()
  want, _, cross_scale = snp.row_sums(truth[None], truth, lat)
  bound = snp.row_bounds(want, cross_scale, dtype)
  assert (np.abs(qu).max(axis=-1) <= bound[..., 3]).all()
  err = np.abs(pf + pt - 2 * co).max(axis=-1)
  assert (err <= bound[..., 0] + bound[..., 1] + 2 * bound[..., 2]).all()


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_the_error_spectrum_is_the_spectrum_of_the_error(dtype):
  """error_spectrum(table) against ZonalEnergySpectrum of f - t, area-averaged
  (one member, global): within the four terms' bounds plus that spectrum's
  own tolerance.  The difference is formed in float64 and rounded to the row
  dtype once, which the float32 bound covers (u of the rows' scale)."""
  n_lat, n_lon = 9, 240
  ens, truth = cases.arrays(1, 2, n_lat, n_lon, dtype, seed=23)
  forecast, tru = cases.datasets(ens, truth, ensemble=False)
  table = spectral.CrossSpectrumTable().compute_chunk(
      _device_dataset(g(forecast)), _device_dataset(g(tru)))
  got = spectral.error_spectrum(table)[NAME]
  assert got.dims == ('time', WAVE)
  diff = (ens[0].astype(np.float64) - truth.astype(np.float64)).astype(dtype)
  lat, lon = cases.grid(n_lat, n_lon)
  ds = xl.Dataset({NAME: xl.DataArray(_dev(diff), cases.DIMS[1:])},
                  {'time': np.arange(2), 'latitude': lat, 'longitude': lon})
  want = dv.zonal_energy_spectrum_area_mean(ds, NAME).values
  tol = snp.TOL[np.dtype(dtype)]
  scale = snp.table_scale(table[NAME].values)             # [time, 4]
  bound = tol * (scale[:, 0] + scale[:, 1] + 2 * 2 * scale[:, 2] +
                 np.abs(want).sum(axis=-1))
  err = np.abs(got.values - want).max(axis=-1)
  print(dtype.__name__, 'share of the bound', err / bound)
  assert (err <= bound).all()


@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_the_phase_of_a_displaced_truth(dtype):
  """Three unit sinusoids (k = 1, 3, 7, no mean) displaced EASTWARD by s
  points: phase = -2 pi k s / N (mod 2 pi) within 3 sqrt(2) * 2 tol -- each
  bin holds a third of the row's cross scale, and an error e of a complex
  number z turns its angle by at most sqrt(2) e / |z| --, coherence 1 within
  the same order."""
  n_lat, n_lon, shift = 5, 64, 3
  lat, lon = cases.grid(n_lat, n_lon)
  j = np.arange(n_lon)
  row = sum(np.cos(2 * np.pi * k * j / n_lon + 0.3 * k) for k in (1, 3, 7))
  truth = np.broadcast_to(row, (1, n_lat, n_lon)).astype(dtype)
  ens = np.roll(truth, shift, axis=-1)[None]
  forecast, tru = cases.datasets(ens, truth, ensemble=False)
  table = spectral.CrossSpectrumTable().compute_chunk(
      _device_dataset(g(forecast)), _device_dataset(g(tru)))
  ks = np.array([1, 3, 7])
  tol = snp.TOL[np.dtype(dtype)]
  bound = 3 * np.sqrt(2) * 2 * tol
  got = spectral.phase(table)[NAME].values[0, ks]
  want = -2 * np.pi * ks * shift / n_lon
  turn = np.angle(np.exp(1j * (got - want)))
  assert (np.abs(turn) <= bound).all(), turn
  coh = spectral.coherence(table)[NAME].values[0, ks]
  assert (np.abs(coh - 1) <= 4 * bound).all(), coh
  assert float(spectral.amplitude_ratio(table)[NAME].values[0, 3]
               ) == pytest.approx(1.0, abs=4 * bound)


# ---------------------------------------------------------------------------
# 6. the fold
# ---------------------------------------------------------------------------
def test_fold_equals_the_host_fold_and_two_runs_are_bit_equal():
  n_lat, n_lon = 7, 96
  lat, _ = cases.grid(n_lat, n_lon)
  ens, truth = cases.arrays(3, 4, n_lat, n_lon, np.float32, seed=31)
  truth[2, 3, 9] = np.nan
  rs = np.random.RandomState(2)
  wrow = rs.rand(3, n_lat) * rs.randint(0, 3, size=(3, n_lat))
  runs = []
  for _ in range(2):
    sums, cnt = engine.cross_spectrum_rows(
        _dev(ens), truth.size, 3, None, _dev(truth), None, 4, n_lat, n_lon,
        snp.circumference(lat))
    table, counts = engine.cross_spectrum_fold(sums, cnt, wrow)
    assert tuple(table.shape) == (4, 3, 4, n_lon // 2 + 1)
    assert tuple(counts.shape) == (4, 3, 2)
    runs.append([x.cpu().numpy() for x in (sums, cnt, table, counts)])
  for a, b in zip(*runs):
    np.testing.assert_array_equal(_bits(a), _bits(b))
  sums, cnt, table, counts = runs[0]
  want_table, want_counts = spectral.host_fold(sums, cnt, wrow)
  np.testing.assert_array_equal(_bits(table), _bits(want_table))
  np.testing.assert_array_equal(_bits(counts), _bits(want_counts))


# ---------------------------------------------------------------------------
# 7. the public path
# ---------------------------------------------------------------------------
def test_compute_eval_and_the_area_mean_spectrum():
  from weatherbench2_amd import config, evaluation
  n_lat, n_lon = 9, 240
  lat, lon = cases.grid(n_lat, n_lon)
  ens, truth = cases.arrays(1, 3, n_lat, n_lon, np.float32, seed=41)
  forecast, tru = cases.datasets(ens, truth, ensemble=False)
  f_dev, t_dev = _device_dataset(g(forecast)), _device_dataset(g(tru))
  metric = spectral.CrossSpectrumTable()
  whole = metric.compute(f_dev, t_dev)
  assert whole[NAME].dims == ('term', WAVE)
  assert whole.attrs == {'ensemble_size': 1}
  chunks = metric.compute_chunk(f_dev, t_dev)[NAME].values
  np.testing.assert_allclose(whole[NAME].values, chunks.mean(axis=0),
                             rtol=1e-12, atol=0)
  every = helpers.predefined_regions(oracle=False)
  regions = {'global': every['global'], 'tropics': every['tropics']}
  cfg = config.Eval(metrics={'cross': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(f_dev, t_dev, cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims and da.dims[-2:] == ('term', WAVE)
  table = np.asarray(da.values).reshape(2, 3, 4, n_lon // 2 + 1)
  np.testing.assert_array_equal(
      _bits(table[0]), _bits(chunks))  # (the global region: the plain table)
  # the power terms of the global table: the area-mean spectrum
  for slot, ds in ((0, f_dev), (1, t_dev)):
    want = dv.zonal_energy_spectrum_area_mean(ds, NAME).values
    np.testing.assert_allclose(table[0][:, slot], want, rtol=1e-12,
                               atol=1e-12 * np.abs(want).max())
