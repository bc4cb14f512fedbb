"""Scale-dependent verification on the host: the NumPy path of
weatherbench2_amd/spectral.py against the dense restatement
(tests/cross_spectrum_np.py), the scores on hand-made tables, the bootstrap,
the refusals, the C ABI of K25 (csrc/cross_spectrum.hip) up to, not including,
a launch, and the per-lane code of the kernel run on the CPU
(tools/cross_fft_host_check.hip)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import cross_spectrum_cases as cases
from tests import cross_spectrum_np as snp
from tests import helpers
from tests.test_cabi_cpu import _oracle_region_weights
from weatherbench2_amd import bootstrap as bs
from weatherbench2_amd import engine
from weatherbench2_amd import regions as greg
from weatherbench2_amd import spectral
from weatherbench2_amd import xarray_lite as xl

g = helpers.to_gpu_dataset
NAME = cases.NAME
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda v: getattr(v, '__name__', None) or str(v)
WAVE = spectral.WAVENUMBER


# ---------------------------------------------------------------------------
# 1. the host path against the restatement
# ---------------------------------------------------------------------------
def _assert_table(got, want, msg):
  """Row-relative error < 1e-12 (the project's float64 spectrum tolerance)."""
  assert got.shape == want.shape, msg
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
  scale = snp.table_scale(np.nan_to_num(want))[..., None]
  err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
  assert (err <= 1e-12 * scale).all(), (msg, float((err / np.maximum(
      scale, 1e-300)).max()))


@pytest.mark.parametrize('n_member', [1, 3])
@pytest.mark.parametrize('dtype', cases.DTYPES, ids=_ID)
def test_host_table_equals_the_dense_restatement(dtype, n_member):
  n_time, n_lat, n_lon = 2, 19, 64
  ens, truth = cases.arrays(n_member, n_time, n_lat, n_lon, dtype, seed=1)
  lat, lon = cases.grid(n_lat, n_lon)
  # an invalid row in a tropical row of time 0 (NaN in the last member) and
  # one at the south pole of time 1 (+inf in the truth)
  ens[-1, 0, 9, 5] = np.nan
  truth[1, 0, 63] = np.inf
  forecast, tru = cases.datasets(ens, truth, ensemble=n_member > 1)
  metric = spectral.CrossSpectrumTable()
  for oregions in (None, cases.oracle_regions(), cases.overlap_regions()):
    for skipna in (False, True):
      if oregions is None:
        got = metric.compute_chunk(g(forecast), g(tru), skipna=skipna)
        names, front = {'global': None}, ()
      else:
        got = metric.compute_chunk(g(forecast), g(tru), skipna=skipna,
                                   regions=cases.product_regions(oregions))
        names, front = oregions, ('region',)
        assert list(got.coords['region']) == list(oregions)
      da = got[NAME]
      assert da.dims == front + ('time', 'term', WAVE)
      assert da.values.dtype == np.float64
      assert list(got.coords['term']) == list(spectral.TERMS)
      np.testing.assert_array_equal(got.coords[WAVE],
                                    np.arange(n_lon // 2 + 1))
      assert np.asarray(got.coords[WAVE]).dtype == np.int64
      assert got.attrs == {'ensemble_size': n_member}
      for r, (name, region) in enumerate(names.items()):
        w = _oracle_region_weights(region, lat, lon)
        want = snp.dense_table(ens, truth, lat, w, skipna)
        mine = da.values[r] if front else da.values
        _assert_table(mine, want, (name, skipna))
      # the cells that hold an invalid row
      values = da.values[0] if front else da.values
      assert np.isnan(values).all(axis=(-1, -2)).tolist() == [
          not skipna, not skipna]


def test_a_region_without_the_invalid_rows_is_not_reached_by_them():
  ens, truth = cases.arrays(1, 1, 19, 64, np.float32, seed=2)
  truth[0, 9, 3] = np.nan  # the equator
  forecast, tru = cases.datasets(ens, truth, ensemble=False)
  regions = cases.product_regions(cases.oracle_regions())
  got = spectral.CrossSpectrumTable().compute_chunk(
      g(forecast), g(tru), regions=regions)[NAME].values
  dead = np.isnan(got).all(axis=(1, 2, 3))
  assert dead.tolist() == [True, True, False, False]
  assert not np.isnan(got[2:]).any()


# ---------------------------------------------------------------------------
# 2. the scores on hand-made tables
# ---------------------------------------------------------------------------
def _table(pf, pt, co, qu, lead=()):
  p = np.stack([np.asarray(v, np.float64) for v in (pf, pt, co, qu)], axis=-2)
  return xl.DataArray(p, tuple(lead) + ('term', WAVE), {}, NAME)


def test_scores_and_their_zero_over_zero_rules():
  pf = [4.0, 1.0, 0.0, 0.0, 9.0]
  pt = [1.0, 4.0, 0.0, 2.0, 0.0]
  co = [1.0, -2.0, 0.0, 0.0, 0.0]
  qu = [0.0, 0.0, 0.0, 0.0, 0.0]
  t = _table(pf, pt, co, qu)
  coh = spectral.coherence(t)
  assert coh.dims == (WAVE,)
  np.testing.assert_array_equal(coh.values[:2], [0.25, 1.0])
  assert np.isnan(coh.values[2:]).all()  # 0/0, and 0/0 again with one power 0
  cor = spectral.spectral_correlation(t).values
  np.testing.assert_array_equal(cor[:2], [0.5, -1.0])
  assert np.isnan(cor[2:]).all()
  amp = spectral.amplitude_ratio(t).values
  np.testing.assert_array_equal(amp[[0, 1, 3]], [2.0, 0.5, 0.0])
  assert np.isnan(amp[2]) and np.isinf(amp[4])
  ph = spectral.phase(t).values
  np.testing.assert_array_equal(ph[:2], [0.0, np.pi])
  assert np.isnan(ph[2:]).all()
  assert spectral.phase(_table([1], [1], [0.0], [-1.0])).values[0] == -np.pi / 2
  err = spectral.error_spectrum(t).values
  np.testing.assert_array_equal(
      err, np.array(pf) + np.array(pt) - 2 * np.array(co))
  with pytest.raises(ValueError, match='not a cross-spectrum table'):
    spectral.coherence(xl.DataArray(np.zeros((3, 5)), ('term', WAVE)))


def test_effective_resolution():
  one = np.ones(6)
  def res(coherence, **kwargs):
    c = np.asarray(coherence, np.float64)
    out = spectral.effective_resolution(_table(one, one, np.sqrt(c), 0 * c),
                                        **kwargs)
    assert out.values.dtype == np.float64
    return float(out.values)
  # sqrt and squaring round: levels away from the values
  assert res([0.1, 0.9, 0.8, 0.7, 0.2, 0.9]) == 3.0   # the run ends at k = 3
  assert res([0.0, 0.9, 0.8, 0.7, 0.6, 0.9]) == 5.0   # it never ends
  assert res([1.0, 0.2, 0.9, 0.9, 0.9, 0.9]) == 0.0   # failure at k = 1
  assert res([1.0, 0.9, np.nan, 0.9, 0.9, 0.9]) == 1.0  # a NaN ends the run
  assert res([0.1, 0.9, 0.8, 0.7, 0.2, 0.9], level=0.75) == 2.0
  co = np.array([1.0, 0.9, -0.8, 0.9, 0.9, 0.9])
  t = _table(one, one, co, 0 * co)
  assert float(spectral.effective_resolution(
      t, score=spectral.spectral_correlation).values) == 1.0
  assert float(spectral.effective_resolution(t).values) == 5.0


def test_leading_dims_and_datasets_are_kept():
  rs = np.random.RandomState(0)
  p = rs.rand(7, 2, 4, 9)
  da = xl.DataArray(p, (bs.REPLICATE, 'time', 'term', WAVE),
                    {'time': np.arange(2)}, NAME)
  ds = xl.Dataset({NAME: da, 'other': da}, {'time': np.arange(2)})
  for fn in (spectral.coherence, spectral.spectral_correlation,
             spectral.amplitude_ratio, spectral.phase,
             spectral.error_spectrum):
    out = fn(da)
    assert out.dims == (bs.REPLICATE, 'time', WAVE) and out.shape == (7, 2, 9)
    both = fn(ds)
    assert set(both.keys()) == {NAME, 'other'}
    np.testing.assert_array_equal(both['other'].values, out.values)
  res = spectral.effective_resolution(ds)
  assert res[NAME].dims == (bs.REPLICATE, 'time')
  assert 'coherence of a SINGLE' in spectral.coherence.__doc__


# ---------------------------------------------------------------------------
# 3. bootstrap, compute, Eval
# ---------------------------------------------------------------------------
def _per_time_tables(n_member=3, n_time=6):
  ens, truth = cases.arrays(n_member, n_time, 5, 64, np.float64, seed=5)
  forecast, tru = cases.datasets(ens, truth)
  return forecast, tru, spectral.CrossSpectrumTable().compute_chunk(
      g(forecast), g(tru))


def test_bootstrap_returns_the_five_fields_per_score():
  _, _, tables = _per_time_tables()
  assert tables[NAME].dims == ('time', 'term', WAVE)
  out = bs.bootstrap(tables, spectral.coherence, n_replicate=20,
                     block_length=2, seed=1)
  for field in ('', '_lower', '_upper', '_standard_error',
                '_valid_replicates'):
    assert out[NAME + field].dims == (WAVE,), field
    assert out[NAME + field].shape == (33,)
  assert (out[NAME + '_lower'].values <= out[NAME + '_upper'].values).all()
  whole = spectral.coherence(tables.mean('time'))[NAME].values
  np.testing.assert_allclose(out[NAME].values, whole, rtol=1e-12)
  assert ((whole > 0) & (whole <= 1 + 1e-12)).all()


def test_compute_is_the_time_mean_and_eval_takes_the_generic_path():
  from weatherbench2_amd import config, evaluation
  forecast, tru, tables = _per_time_tables(n_time=3)
  metric = spectral.CrossSpectrumTable()
  whole = metric.compute(g(forecast), g(tru))
  assert whole[NAME].dims == ('term', WAVE)
  assert whole.attrs == {'ensemble_size': 3}
  np.testing.assert_allclose(whole[NAME].values,
                             tables[NAME].values.mean(axis=0), rtol=1e-12)
  regions = cases.product_regions(cases.oracle_regions())
  every = metric.compute_chunk(g(forecast), g(tru), regions=regions)
  fan = metric.compute_chunk_regions(g(forecast), g(tru), regions)
  np.testing.assert_array_equal(fan[NAME].values, every[NAME].values)
  mean = metric.compute_regions(g(forecast), g(tru), regions)
  assert mean[NAME].dims == ('region', 'term', WAVE)
  assert metric._fused_regions and not metric._reads_slabs_in_place
  cfg = config.Eval(metrics={'cross': metric}, regions=regions)
  loop = evaluation._metric_and_region_loop(g(forecast), g(tru), cfg, False,
                                            compute_chunk=True)
  da = loop[NAME]
  assert 'region' in da.dims and da.dims[-2:] == ('term', WAVE)
  np.testing.assert_array_equal(
      np.asarray(da.values).reshape(every[NAME].shape), every[NAME].values)


# ---------------------------------------------------------------------------
# 4. the refusals
# ---------------------------------------------------------------------------
def _refuses(call, match):
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))
  try:
    with pytest.raises(ValueError, match=match):
      call()
  finally:
    engine.set_launch_hook(old)
  assert not calls


def test_refusals_come_before_any_launch():
  metric = spectral.CrossSpectrumTable()
  ens, truth = cases.arrays(3, 1, 5, 64, np.float32)
  forecast, tru = cases.datasets(ens, truth)
  run = lambda f, t_, **kw: metric.compute_chunk(g(f), g(t_), **kw)
  # a row length without a kernel
  odd = cases.datasets(*cases.arrays(3, 1, 5, 72, np.float32))
  _refuses(lambda: run(*odd), '72 longitudes.*64, 96')
  # a regional and a non-uniform longitude axis
  for lon in (np.linspace(0.0, 180.0, 64, endpoint=False),
              np.concatenate([np.arange(63.0) * 5.625, [359.0]])):
    bad = [ds.__class__(dict(ds.items()), dict(ds.coords, longitude=lon))
           for ds in (forecast, tru)]
    _refuses(lambda: run(*bad), 'not cyclic')
  for dtype in (np.float16, np.int32):
    _refuses(lambda: run(*cases.datasets(ens.astype(dtype), truth)),
             'float32 and float64')
    _refuses(lambda: run(*cases.datasets(ens, truth.astype(dtype))),
             'float32 and float64')
  big = cases.datasets(*cases.arrays(129, 1, 5, 64, np.float32))
  _refuses(lambda: run(*big), '129 members.*1 to 128')
  none = cases.datasets(np.zeros((0, 1, 5, 64), np.float32), truth)
  _refuses(lambda: run(*none), '0 members.*1 to 128')
  # variables that differ in ensemble size
  f, t_ = g(forecast), g(tru)
  two_f = xl.Dataset({NAME: f[NAME], 'other': f[NAME].isel(
      realization=slice(0, 2))}, {k: v for k, v in f.coords.items()
                                  if k != 'realization'})
  two_t = xl.Dataset({NAME: t_[NAME], 'other': t_[NAME]}, t_.coords)
  _refuses(lambda: metric.compute_chunk(two_f, two_t), 'differ in ensemble')
  # regions whose weights are no row weight times one constant
  every = helpers.predefined_regions(oracle=False)
  _refuses(lambda: run(forecast, tru, regions={
      'global': every['global'], 'europe': every['europe']}),
           "'europe'.*column multiplicity")
  _refuses(lambda: run(forecast, tru, region=greg.SliceRegion(
      lon_slice=slice(0, 90))), 'column multiplicity')
  lat, lon = cases.grid(5, 64)
  lsm = xl.DataArray(np.ones((5, 64)), ('latitude', 'longitude'),
                     {'latitude': lat, 'longitude': lon})
  _refuses(lambda: run(forecast, tru, regions={
      'the-land': greg.LandRegion(lsm)}), 'the-land.*LandRegion.*2-D')
  # 128 members are taken
  most = cases.datasets(*cases.arrays(128, 1, 3, 64, np.float32))
  assert run(*most).attrs['ensemble_size'] == 128


# ---------------------------------------------------------------------------
# 5. the built library without a GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_both_symbols_are_exported_and_declared(lib):
  h = lib.load()
  header = open(os.path.join(ROOT, 'include', 'wb2hip.h')).read()
  for name in ('wb2_cross_spectrum_rows', 'wb2_cross_spectrum_geometry'):
    assert getattr(h, name) is not None
    assert re.search(r'^int %s\(' % name, header, re.M), name
  assert 'K25' in header and 'displaced EASTWARD' in header


def test_entry_point_refuses_in_the_stated_order(lib):
  h = lib.load()
  buf = np.zeros(256, dtype=np.int64)  # (zeros: also a plan without tables)
  b = buf.ctypes.data
  good = dict(plan=b, dtype=lib.WB2_F32, ens=b, truth=b, n_member=3, stride=64,
              n_outer=2, n_row=2, n_col=64, circ=b, sums=b, cnt=b)

  def rows(**kwargs):
    a = dict(good, **kwargs)
    return h.wb2_cross_spectrum_rows(
        a['plan'], a['dtype'], a['ens'], None, a['truth'], None, a['n_member'],
        a['stride'], a['n_outer'], a['n_row'], a['n_col'], a['circ'],
        a['sums'], a['cnt'], None)
  # each refusal, with every LATER check failing as well: the order
  steps = [(dict(dtype=7), b'unknown dtype'),
           (dict(n_col=100), b'not instantiated'),
           (dict(n_member=129), b'n_member='),
           (dict(stride=-2), b'member_stride='),
           (dict(n_row=-1), b'negative'),
           (dict(ens=b + 4), b'aligned'),
           (dict(sums=None), b'null pointer'),
           (dict(n_outer=1 << 41), b'the grid does not fit'),
           (dict(), b'the plan')]
  for first in range(len(steps)):
    bad = {}
    for kwargs, _ in steps[first:]:
      bad.update(kwargs)
    assert rows(**bad) < 0
    assert steps[first][1] in h.wb2_last_error(), (first, h.wb2_last_error())
  assert b' 64 128 240 ' in (rows(n_col=100), h.wb2_last_error())[1]
  for kwargs, words in ((dict(n_member=0), b'n_member='),
                        (dict(n_col=63), b'not instantiated'),
                        (dict(n_outer=-1), b'negative'),
                        (dict(truth=b + 4), b'aligned'),
                        (dict(stride=63), b'aligned'),
                        (dict(dtype=lib.WB2_F64, ens=b + 8), b'aligned'),
                        (dict(plan=None), b'null pointer'),
                        (dict(ens=None), b'null pointer'),
                        (dict(truth=None), b'null pointer'),
                        (dict(circ=None), b'null pointer'),
                        (dict(cnt=None), b'null pointer')):
    assert rows(**kwargs) < 0 and words in h.wb2_last_error(), kwargs
  for empty in (dict(n_outer=0), dict(n_row=0)):
    assert rows(ens=None, plan=None, **empty) == 0


def test_geometry_reports_the_lengths_the_waves_and_the_lds(lib):
  for dtype in (torch.float32, torch.float64):
    taken = [n for n in range(1, 4097) if engine.cross_spectrum_geometry(
        dtype, n)['supported']]
    assert taken == sorted(spectral.ROW_LENGTHS) and len(taken) == 22
  # K4f's own list (read from its source): the same lengths
  from tests import spectrum_geometry_cases
  assert sorted(spectrum_geometry_cases.FUSED_N_LON) == sorted(
      spectral.ROW_LENGTHS)
  # complex size * ((N / 4 + 2) + waves * 2 * slab slots): include/wb2hip.h
  for dtype, n_col, waves, lds in (
      (torch.float32, 64, 4, 8 * (18 + 4 * 2 * 32)),
      (torch.float32, 1440, 4, 8 * (362 + 4 * 2 * 840)),
      (torch.float64, 3600, 2, 16 * (902 + 2 * 2 * 1800))):
    geo = engine.cross_spectrum_geometry(dtype, n_col, 50)
    assert geo['supported'] == 1 and geo['waves_per_group'] == waves
    assert geo['lds_bytes'] == lds <= 160 * 1024
    assert geo['max_grid_outer'] > 0
  assert 16 * (902 + 4 * 2 * 1800) > 160 * 1024  # (why float64 3600 gets 2)
  none = engine.cross_spectrum_geometry(torch.float32, 100)
  assert (none['supported'], none['waves_per_group'], none['lds_bytes']) == (
      0, 0, 0)
  for n_member in (0, 129):
    with pytest.raises(lib.Wb2HipError, match='n_member='):
      engine.cross_spectrum_geometry(torch.float32, 64, n_member)


def test_engine_refuses_on_the_host(lib):
  ens, truth = cases.arrays(3, 2, 3, 64, np.float32)
  e, y = torch.from_numpy(ens), torch.from_numpy(truth)
  circ = np.ones(3)
  slab = 3 * 64
  calls = []
  old = engine.set_launch_hook(lambda *a: calls.append(a))

  def rows(ens=e, stride=2 * slab, n_member=3, ens_slab=None, truth=y,
           n_outer=2, n_col=64, circ=circ):
    return engine.cross_spectrum_rows(ens, stride, n_member, ens_slab, truth,
                                      None, n_outer, 3, n_col, circ)
  try:
    for kwargs, error, match in (
        (dict(n_col=72), ValueError, 'n_col=72'),
        (dict(n_member=0), ValueError, '0 members'),
        (dict(n_member=129), ValueError, '129 members'),
        (dict(circ=np.ones(4)), ValueError, 'circumference'),
        (dict(ens_slab=np.arange(2) + 1), IndexError, 'member slabs'),
        (dict(truth=y[:1].clone()), IndexError, 'truth slabs'),
        (dict(stride=-2), ValueError, 'bad sizes'),
        (dict(truth=y.double()), TypeError, 'dtype')):
      with pytest.raises(error, match=match):
        rows(**kwargs)
      assert not calls, kwargs
  finally:
    engine.set_launch_hook(old)
  with pytest.raises(ValueError, match='sums must be'):
    engine.cross_spectrum_fold(torch.zeros(1, 2, 3, 5, dtype=torch.float64),
                               torch.zeros(1, 2, 2, dtype=torch.int32),
                               np.ones((1, 2)))
  with pytest.raises(ValueError, match='wrow'):
    engine.cross_spectrum_fold(torch.zeros(1, 2, 4, 5, dtype=torch.float64),
                               torch.zeros(1, 2, 2, dtype=torch.int32),
                               np.ones((1, 3)))


# ---------------------------------------------------------------------------
# 6. the per-lane code of the kernel on the CPU
# ---------------------------------------------------------------------------
def _hipcc():
  for cand in ('/opt/rocm/bin/hipcc', shutil.which('hipcc')):
    if cand and os.path.exists(cand):
      return cand
  return None


@pytest.mark.skipif(_hipcc() is None, reason='hipcc not installed')
def test_host_emulation_of_the_transforms_and_the_new_recombination(tmp_path):
  """Every plan length in float32 against a float64 DFT.  The bounds of the
  GPU tests (tests/cross_spectrum_np.py) with a factor 2 to spare: 1e-6 for
  the powers, 2e-6 for the cospectrum and the quadrature.  Worst values when
  this was written: pf 1.7e-7, pt 2.1e-7, co 1.2e-7, qu 2.4e-9."""
  exe = str(tmp_path / 'cross_fft_host_check')
  subprocess.run(
      [_hipcc(), '--cuda-host-only', '-O2', '-std=c++17',
       '-I' + os.path.join(ROOT, 'weatherbench2_amd', 'csrc'),
       os.path.join(ROOT, 'tools', 'cross_fft_host_check.hip'), '-o', exe],
      check=True, cwd=str(tmp_path))
  out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
  print(out)
  lines = [l.split() for l in out.strip().splitlines()]
  sizes = {int(l[1]): [float(l[3]), float(l[5]), float(l[7]), float(l[9])]
           for l in lines if l[0] == 'N'}
  assert set(sizes) == set(spectral.ROW_LENGTHS)
  tol = snp.TOL[np.dtype(np.float32)]
  for n, (pf, pt, co, qu) in sizes.items():
    assert max(pf, pt) < tol / 2, (n, pf, pt)
    assert max(co, qu) < 2 * tol / 2, (n, co, qu)
