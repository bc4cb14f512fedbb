"""`deterministic_spatial` chunk by chunk (weatherbench2_amd/map_suite.py): the
three map metrics of every variable of a chunk through ONE fused launch into
the running temporal mean must leave the bits of the generic path (maps ->
metric concat -> wb2_time_accumulate), which equal the oracle's time mean of
the per-chunk maps.  Reference: scripts/evaluate.py:431-435, 471-478;
metrics.py:304-374; evaluation.py:583-599, 735-744."""
import numpy as np
import pytest

from tests import helpers, official_chunks as oc

pytestmark = pytest.mark.gpu


def _setup(metric_names=('bias', 'mse', 'mae'), **kw):
  from weatherbench2_amd import config, evaluation, metrics as gm
  forecast, truth, clim = oc.make(**kw)
  gf, gt = (evaluation.make_resident(helpers.to_gpu_dataset(x))
            for x in (forecast, truth))
  every = {'bias': gm.SpatialBias(), 'mse': gm.SpatialMSE(),
           'mae': gm.SpatialMAE()}
  cfg = config.Eval(metrics={k: every[k] for k in metric_names})
  return forecast, truth, gf, gt, cfg


def _same(a, b):
  assert sorted(a.data_vars) == sorted(b.data_vars)
  for k in a.coords:
    ca, cb = a.coords[k], b.coords[k]
    np.testing.assert_array_equal(np.asarray(getattr(ca, 'values', ca)),
                                  np.asarray(getattr(cb, 'values', cb)))
  for name in a.data_vars:
    x, y = np.asarray(a[name].values), np.asarray(b[name].values)
    assert a[name].dims == b[name].dims and x.dtype == y.dtype
    assert np.array_equal(x, y, equal_nan=True), name


def _count_runs(monkeypatch):
  from weatherbench2_amd import map_suite
  calls = []
  real = map_suite.MapSuite.run

  def run(self, *a, **k):
    calls.append(1)
    return real(self, *a, **k)
  monkeypatch.setattr(map_suite.MapSuite, 'run', run)
  return calls


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('batch', [1, 2, None])
@pytest.mark.parametrize('order', ['init', 'lead'])
def test_fused_maps_give_the_generic_paths_bits(order, batch, skipna,
                                                monkeypatch):
  from weatherbench2_amd import evaluation
  forecast, truth, gf, gt, cfg = _setup(n_init=5, n_lead=3, n_lat=19,
                                        n_lon=36, nan_frac=0.02)
  chunks = oc.chunk_pairs(gf, gt, order=order)
  kwargs = {} if batch is None else {'batch_chunks': batch}
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                    batch_chunks=1)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  calls = _count_runs(monkeypatch)
  got = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0, **kwargs)
  _same(got, want)
  if batch == 1:
    assert len(calls) == len(chunks) - 1
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', 'verify')
  _same(evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0, **kwargs),
        want)
  # against the oracle: the time mean of the per-chunk maps
  from oracle import metrics_np as om
  kinds = {'bias': om.SpatialBias(), 'mse': om.SpatialMSE(),
           'mae': om.SpatialMAE()}
  labels = list(got.coords['metric'])
  for mname, metric in kinds.items():
    with np.errstate(all='ignore'):
      per = metric.compute_chunk(forecast, truth)
    for name, var in per.items():
      ax = var.dims.index('init_time')
      data = np.asarray(var.data, dtype=np.float64)
      with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
          warnings.simplefilter('ignore')
          mean = (np.nanmean if skipna else np.mean)(data, axis=ax)
      dims = tuple(d for d in var.dims if d != 'init_time')
      res = got[name]
      rdims = [d for d in res.dims if d != 'metric']
      vals = res.values[labels.index(mname)]
      vals = np.transpose(vals, [rdims.index(d) for d in dims])
      helpers.assert_close(vals, mean, rtol=1e-6, atol=1e-7,
                           err_msg=f'{mname}/{name}')


def test_a_subset_of_the_maps_in_another_order(monkeypatch):
  """Only (mae, bias): the kernel skips the sum it has no destination for."""
  from weatherbench2_amd import evaluation
  _, _, gf, gt, cfg = _setup(('mae', 'bias'), n_init=4, n_lead=2, n_lat=19,
                             n_lon=36)
  chunks = oc.chunk_pairs(gf, gt)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                    batch_chunks=1)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  calls = _count_runs(monkeypatch)
  got = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                   batch_chunks=1)
  _same(got, want)
  assert len(calls) == len(chunks) - 1
  assert sorted(got.coords['metric']) == ['bias', 'mae']


def test_float64_inputs_and_the_unaligned_layout(monkeypatch):
  """float64 chunks on 19 x 36 (684 points, 5 472-byte slabs: an even point
  count on 16-byte slabs, so the suite's launch takes the two-wide vector
  path) and on 19 x 37 (703 points, 5 624 bytes: the scalar path), and
  float32 on 19 x 37 (2 812 bytes: the scalar path too)."""
  from weatherbench2_amd import _lib, evaluation
  lib = _lib.load()
  real = lib.wb2_spatial_accumulate_addr
  aligned = []

  def spy(*args):
    aligned.append(args[2])
    return real(*args)
  monkeypatch.setattr(lib, 'wb2_spatial_accumulate_addr', spy)
  for dtype, n_lon, vector in ((np.float64, 36, 1), (np.float64, 37, 0),
                               (np.float32, 37, 0)):
    _, _, gf, gt, cfg = _setup(n_init=3, n_lead=2, n_lat=19, n_lon=n_lon,
                               dtype=dtype)
    chunks = oc.chunk_pairs(gf, gt)
    monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
    want = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                      batch_chunks=1)
    monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
    calls = _count_runs(monkeypatch)
    del aligned[:]
    got = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                     batch_chunks=2)
    _same(got, want)
    assert calls
    assert aligned and set(aligned) == {vector}, (dtype, n_lon, aligned)


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('order', ['init', 'lead'])
def test_with_the_spatial_seeps_pair_of_compute_seeps(order, skipna,
                                                      monkeypatch):
  """`--compute_seeps=True` adds two SpatialSEEPS entries to the config
  (scripts/evaluate.py:446-457): maps of their precipitation variable only,
  NaN for every other variable in the merged result.  The suite fuses the three
  map metrics, lets SpatialSEEPS compute its own map and accumulates it slab by
  slab; rows of new lead labels get their NaN fills -- the generic path's bits,
  and the oracle's SpatialSEEPS time mean."""
  import warnings
  from oracle import metrics_np as om
  from oracle.named import DS, NA
  from weatherbench2_amd import config, evaluation, metrics as gm
  forecast, truth, clim = oc.make(n_init=4, n_lead=3, n_lat=19, n_lon=36)
  rs = np.random.RandomState(5)
  names = ('2m_temperature', '10m_u_component_of_wind')
  cvars = dict(clim.items())
  for name in names:
    shape, cdims = clim[name].data.shape, clim[name].dims
    cvars[f'{name}_seeps_threshold'] = NA(
        rs.uniform(0.3, 1.2, size=shape).astype(np.float32), cdims)
    frac = rs.uniform(0.0, 1.0, size=shape).astype(np.float32)
    frac[:, :, 3, 5] = np.nan
    cvars[f'{name}_seeps_dry_fraction'] = NA(frac, cdims)
  clim = DS(cvars, clim.coords)
  gf, gt, gc = (evaluation.make_resident(helpers.to_gpu_dataset(x))
                for x in (forecast, truth, clim))
  metrics = {'bias': gm.SpatialBias(), 'mse': gm.SpatialMSE(),
             'mae': gm.SpatialMAE()}
  for key, name in zip(('seeps_a', 'seeps_b'), names):
    metrics[key] = gm.SpatialSEEPS(climatology=gc, precip_name=name,
                                   dry_threshold_mm=100.0)
  cfg = config.Eval(metrics=metrics)
  chunks = oc.chunk_pairs(gf, gt, order=order)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                    batch_chunks=1)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  calls = _count_runs(monkeypatch)
  got = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                   batch_chunks=1)
  _same(got, want)
  assert len(calls) == len(chunks) - 1
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', 'verify')
  _same(evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                   batch_chunks=1), want)
  # in windows the SEEPS maps of the k chunks of a lead label are ONE
  # wb2_seeps_map_addr launch + one accumulate of k steps: the same bits
  from weatherbench2_amd import map_suite
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  many = []
  real_many = map_suite._FastSeeps.run_many
  monkeypatch.setattr(
      map_suite._FastSeeps, 'run_many',
      lambda self, pairs, mean: (many.append(len(pairs)),
                                 real_many(self, pairs, mean))[1])
  for kwargs in ({'batch_chunks': 6}, {}):
    _same(evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                     **kwargs), want)
  assert many and max(many) > 1, many
  labels = list(got.coords['metric'])
  # every other variable is NaN under the SEEPS labels
  assert np.isnan(got['geopotential'].values[labels.index('seeps_a')]).all()
  assert np.isnan(got[names[1]].values[labels.index('seeps_a')]).all()
  assert np.isfinite(got['geopotential'].values[labels.index('mse')]).all()
  for key, name in zip(('seeps_a', 'seeps_b'), names):
    oseeps = om.SpatialSEEPS(climatology=clim, precip_name=name,
                             dry_threshold_mm=100.0)
    with np.errstate(all='ignore'):
      per = oseeps.compute_chunk(forecast, truth)[name]
    ax = per.dims.index('init_time')
    data = np.asarray(per.data, dtype=np.float64)
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      mean = (np.nanmean if skipna else np.mean)(data, axis=ax)
    dims = tuple(d for d in per.dims if d != 'init_time')
    res = got[name]
    rdims = [d for d in res.dims if d != 'metric']
    vals = np.transpose(res.values[labels.index(key)],
                        [rdims.index(d) for d in dims])
    helpers.assert_close(vals, mean, rtol=1e-9, atol=1e-12, err_msg=key)


def test_later_chunks_reuse_the_first_chunks_offsets(monkeypatch):
  """Device-resident chunks of one structure: the slab offsets and destination
  offsets are worked out once (MapSuite._first), later chunks add their base
  pointers; host chunks (copied per chunk) take the long way every time --
  same bits either way."""
  from weatherbench2_amd import evaluation, map_suite
  _, _, gf, gt, cfg = _setup(n_init=4, n_lead=3, n_lat=19, n_lon=36)
  chunks = oc.chunk_pairs(gf, gt, order='lead')
  firsts = []
  real = map_suite.MapSuite._first

  def first(self, *a, **k):
    firsts.append(1)
    return real(self, *a, **k)
  monkeypatch.setattr(map_suite.MapSuite, '_first', first)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  calls = _count_runs(monkeypatch)
  got = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                   batch_chunks=1)
  assert len(calls) == len(chunks) - 1 and len(firsts) == 1
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = evaluation.evaluate_chunks(chunks, cfg, False, prefetch=0,
                                    batch_chunks=1)
  _same(got, want)


def test_other_configs_keep_the_generic_path(monkeypatch):
  """Regions, a fourth metric or temporal_mean=False: not this suite's."""
  import dataclasses
  from weatherbench2_amd import map_suite, metrics as gm, regions as gr
  _, _, gf, gt, cfg = _setup(n_init=2, n_lead=1)
  assert map_suite.applies(cfg)
  assert not map_suite.applies(dataclasses.replace(cfg, temporal_mean=False))
  assert not map_suite.applies(dataclasses.replace(
      cfg, regions={'global': gr.SliceRegion()}))
  more = dict(cfg.metrics)
  more['mse_scalar'] = gm.MSE()
  assert not map_suite.applies(dataclasses.replace(cfg, metrics=more))
  assert map_suite.applies(dataclasses.replace(cfg, metrics={
      **cfg.metrics, 'seeps': gm.SpatialSEEPS(climatology=None)}))
  assert not map_suite.applies(dataclasses.replace(cfg, metrics={
      'seeps': gm.SpatialSEEPS(climatology=None)}))
  twice = dict(cfg.metrics)
  twice['mse_again'] = gm.SpatialMSE()
  assert not map_suite.applies(dataclasses.replace(cfg, metrics=twice))


def test_large_map_results_use_one_table_entry_per_run():
  """RunningMean with a split dim and map-valued results: the destination
  table has one entry per run behind the split dim, and the accumulation
  equals the per-element table's."""
  import torch
  from weatherbench2_amd import evaluation
  from weatherbench2_amd import xarray_lite as xl
  dev = torch.device('cuda')
  gen = torch.Generator(device=dev).manual_seed(3)
  leads = np.array([0, 6, 12], dtype='timedelta64[h]').astype('timedelta64[ns]')
  dims = ('metric', 'init_time', 'lead_time', 'latitude', 'longitude')
  outs = []
  for run_min in (1 << 40, 1):
    old = evaluation._RUN_MIN
    evaluation._RUN_MIN = run_min
    try:
      mean = evaluation.RunningMean('init_time', True, dev,
                                    split_dim='lead_time')
      g = torch.Generator(device=dev).manual_seed(3)
      for i in range(4):
        for sel in ([0, 1], [2], [1, 2]):
          v = torch.randn((2, 1, len(sel), 19, 36), generator=g, device=dev)
          v[0, 0, 0, 3, 5] = float('nan')
          coords = {'metric': ['a', 'b'], 'lead_time': leads[sel],
                    'init_time': np.array([i]), 'latitude': np.arange(19.0),
                    'longitude': np.arange(36.0)}
          mean.add(xl.Dataset({'z': xl.DataArray(v, dims, coords, 'z')},
                              coords))
      acc = mean._acc['z']
      sizes = sorted(t.numel() for t, _ in acc.dst.values())
      outs.append((mean.result()['z'].values, sizes))
    finally:
      evaluation._RUN_MIN = old
  (a, per_element), (b, per_run) = outs
  assert np.array_equal(a, b, equal_nan=True)
  assert per_element[0] == 2 * 1 * 19 * 36 and per_run[0] == 2 * 1
  del gen


def test_a_map_config_beside_scalar_configs_in_one_call(monkeypatch):
  """{deterministic, deterministic_spatial}: the scalar config replays its
  chunk program, the map config its suite, each result equals a call of its
  own."""
  from tests import test_chunk_program_gpu as tp
  from weatherbench2_amd import evaluation
  _, _, gf, gt, scalar = tp._setup(n_init=4, n_lead=2, n_lat=19, n_lon=36)
  _, _, _, _, maps = _setup(n_init=1, n_lead=1)
  both = {'deterministic': scalar, 'deterministic_spatial': maps}
  chunks = oc.chunk_pairs(gf, gt)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '0')
  want = {k: evaluation.evaluate_chunks(chunks, c, False, prefetch=0,
                                        batch_chunks=1)
          for k, c in both.items()}
  for how in ('1', 'verify'):
    monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', how)
    calls = _count_runs(monkeypatch)
    got = evaluation.evaluate_chunks(chunks, both, False, prefetch=0)
    for k in both:
      _same(got[k], want[k])
    assert len(calls) >= len(chunks) - 1


def test_map_results_without_skipna_keep_no_count_map():
  """RunningMean over map-valued device results (>= 2^20 elements per lead row)
  without skipna: every element of a row has the row's number of time steps --
  no count map is allocated (half of the accumulator state of
  `deterministic_spatial`), the mean is the sum over the steps / their number,
  NaNs propagate; with skipna the count map is there as before."""
  import torch
  from weatherbench2_amd import evaluation
  from weatherbench2_amd import xarray_lite as xl
  dev = torch.device('cuda')
  g = torch.Generator(device=dev).manual_seed(9)
  leads = np.array([0, 6], dtype='timedelta64[h]').astype('timedelta64[ns]')
  dims = ('metric', 'init_time', 'lead_time', 'latitude', 'longitude')
  n_lat, n_lon = 512, 2048
  values = torch.randn((1, 3, 2, n_lat, n_lon), generator=g, device=dev)
  values[0, 1, 0, 7, 9] = float('nan')
  coords_of = lambda i, sel: {
      'metric': ['m'], 'init_time': np.array([i]), 'lead_time': leads[sel],
      'latitude': np.arange(float(n_lat)), 'longitude': np.arange(float(n_lon))}
  for skipna in (False, True):
    mean = evaluation.RunningMean('init_time', skipna, dev,
                                  split_dim='lead_time',
                                  split_order='first_seen')
    for i in range(3):
      for sel in ([1], [0]):   # lead-major inside an init: rows 0 <-> label 1
        c = coords_of(i, sel)
        mean.add(xl.Dataset({'z': xl.DataArray(
            values[:, i:i + 1][:, :, sel].contiguous(), dims, c, 'z')}, c))
    acc = mean._acc['z']
    assert (acc._count is None) == (not skipna)
    got = mean.result()['z']
    np.testing.assert_array_equal(np.asarray(got.coords['lead_time']),
                                  leads[[1, 0]])
    v = values.double().cpu().numpy()[:, :, [1, 0]]
    with np.errstate(all='ignore'):
      import warnings
      with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = (np.nanmean if skipna else np.mean)(v, axis=1)
    # sums continue value by value in time order: the same float64 additions
    seq = np.zeros_like(want)
    cnt = np.zeros_like(want)
    for i in range(3):
      x = v[:, i]
      keep = ~np.isnan(x) if skipna else np.ones_like(x, bool)
      seq += np.where(keep, x, 0.0)
      cnt += keep
    with np.errstate(all='ignore'):
      exact = seq / cnt
    assert np.array_equal(got.values, exact, equal_nan=True)
    np.testing.assert_allclose(got.values, want, rtol=1e-12, equal_nan=True)
    assert np.isnan(got.values[0, 1, 7, 9]) == (not skipna)


@pytest.mark.parametrize('skipna', [False, True])
@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('order', ['init', 'lead'])
def test_windows_accumulate_k_chunks_of_a_lead_per_launch(order, k, skipna,
                                                          monkeypatch):
  """xbeam.Mean combines any number of chunks per key before touching the
  output (evaluation.py:735-744): inside a window the chunks that carry the
  same lead label are added by ONE launch (k time steps of that lead: the
  running sums are loaded and stored once) -- the additions of k separate
  launches in the same order, so the bits of chunk by chunk, whatever k and
  whatever the order of the chunk list."""
  from weatherbench2_amd import evaluation, map_suite
  n_lead = 3
  forecast, truth, gf, gt, cfg = _setup(n_init=8, n_lead=n_lead, n_lat=19,
                                        n_lon=36,
                                        nan_frac=0.02 if skipna else 0.0)
  chunks = oc.chunk_pairs(gf, gt, order=order)
  want = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                    batch_chunks=1)
  # (with WB2HIP_CHUNK_PROGRAM=verify every chunk goes alone, both ways)
  monkeypatch.setenv('WB2HIP_CHUNK_PROGRAM', '1')
  groups = []
  real = map_suite.MapSuite.run_many

  def run_many(self, pairs, mean):
    groups.append(len(pairs))
    return real(self, pairs, mean)
  monkeypatch.setattr(map_suite.MapSuite, 'run_many', run_many)
  # init-major: a window of k * n_lead chunks holds k chunks of every lead;
  # lead-major: k consecutive chunks share their lead
  window = k * n_lead if order == 'init' else k
  got = evaluation.evaluate_chunks(chunks, cfg, skipna, prefetch=0,
                                   batch_chunks=window)
  _same(got, want)
  if k > 1:
    assert max(groups) == k, groups
    # every chunk but the generic first one went through a group
    assert sum(groups) == len(chunks) - 1, groups
