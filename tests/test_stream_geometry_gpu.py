"""The streaming reduction across tile, row-end and segment boundaries (-m gpu).

K1 (stream_partials_kernel), K1p (stream_pair_kernel) and the K2 fold against
a plain float64 reference, over the geometry sweep of
tests/stream_geometry_cases.py (its coverage is asserted on the CPU by
test_stream_geometry_cpu.py).

The reference is independent of plan.py: per-point region weights are
oracle/metrics_np.get_lat_weights times what oracle/regions_np's Region.apply
leaves (land fraction included), per-point quantities are computed in the
input dtype like the kernels (the library is built with -ffp-contract=off, so
float32 NumPy arithmetic gives the kernels' values bit for bit), and every sum
is a math.fsum of the float64 products.  Only the order of the float64
additions differs, so a sum may be off by 1e-12 * sum|w x| at most.  The data
keep every point's |w x| above 1e-8 * sum|w x| (bounded values, no exact
zeros): one dropped or double-counted point fails that tolerance, which each
case proves on the reference itself.
"""
import numpy as np
import pytest

from oracle import metrics_np as om
from oracle.named import DS, NA
from tests import geometry_reference as gr
from tests import helpers
from tests import stream_geometry_cases as sg

pytestmark = pytest.mark.gpu

SUM_RTOL = gr.SUM_RTOL
N_POOL = 3
TABLE = (2, 0, 2, 1)  # permutes and repeats the pool's slabs


@pytest.fixture(scope='module')
def dev():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device')
  return torch.device('cuda')


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import _lib
  return _lib.load()


# ---- the reference ----------------------------------------------------------
def point_slots(mode, skipna, ins):
  """The K per-point values of PointOps<MODE> (stream_reduce.hip), float64."""
  def keep(q):
    ok = ~np.isnan(q)
    return np.where(ok, q, 0).astype(np.float64), ok.astype(np.float64)
  if mode == 'wind':
    du, dv = ins[0] - ins[1], ins[2] - ins[3]
    q, ok = keep(du * du + dv * dv)
    return [q, ok] if skipna else [q]
  d = ins[0] - ins[1]
  qs = [d, d * d]
  if mode == 'det_acc':
    fa, ta = ins[0] - ins[2], ins[1] - ins[2]
    qs += [fa * ta, fa * fa, ta * ta]
  if not skipna:
    x = [q.astype(np.float64) for q in qs]
    return [x[0], np.abs(x[0])] + x[1:]
  kept = [keep(q) for q in qs]
  x = [v for v, _ in kept]
  out = [x[0], np.abs(x[0])] + x[1:]
  if mode == 'det':
    return out + [kept[0][1]]
  return out + [kept[0][1], kept[2][1], kept[3][1], kept[4][1]]


def ref_metrics(mode, skipna, sums, wsum):
  """K2's metrics [MSE, RMSE, MAE, Bias, ACC][n_region][n_outer]."""
  def den(x):
    return np.where(x != 0, x, np.nan)
  s = np.moveaxis(sums, 0, -1)  # [n_region, K, n_outer]
  n_region, _, n_outer = s.shape
  out = np.full((5, n_region, n_outer), np.nan)
  w = wsum[:, None]
  with np.errstate(all='ignore'):
    if mode == 'wind':
      out[0] = s[:, 0] / (den(s[:, 1]) if skipna else den(w))
      out[1] = np.sqrt(out[0])
      return out
    kq = 6 if mode == 'det_acc' else 3
    dd = den(s[:, kq]) if skipna else den(w)
    out[3], out[2], out[0] = s[:, 0] / dd, s[:, 1] / dd, s[:, 2] / dd
    out[1] = np.sqrt(out[0])
    if mode == 'det_acc':
      dp, df, dt = ((den(s[:, j]) if skipna else den(w)) for j in (7, 8, 9))
      out[4] = (s[:, 3] / dp) / np.sqrt((s[:, 4] / df) * (s[:, 5] / dt))
  return out


def assert_metrics(got, want, names, tag):
  """Every metric is a quotient of sums that are good to SUM_RTOL relative to
  their sum |w x|: 1e-10 relative is ~20x that bound for MSE / RMSE / MAE /
  ACC (quotients of positive sums here).  Bias cancels: its numerator is good
  to SUM_RTOL * sum|w d|, i.e. to SUM_RTOL * MAE after the division, so it
  gets 4 * SUM_RTOL * MAE on top."""
  got = np.asarray(got, dtype=np.float64)
  assert got.shape == want.shape, (got.shape, want.shape, tag)
  for m in range(5):
    atol = 4 * SUM_RTOL * np.nan_to_num(np.abs(want[2])) if m == 3 else 0.0
    ok = (np.isnan(got[m]) == np.isnan(want[m])) & (
        np.isnan(want[m]) | (np.abs(got[m] - want[m]) <= 1e-10 * np.abs(
            want[m]) + atol))
    if not ok.all():
      r, o = np.argwhere(~ok)[0]
      raise AssertionError(
          f'{tag}: metric {m} region {names[r]} outer {o}: got '
          f'{got[m, r, o]!r} want {want[m, r, o]!r}')


def prove_tolerance(res, weights, slots, sums, mags, o):
  """A kernel that dropped the first owned column of tile 1, or counted the
  last column twice, would fail SUM_RTOL: shown on the reference (global
  region, outer slab `o`, whose row 0 has no NaN) for every slot that cannot
  cancel."""
  sign_free = [j for j in range(len(slots))
               if res.case.mode == 'wind' or j != 0]
  gr.prove_tolerance(weights, slots, sums, mags, o,
                     64 * sg.launch_vec(res), sign_free)


# ---- data -------------------------------------------------------------------
def pool_inputs(res, rs, weights):
  """The pool's input slabs [N_POOL, n_row, n_col] in the case's dtype: every
  per-point value bounded away from 0, NaNs (skipna only) in the row-end
  window, on the first column of tiles, over a whole row and over all of
  region 'one_col' of slab 2."""
  case = res.case
  shape = (N_POOL, res.n_row, res.n_col)

  def signed(lo, hi):
    return np.where(rs.rand(*shape) < 0.5, -1.0, 1.0) * rs.uniform(lo, hi,
                                                                    shape)
  if case.mode == 'det_acc':
    c = rs.uniform(-3, 3, shape)
    t = c + signed(1.0, 2.0)
    ins = [t + signed(0.25, 0.5), t, c]
  elif case.mode == 'det':
    t = rs.uniform(-3, 3, shape)
    ins = [t + signed(0.5, 2.0), t]
  else:
    tu, tv = rs.uniform(-3, 3, shape), rs.uniform(-3, 3, shape)
    ins = [tu + signed(0.5, 2.0), tu, tv + signed(0.5, 2.0), tv]
  ins = [x.astype(case.dtype) for x in ins]
  if case.skipna:
    n, v, tile = res.n_col, sg.launch_vec(res), 64 * sg.launch_vec(res)
    rows = np.arange(res.n_row)
    f, t = ins[0], ins[1]
    f[0, rows % 3 == 2, n - 1] = np.nan              # the last column
    for c in range(max(n - v, 0), n):                 # the row-end window
      t[0, rows % 3 == 1, c] = np.nan
    for c in range(tile, n, tile):                    # first column of a tile
      f[0, rows % 2 == 1, c] = np.nan
    t[1, res.n_row // 2, :] = np.nan                  # a whole row
    if 'one_col' in res.regions:                      # a whole region
      f[2][weights[list(res.regions).index('one_col')] != 0] = np.nan
    if case.mode == 'det_acc':
      ins[2][1, 0, 0] = np.nan
  return ins


def make_plan(res, dev):
  from weatherbench2_amd import plan as plan_lib
  return plan_lib.build_plan(
      res.lat, res.lon,
      plan_lib.LATLON if res.case.layout == 'latlon' else plan_lib.LONLAT,
      {k: helpers.to_gpu_region(v) for k, v in res.regions.items()}, dev,
      rows_per_chunk=res.case.rows_per_chunk or plan_lib.DEFAULT_ROWS_PER_CHUNK)


def mode_code(mode):
  from weatherbench2_amd import _lib
  return {'det': _lib.MODE_DET, 'det_acc': _lib.MODE_DET_ACC,
          'wind': _lib.MODE_WIND}[mode]


def run_k1(res, pl, ins, dev):
  """K1 + K2 over the case's slab layout: (metrics, sums, outer -> pool)."""
  import torch
  from weatherbench2_amd import engine
  case = res.case
  tdt = getattr(torch, case.dtype)
  mode = mode_code(case.mode)
  if case.slabs == 'contiguous':
    t_ins = [torch.as_tensor(x, device=dev) for x in ins]
    m, s = engine.stream_reduce(pl, mode, t_ins, [None] * len(ins), N_POOL,
                                case.skipna, want_sums=True)
    return m, s, np.arange(N_POOL)
  table = np.array(TABLE)
  if case.slabs == 'table':
    t_ins = [torch.as_tensor(x, device=dev) for x in ins]
    tabs = [torch.as_tensor(table, dtype=torch.int64, device=dev)
            for _ in ins]
    m, s = engine.stream_reduce(pl, mode, t_ins, tabs, len(table),
                                case.skipna, want_sums=True)
    return m, s, table
  # by address: every slab 16-byte aligned (a padded pool), or every slab
  # one element past an aligned address
  elem = np.dtype(case.dtype).itemsize
  n_el = res.n_row * res.n_col
  keep, addr = [], []
  for x in ins:
    if case.slabs == 'addr':
      stride = -(-n_el * elem // 16) * 16 // elem
      buf = torch.zeros((N_POOL, stride), dtype=tdt, device=dev)
      buf[:, :n_el] = torch.as_tensor(x.reshape(N_POOL, n_el), device=dev)
      first = buf.data_ptr()
    else:
      stride = n_el
      buf = torch.zeros((N_POOL * n_el + 1,), dtype=tdt, device=dev)
      buf[1:] = torch.as_tensor(x.ravel(), device=dev)
      first = buf.data_ptr() + elem
    keep.append(buf)
    addr.append(torch.as_tensor(first + table * stride * elem,
                                dtype=torch.int64, device=dev))
  m, s = engine.stream_reduce_addr(pl, mode, tdt, addr,
                                   case.slabs == 'addr', len(table),
                                   case.skipna, want_sums=True)
  torch.cuda.synchronize()
  del keep
  return m, s, table


def all_weights(res):
  return [gr.region_weights(r, res.lat, res.lon, res.case.layout)
          for r in res.regions.values()]


def reference(res, ins, outer, weights):
  slots = point_slots(res.case.mode, res.case.skipna, [x[outer] for x in ins])
  sums, mags, wsum = gr.ref_sums(weights, slots)
  return slots, sums, mags, wsum


def _case_seed(case):
  return sum(map(ord, case.id)) % 100003


# ---- K1 + K2 over the sweep -------------------------------------------------
@pytest.mark.parametrize('case', sg.CASES, ids=lambda c: c.id)
def test_stream_reduce_geometry(dev, lib, case):
  res = sg.resolve(lib, case)
  rs = np.random.RandomState(_case_seed(case))
  weights = all_weights(res)
  ins = pool_inputs(res, rs, weights)
  pl = make_plan(res, dev)
  got_m, got_s, outer = run_k1(res, pl, ins, dev)
  slots, sums, mags, wsum = reference(res, ins, outer, weights)
  prove_tolerance(res, weights, slots, sums, mags, int(np.argmax(outer == 0)))
  tag = f'{case.id} n_col={res.n_col} T={res.tile}'
  gr.assert_sums(got_s.cpu().numpy(), sums, mags, tag)
  want_m = ref_metrics(case.mode, case.skipna, sums, wsum)
  assert_metrics(got_m.cpu().numpy(), want_m, list(res.regions), tag)
  if case.skipna and 'one_col' in res.regions and 2 in outer:
    # region 'one_col' of slab 2 is all NaN: count 0, NaN metrics
    r = list(res.regions).index('one_col')
    o = int(np.argmax(outer == 2))
    k_count = {'det': 3, 'det_acc': 6, 'wind': 1}[case.mode]
    assert got_s[o, r, k_count].item() == 0.0
    assert np.isnan(got_m[0, r, o].item())


# ---- the production paths: SuiteStep and PairSuiteStep (K1p) ------------------
PRODUCTION_CASES = [c for c in sg.CASES
                    if c.mode == 'det_acc' or (c.mode == 'det' and c.skipna
                                               and c.layout == 'latlon')]


@pytest.mark.parametrize('case', PRODUCTION_CASES, ids=lambda c: c.id)
def test_suite_steps_geometry(dev, lib, case):
  """engine.SuiteStep (bench.py, the chunk replay) and engine.PairSuiteStep:
  per-variable metrics of every slab and, where a pair kernel exists, the
  wind-vector MSE / RMSE of the last two slabs as a (u, v) pair, both against
  the float64 reference.  The pair kernel exists at the full lane width only:
  not for n_col in {1, VEC-1} (n_col < VEC)."""
  import torch
  from weatherbench2_amd import engine
  res = sg.resolve(lib, case)
  rs = np.random.RandomState(_case_seed(case) + 1)
  weights = all_weights(res)
  ins = pool_inputs(res, rs, weights)
  pl = make_plan(res, dev)
  tdt = getattr(torch, case.dtype)
  mode = mode_code(case.mode)
  table = np.array(TABLE)
  t_ins = [torch.as_tensor(x, device=dev) for x in ins]
  tabs = [torch.as_tensor(table, dtype=torch.int64, device=dev) for _ in ins]
  slots, sums, mags, wsum = reference(res, ins, table, weights)
  want = ref_metrics(case.mode, case.skipna, sums, wsum)
  names = list(res.regions)
  tag = f'{case.id} n_col={res.n_col} T={res.tile}'

  step = engine.SuiteStep(pl, mode, tdt, case.skipna, len(table))
  got = step.run(t_ins, tabs).cpu().numpy()
  assert_metrics(got, want, names, 'SuiteStep ' + tag)

  supported = engine.pairs_supported(pl, mode, tdt, case.skipna)
  assert supported == (res.n_col >= res.vec), tag
  if not supported:
    return
  step = engine.PairSuiteStep(pl, mode, tdt, case.skipna, len(table), 1)
  got_det, got_wind = step.run(t_ins, tabs)
  assert_metrics(got_det.cpu().numpy(), want, names,
                 'PairSuiteStep ' + tag)
  u, v = table[-2], table[-1]
  wslots = point_slots('wind', case.skipna, [
      ins[0][u:u + 1], ins[1][u:u + 1], ins[0][v:v + 1], ins[1][v:v + 1]])
  wsums, _, _ = gr.ref_sums(weights, wslots)
  want_w = ref_metrics('wind', case.skipna, wsums, wsum)
  assert_metrics(np.concatenate([got_wind[:2].cpu().numpy(), want_w[2:]]),
                 want_w, names, 'PairSuiteStep wind ' + tag)


# ---- GAUSS, GAUSS_THR and SEEPS through the public classes -------------------
# (dtype, n_col, layout, skipna, n_row, field): every n_col of the sweep in
# float64 at rtol 1e-9 (one dropped point of <= 37 x (5T + 3) moves a mean by
# ~1e-5), a float32 subset at test_fuzz_gpu.py's float32 tolerances
GENERIC_CASES = (
    [('float64', sym, ('latlon', 'lonlat')[i % 2], bool(i % 3 == 1),
      sg.N_ROW[i % 4], ('f64', None)[i % 2]) for i, sym in enumerate(sg.N_COL)]
    + [('float32', sym, ('lonlat', 'latlon')[i % 2], bool(i % 2),
        sg.N_ROW[(i + 2) % 4], None)
       for i, sym in enumerate(('VEC-1', 'T+1', '3T+VEC-1', '5T+3'))])


def _generic_geometry(lib, dtype, sym, layout, skipna, n_row, field):
  from weatherbench2_amd import _lib
  code = _lib.WB2_F32 if dtype == 'float32' else _lib.WB2_F64
  vec = lib.wb2_tile_cols_ex(_lib.MODE_GAUSS, code, int(skipna),
                             int(field is not None), 1 << 20, 1) // 64
  n_col = sg.n_col_of(sym, vec, 64 * vec)
  lat, lon = sg.coords(n_row, n_col, layout)
  case = sg.Case('det', dtype, layout, skipna, sym, n_row, None, field,
                 'contiguous')
  regs = sg.regions(case, n_row, n_col, vec, 64 * vec, lat, lon)
  spatial = (('latitude', 'longitude') if layout == 'latlon' else
             ('longitude', 'latitude'))
  return n_col, vec, lat, lon, regs, spatial


def _with_nans(x, n_col, vec, rs):
  """NaNs in the last column, on the first column of every tile and at a few
  random points of [..., n_row, n_col] slabs."""
  x = x.copy()
  x[..., 1::2, n_col - 1] = np.nan
  x[..., 1::2, 64 * vec::64 * vec] = np.nan
  x[rs.rand(*x.shape) < 0.01] = np.nan
  return x


@pytest.mark.parametrize('geo', GENERIC_CASES, ids=lambda g: '-'.join(
    str(v) for v in g))
def test_gaussian_and_seeps_geometry(dev, lib, geo):
  from oracle import thresholds_np as oth
  from weatherbench2_amd import metrics as gm
  from weatherbench2_amd import thresholds as gth
  dtype, sym, layout, skipna, n_row, field = geo
  n_col, vec, lat, lon, regs, spatial = _generic_geometry(lib, *geo)
  dt = np.dtype(dtype)
  rs = np.random.RandomState(sum(map(ord, '-'.join(map(str, geo)))))
  g = helpers.to_gpu_dataset
  g_regs = {k: helpers.to_gpu_region(v) for k, v in regs.items()}
  tol = (dict(rtol=1e-9, atol=1e-12) if dtype == 'float64' else None)
  n_time = 2
  t0 = np.datetime64('2021-02-27T00', 'ns')
  time = t0 + np.arange(n_time) * np.timedelta64(24, 'h')
  sshape = tuple(len(lat) if d == 'latitude' else len(lon) for d in spatial)
  shape = (n_time,) + sshape
  dims = ('time',) + spatial
  coords = {'time': time, 'latitude': lat, 'longitude': lon}
  tag = f'{geo} n_col={n_col}'

  mean = rs.uniform(-2, 2, shape)
  if skipna:
    mean = _with_nans(mean, shape[-1], vec, rs)
  std = rs.uniform(0.5, 1.5, shape)
  truth = DS({'z': NA(rs.uniform(-2, 2, shape).astype(dt), dims)}, coords)
  gf = DS({'z': NA(mean.astype(dt), dims), 'z_std': NA(std.astype(dt), dims)},
          coords)
  cdims = ('dayofyear', 'level') + spatial
  cshape = (3, 1) + sshape
  ccoords = {'dayofyear': 57 + np.arange(3), 'level': np.array([500]),
             'latitude': lat, 'longitude': lon}
  clim = DS({'z': NA(rs.uniform(-0.5, 0.5, cshape).astype(dt), cdims),
             'z_std': NA(rs.uniform(0.5, 1.0, cshape).astype(dt), cdims)},
            ccoords)
  oths = [oth.GaussianQuantileThreshold(clim, 0.3)]
  gths = [gth.GaussianQuantileThreshold(climatology=g(clim), quantile=0.3)]
  gdims = ('time', 'level') + spatial
  gl = DS({k: NA(v.data[:, None], gdims) for k, v in gf.items()},
          {**coords, 'level': np.array([500])})
  tl = DS({'z': NA(truth['z'].data[:, None], gdims)}, gl.coords)

  with gm.fused_regions(g_regs):
    for name in ('GaussianCRPS', 'GaussianVariance'):
      t_ = tol or dict(rtol=2e-5, atol=1e-6)
      for rname, region in regs.items():
        want = getattr(om, name)().compute_chunk(gf, truth, region=region,
                                                 skipna=skipna)['z']
        got = getattr(gm, name)().compute_chunk(
            g(gf), g(truth), region=g_regs[rname], skipna=skipna)['z']
        helpers.assert_close(got.values, want.data,
                             err_msg=f'{name} {rname} {tag}', **t_)
    for rname, region in regs.items():
      t_ = tol or dict(rtol=3e-5, atol=2e-6)
      want = om.GaussianBrierScore(thresholds=oths).compute_chunk(
          gl, tl, region=region, skipna=skipna)['z']
      got = gm.GaussianBrierScore(thresholds=gths).compute_chunk(
          g(gl), g(tl), region=g_regs[rname], skipna=skipna)['z']
      helpers.assert_close(got.values, want.data,
                           err_msg=f'GaussianBrierScore {rname} {tag}', **t_)

  # SEEPS: precipitation with values exactly on the dry and wet thresholds
  name = 'total_precipitation_24hr'
  dry = 0.25 / 1000.0
  wet = rs.uniform(0.002, 0.02, size=(4, 3) + sshape).astype(dt)
  frac = rs.uniform(0.15, 0.8, size=(4, 3) + sshape).astype(dt)

  def precip():
    x = rs.gamma(0.3, 2.0, size=shape) * 1e-2
    pick = rs.rand(*shape)
    x = np.where(pick < 0.1, dry, x)
    x = np.where((pick >= 0.1) & (pick < 0.2), wet[0, 0][None], x)
    return _with_nans(x, shape[-1], vec, rs).astype(dt)
  scoords = {**coords, 'valid_time': NA(time, ('time',))}
  forecast = DS({name: NA(precip(), dims)}, scoords)
  ptruth = DS({name: NA(precip(), dims)}, scoords)
  clim = DS({name + '_seeps_threshold': NA(wet, ('hour', 'dayofyear') +
                                           spatial),
             name + '_seeps_dry_fraction': NA(frac, ('hour', 'dayofyear') +
                                              spatial)},
            {'hour': np.array([0, 6, 12, 18]),
             'dayofyear': np.array([57, 58, 59]), 'latitude': lat,
             'longitude': lon})
  t_ = tol or dict(rtol=2e-6, atol=1e-7)
  with gm.fused_regions(g_regs):
    for rname, region in regs.items():
      want = om.SEEPS(climatology=clim).compute_chunk(
          forecast, ptruth, region=region)[name]
      got = gm.SEEPS(climatology=g(clim)).compute_chunk(
          g(forecast), g(ptruth), region=g_regs[rname])[name]
      helpers.assert_close(got.values, want.data,
                           err_msg=f'SEEPS {rname} {tag}', **t_)
