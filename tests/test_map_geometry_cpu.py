"""What the map and running-mean sweep (tests/map_geometry_cases.py, run on the
GPU by test_map_geometry_gpu.py) reaches, asserted on the CPU: every
instantiation of the six kernels in both dtypes and both skipna values, the
point counts around the vector width and the 256-thread blocks, the vector
path turned off by each of its reasons alone, the grid's z dimension, every
remainder of the U-step time loops and of the SEEPS slab group.  Also ties the
per-point SEEPS restatement of tests/geometry_reference.py to the oracle."""
import collections
import re

import numpy as np
import pytest

from oracle import metrics_np as om
from oracle.named import DS, NA
from tests import geometry_reference as gr
from tests import map_geometry_cases as mc
from tests import official_chunks as oc

CASES = mc.CASES


def _of(kind):
  return [c for c in CASES if c.kind == kind]


def test_constants_come_from_the_source():
  assert mc.W == {'float32': 4, 'float64': 2}
  assert mc.BLOCK == 256 and mc.Y_SPLIT == 32768 and mc.SEEPS_Y_SPLIT == 32768
  assert mc.U == 4 and mc.U_TIME == 4 and mc.SEEPS_SLABS == 8
  sp = mc._read(mc.SPATIAL_SRC)
  st = mc._read(mc.STREAM_SRC)
  # the rules Case.vec restates
  assert re.search(r'bool ok = n_point % w == 0 && reinterpret_cast<uintptr_t>'
                   r'\(a\) % 16 == 0 &&\s*reinterpret_cast<uintptr_t>\(b\) % 16 '
                   r'== 0;\s*for \(int i = 0; outs && i < 3; \+\+i\)', sp)
  assert 'pick_vec(dtype, n_point, forecast, truth, p.out)' in sp
  assert 'pick_vec(dtype, n_point, forecast, truth, nullptr)' in sp
  assert 'const int vec = (aligned16 && n_point % w == 0) ? w : 1;' in sp
  assert 'const long long gx = (n_point / vec + 255) / 256;' in sp
  # both accumulate loops run groups of U steps, then the rest one by one
  assert sp.count('for (; i + U <= p.n_time; i += U)') == 2
  assert sp.count('for (; i < p.n_time; ++i)') == 2
  assert 'for (; t < n_time; ++t) add(base[t * n_tail]);' in st
  assert st.count('dim3(256)') >= 6
  for k in ('seeps_map_kernel', 'time_accumulate_kernel',
            'gather_accumulate_kernel'):
    assert re.search(r'__launch_bounds__\(256\)\s*' + k, st) or re.search(
        r'__launch_bounds__\(256\)\n\s+' + k, st), k


def test_every_instantiation_is_reached():
  seen = {c.instantiation for c in CASES}
  want = set()
  for d in mc.DTYPES:
    w = mc.W[d]
    want |= {('spatial_maps_kernel', d, v, None) for v in (1, w)}
    for s in (False, True):
      want |= {('spatial_accumulate_kernel', d, v, s) for v in (1, w)}
      want |= {('spatial_accumulate_addr_kernel', d, v, s) for v in (1, w)}
      want |= {('time_accumulate_kernel', d, e, s)
               for e in ('scatter', 'runs')}
    want |= {('seeps_map_kernel', d, e, None) for e in ('in', 'addr')}
  for s in (False, True):
    want.add(('time_accumulate_kernel', 'float64', 'plain', s))
    want |= {('gather_accumulate_kernel', 'float64', e, s)
             for e in ('plain', 'rows')}
  assert seen == want, (sorted(want - seen, key=str),
                        sorted(seen - want, key=str))


def _point_edges(d):
  w = mc.W[d]
  b = mc.BLOCK * w
  return {1, max(w - 1, 1), w, w + 1, b - 1, b, b + 1, b + w,
          mc.BLOCK - 1, mc.BLOCK + 1}


def test_point_counts_around_the_vector_and_the_blocks():
  for kind in ('maps', 'acc', 'addr'):
    for d in mc.DTYPES:
      pts = {c.n_point for c in _of(kind) if c.dtype == d}
      if kind == 'acc':
        for s in (False, True):
          assert {c.n_point for c in _of(kind) if c.dtype == d and
                  c.skipna == s} >= _point_edges(d), (d, s)
      assert pts >= _point_edges(d), (kind, d, sorted(_point_edges(d) - pts))
      # several blocks of vector threads, the last one ragged
      w = mc.W[d]
      assert any(c.dtype == d and c.vec == w and c.threads > 2 * mc.BLOCK and
                 c.threads % mc.BLOCK for c in _of(kind)), (kind, d)
      # both sides of one block of vector threads
      thr = {c.threads for c in _of(kind) if c.dtype == d and c.vec == w}
      assert {mc.BLOCK, mc.BLOCK + 1} <= thr, (kind, d)
      thr1 = {c.threads for c in _of(kind) if c.dtype == d and c.vec == 1}
      assert {mc.BLOCK - 1, mc.BLOCK + 1} <= thr1, (kind, d)


def test_the_vector_path_turned_off_by_each_reason_alone():
  for d in mc.DTYPES:
    w = mc.W[d]
    maps = [c for c in _of('maps') if c.dtype == d]
    reasons = {c.misalign for c in maps if c.n_point % w == 0 and c.vec == 1}
    assert reasons == {'f', 't', 'bias', 'mse', 'mae'}, reasons
    for c in maps:
      if c.misalign in mc.OUTS:
        assert 'bms'[mc.OUTS.index(c.misalign)] in c.outs
    assert any(c.n_point % w and not c.misalign and c.n_point > w
               for c in maps)
    for s in (False, True):
      acc = [c for c in _of('acc') if c.dtype == d and c.skipna == s]
      assert {c.misalign for c in acc if c.n_point % w == 0 and
              c.vec == 1} == {'f', 't'}
      assert any(c.n_point % w and not c.misalign for c in acc)
      addr = [c for c in _of('addr') if c.dtype == d and c.skipna == s]
      modes = {(c.aligned16, c.vec) for c in addr if c.n_point > w}
      assert modes == {('yes', w), ('off', 1), ('ragged', 1)}, modes
      assert all(c.n_point % w == 0 for c in addr if c.aligned16 == 'off')


def test_output_subsets_and_slab_tables():
  for d in mc.DTYPES:
    w = mc.W[d]
    maps = [c for c in _of('maps') if c.dtype == d]
    assert {c.outs for c in maps} == set(mc.SUBSETS)
    for v in (1, w):  # one, two and three outputs on both paths
      assert {len(c.outs) for c in maps if c.vec == v} == {1, 2, 3}, (d, v)
    assert {c.tables for c in maps} == {'', 'perm', 'bcast'}
    for s in (False, True):
      acc = [c for c in _of('acc') if c.dtype == d and c.skipna == s]
      for v in (1, w):
        assert {c.tables for c in acc if c.vec == v} == {'', 'perm', 'bcast'}
      addr = [c for c in _of('addr') if c.dtype == d and c.skipna == s]
      # ('mae', 'bias') as MapSuite passes it, and single kinds
      assert {'bms', 'sb', 'm'} <= {c.outs for c in addr}
      assert {True, False} == {c.sum_off for c in addr}


def test_the_grid_z_dimension():
  for d in mc.DTYPES:
    w = mc.W[d]
    maps = {(c.n_outer, c.vec) for c in _of('maps') if c.dtype == d}
    for n in mc.Y_EDGES:
      assert {(n, 1), (n, w)} <= maps, (d, n)
    assert {c.grid_z for c in _of('maps') if c.dtype == d} >= {1, 2, 3}
    for s in (False, True):
      for kind in ('acc', 'addr'):
        rows = {(c.n_outer, c.vec) for c in _of(kind)
                if c.dtype == d and c.skipna == s}
        for n in (mc.Y_SPLIT, mc.Y_SPLIT + 1):
          assert {(n, 1), (n, w)} <= rows, (kind, d, s, n)
        assert any(n == 1 for n, _ in rows)
        assert {c.grid_z for c in _of(kind) if c.dtype == d} == {1, 2}
    for e in ('in', 'addr'):
      seeps = [c for c in _of('seeps') if c.dtype == d and c.entry == e]
      assert {c.grid_z for c in seeps} == {1, 2}
      assert all(c.n_point == 1 for c in seeps if c.grid_z > 1)
      assert mc.SEEPS_SLABS * mc.SEEPS_Y_SPLIT + 1 in {c.n_outer for c in seeps}


def test_every_remainder_of_the_time_loops():
  for d in mc.DTYPES:
    w = mc.W[d]
    for s in (False, True):
      nts = {c.n_time for c in _of('acc')
             if c.dtype == d and c.skipna == s and c.vec == w}
      assert nts >= set(mc.N_TIMES), (d, s)
      # the scalar path: fewer steps than a group, every remainder, 2 groups
      nts = {c.n_time for c in _of('acc')
             if c.dtype == d and c.skipna == s and c.vec == 1}
      assert nts >= set(range(1, 2 * mc.U)), (d, s)
      nts = {c.n_time for c in _of('addr') if c.dtype == d and c.skipna == s}
      assert nts >= set(mc.N_TIMES)
      vt = {c.n_time for c in _of('addr') if c.dtype == d and
            c.skipna == s and c.vec == w}
      assert {n % mc.U for n in vt if n > mc.U} | {0} == set(range(mc.U))
      assert min(vt) < mc.U
      for e in ('scatter', 'runs') + (('plain',) if d == 'float64' else ()):
        nts = {c.n_time for c in _of('time')
               if c.dtype == d and c.skipna == s and c.entry == e}
        assert nts == set(range(1, 10)), (d, s, e)
  for e in ('plain', 'rows'):
    for s in (False, True):
      nts = {c.n_time for c in _of('gather') if c.entry == e and c.skipna == s}
      assert nts == set(range(1, 10))
  assert set(mc.N_TIMES) >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 13}
  assert {n % mc.U for n in mc.N_TIMES} == set(range(mc.U))


def test_seeps_slab_groups_and_points():
  for d in mc.DTYPES:
    for e in ('in', 'addr'):
      seeps = [c for c in _of('seeps') if c.dtype == d and c.entry == e]
      outer = {c.n_outer for c in seeps}
      assert outer >= set(mc.SEEPS_OUTER), (d, e)
      assert {n % mc.SEEPS_SLABS for n in outer} == set(range(mc.SEEPS_SLABS))
      assert {c.n_point for c in seeps} >= set(mc.SEEPS_POINTS)
      assert {c.tables for c in seeps} == {'', 'wet'}
      assert all(c.nan for c in seeps)


def test_time_shapes_runs_and_gathers():
  for d in mc.DTYPES:
    time = [c for c in _of('time') if c.dtype == d]
    n = {c.n_outer * c.n_tail for c in time}
    assert {mc.BLOCK - 1, mc.BLOCK, mc.BLOCK + 1, 2 * mc.BLOCK,
            2 * mc.BLOCK + 1} <= n, sorted(n)
    runs = [c for c in time if c.entry == 'runs']
    assert all(c.run > 1 and (c.n_outer * c.n_tail) % c.run == 0 for c in runs)
    assert len({c.run for c in runs}) >= 3
    # a run as long as the whole result (a prime element count)
    assert any(c.run == c.n_outer * c.n_tail for c in runs)
    assert all(c.run == 1 for c in time if c.entry != 'runs')
    assert {c.n_outer for c in time} > {1} and {c.n_tail for c in time} > {1}
  n_out = {c.n_outer for c in _of('gather')}
  assert {mc.BLOCK - 1, mc.BLOCK, mc.BLOCK + 1} <= n_out


def test_nan_kinds_meet_every_accumulate_instantiation():
  """The data builder (test_map_geometry_gpu.inject) puts forecast-only,
  truth-only, both and inf - inf NaNs at every fourth point, kind (slab +
  point // 4) % 5 + 1: a case with identity tables meets them all with two
  points and four slabs, or fourteen points."""
  for c in mc.CASES:
    if c.kind in ('acc', 'addr') and c.skipna:
      assert c.nan
  inst = collections.defaultdict(bool)
  for c in _of('acc') + _of('addr'):
    n_slab = c.n_time * c.n_outer
    full = c.n_point >= 2 and (n_slab >= 4 or c.n_point >= 14)
    ident = c.tables == '' and (c.kind == 'acc' or c.n_outer == 1)
    inst[c.instantiation] |= bool(c.skipna and c.nan and full and ident)
  assert all(v for k, v in inst.items() if k[3]), inst


def test_cases_are_unique_and_bounded():
  ids = [c.id for c in CASES]
  assert len(ids) == len(set(ids))
  assert 300 <= len(CASES) <= 480, len(CASES)
  for c in CASES:
    e = mc.ESIZE[c.dtype]
    elems = c.n_point * c.n_outer * max(c.n_time, 1)
    assert elems * e <= 2 ** 24, c.id


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_seeps_restatement_is_the_oracles(dtype):
  """gr.seeps_map against oracle/metrics_np.SpatialSEEPS.compute_chunk on a
  small dataset with values on both thresholds, NaNs and masked p1: the same
  bits (both compute the scoring matrix in p1's dtype, here the data's)."""
  name = '2m_temperature'
  forecast, truth, clim = oc.make(n_init=3, n_lead=3, n_level=1, n_lat=5,
                                  n_lon=7, seed=4, dtype=dtype)
  rs = np.random.RandomState(8)
  shape, cdims = clim[name].data.shape, clim[name].dims
  wet = rs.uniform(0.3, 1.2, size=shape).astype(dtype)
  frac = rs.uniform(0.0, 1.0, size=shape).astype(dtype)
  frac[:, :, 1, 2] = np.nan
  cvars = dict(clim.items())
  cvars[f'{name}_seeps_threshold'] = NA(wet, cdims)
  cvars[f'{name}_seeps_dry_fraction'] = NA(frac, cdims)
  clim = DS(cvars, clim.coords)
  metric = om.SpatialSEEPS(climatology=clim, precip_name=name,
                           dry_threshold_mm=100.0)
  dry = metric.dry_threshold_mm / 1000.0
  fdims = forecast[name].dims
  # the wet threshold at every valid time, as the oracle selects it
  doy, hour = om._dayofyear_hour(forecast.coords['valid_time'].data)
  di = {v: i for i, v in enumerate(clim.coord('dayofyear').tolist())}
  hi = {v: i for i, v in enumerate(clim.coord('hour').tolist())}
  wet_t = wet.transpose([cdims.index(d) for d in
                         ('hour', 'dayofyear', 'latitude', 'longitude')])
  wet_vt = wet_t[np.vectorize(hi.get)(hour), np.vectorize(di.get)(doy)]
  f = np.abs(forecast[name].data).astype(dtype)
  y = np.abs(truth[name].transpose(*fdims).data).astype(dtype)
  f[0, 0, 0, :3] = dtype(dry)
  f[1, 1, 2] = wet_vt[1, 1, 2]
  y[0, 1, :, 0] = dtype(dry)
  y[2, 0, 1] = wet_vt[2, 0, 1]
  f[2, 2, 3, 4] = np.nan
  y[1, 0, 4, 6] = np.nan
  fds = DS({name: NA(f, fdims)}, forecast.coords)
  tds = DS({name: NA(y, fdims)}, forecast.coords)
  with np.errstate(all='ignore'):
    want = metric.compute_chunk(fds, tds)[name]
  want = np.asarray(want.transpose(*fdims).data)
  p1 = metric.p1.transpose('latitude', 'longitude').data
  with np.errstate(invalid='ignore'):
    keep = (p1 < metric.max_p1) & (p1 > metric.min_p1)
  aux = np.where(keep, p1.astype(np.float64), np.nan)
  got = gr.seeps_map(f, y, wet_vt, aux, dry, dtype)
  assert want.dtype == np.float64
  gr.assert_bits(got, want, f'SpatialSEEPS {np.dtype(dtype).name}')
  assert np.isnan(want).any() and (want == 0).any() and (want > 0).any()
  # every cell of the scoring matrix and the threshold values occur
  cat = lambda x: np.select([x < dtype(dry), (x > dtype(dry)) & (x < wet_vt),
                             x >= wet_vt], [0, 1, 2], 3)
  with np.errstate(invalid='ignore'):
    cells = set(zip(cat(f).ravel().tolist(), cat(y).ravel().tolist()))
  assert {(i, j) for i in range(3) for j in range(3)} <= cells, cells
  assert (f == dtype(dry)).any() and (y == wet_vt).any()
