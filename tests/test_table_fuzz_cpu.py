"""The verification-table fuzz without a GPU: what the case list of
tests/table_fuzz_cases.py reaches, the package's host path against the
independent definitions of tests/*_np.py on every case, the conditions that
keep the fuzz from going blind, and planted mutants of the host path that the
cases must catch."""
import functools

import numpy as np
import pytest

from tests import conditional_cases
from tests import pooling_cases
from tests import table_fuzz_cases as fc
from tests import table_fuzz_checks as checks
from weatherbench2_amd import conditional
from weatherbench2_amd import crps_decomposition
from weatherbench2_amd import events
from weatherbench2_amd import neighborhood
from weatherbench2_amd import pooling
from weatherbench2_amd import threshold_weighted

WITH_THRESHOLDS = ('k18', 'k19', 'k21')
WITH_WINDOWS = ('k19', 'k22')
WITH_CLASSES = ('k18', 'k19', 'k20', 'k21', 'k24')
SORTED = ('k20', 'k21', 'k24')  # the padded sorting networks
_ID = lambda case: case.id


@functools.lru_cache(maxsize=None)
def _host(case):
  """The host-path run of a case: computed once, shared, left unchanged."""
  return checks.run(case, device=False)


# ---------------------------------------------------------------------------
# 1. reach
# ---------------------------------------------------------------------------
def test_the_list_is_forty_seeded_cases_a_family_with_distinct_ids():
  assert len(fc.CASES) == len(fc.FAMILIES) * fc.N_PER_FAMILY
  assert len({c.id for c in fc.CASES}) == len(fc.CASES)
  for family in fc.FAMILIES:
    cases = fc.BY_FAMILY[family]
    assert len(cases) == fc.N_PER_FAMILY
    assert [c.level for c in cases[:2]] == ['engine', 'metric']
  # the draw is a function of the seed alone
  assert fc._case('k19', 7) == fc.BY_FAMILY['k19'][7]
  again = fc.arrays.__wrapped__(fc.CASES[3])
  for key, value in fc.arrays(fc.CASES[3]).items():
    for a, b in zip(*[v if isinstance(v, list) else [v]
                      for v in (value, again[key])]):
      np.testing.assert_array_equal(a, b)


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib


def test_pool_window_limits_are_the_kernels(lib):
  import torch
  from weatherbench2_amd import engine
  for name, dtype in (('float32', torch.float32), ('float64', torch.float64)):
    assert engine.pool_geometry(dtype)['max_window'] == (
        fc.POOL_MAX_WINDOW[name])


@pytest.mark.parametrize('family', fc.FAMILIES)
def test_cases_reach_what_they_are_meant_to(family):
  cases = fc.BY_FAMILY[family]
  have = lambda pred: any(pred(c) for c in cases)
  assert {c.np_dtype for c in cases} == {np.float32, np.float64}
  for edge in (64, 128):
    assert have(lambda c: c.n_col < edge and c.n_col > edge - 64), edge
    assert have(lambda c: c.n_col == edge), edge
    assert have(lambda c: c.n_col > edge), edge
  assert have(lambda c: c.n_col % 4 != 0) and have(lambda c: c.n_col % 4 == 0)
  assert {c.skipna for c in cases} == {False, True}
  assert {c.level for c in cases} == {'engine', 'metric'}
  assert {c.form for c in cases if c.level == 'metric'} == set(fc.FORMS)
  assert have(lambda c: c.n_row == 1) or have(lambda c: c.n_row <= 3)
  assert {c.n_outer for c in cases} == {1, 2, 3}
  if family in SORTED:
    pads = {max(2, 1 << (c.n_member - 1).bit_length()) for c in cases}
    assert pads == {2, 4, 8, 16, 32, 64}
    # (K21, K24: their bounds are derived for two columns or more)
    assert family == 'k20' or all(c.n_col >= 2 for c in cases)
  if family == 'k21':
    assert have(lambda c: c.dtype == 'mixed')
    assert {c.tail for c in cases} == set(fc.TAILS)
    assert have(lambda c: c.nan == 'threshold')
  if family in WITH_THRESHOLDS:
    assert have(lambda c: c.n_thr > 4) and have(lambda c: c.n_thr == 1)
    assert have(lambda c: c.n_thr == 4)
  else:
    assert not have(lambda c: c.n_thr)
  if family in WITH_WINDOWS:
    assert have(lambda c: len(c.windows) > 4)
    assert have(lambda c: max(c.windows) > c.n_row)
    assert have(lambda c: c.n_col in c.windows and c.n_col > 1)
    for c in cases:
      top = 255 if family == 'k19' else fc.POOL_MAX_WINDOW[
          'float64' if c.dtype == 'float64' else 'float32']
      assert 1 <= len(c.windows) <= 6 and len(set(c.windows)) == len(
          c.windows)
      assert all(n % 2 == 1 and 1 <= n <= min(c.n_col, top)
                 for n in c.windows), c.id
      odd = [n for n in range(1, min(c.n_col, top) + 1, 2)]
      if any(n > c.n_row for n in odd):
        assert max(c.windows) > c.n_row, c.id
      if c.n_col % 2 and c.n_col <= top:
        assert c.n_col in c.windows, c.id
  if family == 'k24':
    assert {c.by for c in cases} == set(conditional_cases.BYS)
    assert {c.n_edge for c in cases} >= {1, 8}
    for c in cases:
      a = fc.arrays(c)
      edges = np.array(a['edges'])
      assert 1 <= edges.size == c.n_edge <= 8 and (np.diff(edges) > 0).all()
      values = np.abs(a['truth']) if c.by == 'spread' else a['truth']
      assert np.isin(edges, values.astype(np.float64)).any(), c.id
  if family == 'k22':
    assert {c.kind for c in cases} == set(pooling_cases.KINDS)
    assert have(lambda c: c.nan == 'planted' and np.isinf(
        fc.arrays(c)['x']).any() and np.isnan(fc.arrays(c)['x']).any())
  if family in ('k18', 'k19'):
    assert have(lambda c: c.n_member in (127, 128))
    assert have(lambda c: np.isinf(fc.arrays(c)['ens']).any())
  if family in WITH_CLASSES:
    engine_cases = [c for c in cases if c.level == 'engine']
    unused = again = border = single = 0
    for c in engine_cases:
      cls, wrow, mult = fc.engine_tables(c)
      assert cls.dtype == np.int32 and cls.shape == (c.n_col,)
      assert 0 <= cls.min() and cls.max() < c.n_class <= 64
      used = np.unique(cls)
      assert c.n_class == 1 or used.size < c.n_class, c.id
      assert cls[0] == cls[-1]
      unused += used.size < c.n_class
      single += c.n_class == 1
      # a class that is left and met again; unsorted labels
      runs = cls[np.r_[True, cls[1:] != cls[:-1]]]
      again += runs.size > np.unique(runs).size
      border += c.n_col > 64 and cls[64] != cls[63]
      assert wrow.shape == (fc.N_FOLD_REGION, c.n_row)
      assert mult.shape == (fc.N_FOLD_REGION, c.n_class)
    assert unused >= 10 and again >= 10 and border >= 2 and single >= 1
    assert any((np.diff(fc.engine_tables(c)[0]) < 0).any()
               for c in engine_cases)
    # metric level: a subset of the known regions and the two boxes
    from tests import events_cases
    known = set(events_cases.oracle_regions())
    sizes = set()
    for c in cases:
      if c.level == 'metric':
        names = list(fc.oracle_region_set(c))
        assert names[-2:] == ['box0', 'box1'] and set(names[:-2]) <= known
        sizes.add(len(names))
    assert len(sizes) > 1


# ---------------------------------------------------------------------------
# 2. the host path against the definitions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.CASES, ids=_ID)
def test_host_path_equals_the_definition(case):
  assert checks.has_valid_point(case)
  worst = checks.against_definition(case, _host(case))
  assert worst <= 1.0


# ---------------------------------------------------------------------------
# 3. what keeps the fuzz from going blind
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', fc.FAMILIES)
def test_the_fuzz_is_not_blind(family):
  cases = fc.BY_FAMILY[family]
  void = [c.id for c in cases if checks.all_nan(c, _host(c))]
  print(f'{family}: {len(void)} of {len(cases)} tables are NaN throughout')
  assert 3 * len(void) <= len(cases), void
  assert all(checks.has_valid_point(c) for c in cases)
  assert any(checks.regions_differ(c, _host(c)) for c in cases)
  # ... at both levels
  for level in ('engine', 'metric'):
    assert any(checks.regions_differ(c, _host(c)) for c in cases
               if c.level == level), level


# ---------------------------------------------------------------------------
# 4. planted mutants of the host path
# ---------------------------------------------------------------------------
def _box_wrap_off_by_one(field, h):
  """neighborhood._box with the columns past the row end one too far."""
  n_row, n_col = field.shape[-2:]
  zero = np.zeros(field.shape[:-2] + (1, n_col), dtype=np.int64)
  down = np.concatenate([zero, np.cumsum(field, axis=-2)], axis=-2)
  rows = np.arange(n_row)
  vert = (down[..., np.minimum(rows + h, n_row - 1) + 1, :] -
          down[..., np.maximum(rows - h, 0), :])
  out = np.zeros_like(vert)
  cols = np.arange(n_col)
  for d in range(-h, h + 1):
    j = cols + d
    out += vert[..., np.where(j >= n_col, j + 1, j) % n_col]
  return out


def _box_pole_clip_one_more(field, h):
  """neighborhood._box with a window that is clipped at the last row losing
  that row too."""
  n_row, n_col = field.shape[-2:]
  zero = np.zeros(field.shape[:-2] + (1, n_col), dtype=np.int64)
  down = np.concatenate([zero, np.cumsum(field, axis=-2)], axis=-2)
  rows = np.arange(n_row)
  last = np.where(rows + h > n_row - 1, np.maximum(n_row - 2, rows),
                  np.minimum(rows + h, n_row - 1))
  vert = down[..., last + 1, :] - down[..., np.maximum(rows - h, 0), :]
  out = np.zeros_like(vert)
  for d in range(-h, h + 1):
    out += np.roll(vert, d, axis=-1)
  return out


def _exceedance_or_equal(ens, member_stride, n_member, ens_slab, truth,
                         truth_slab, thresholds, thr_slabs, n_outer, slab):
  """events.host_exceedance with >= for >."""
  thr_slabs = thr_slabs if thr_slabs is not None else [None] * len(thresholds)
  for o, x, tv in events.host_members(ens, member_stride, n_member, ens_slab,
                                      truth, truth_slab, n_outer, slab):
    bad = np.isnan(tv) | np.isnan(x).any(axis=0)
    for ti, (thr, table) in enumerate(zip(thresholds, thr_slabs)):
      hv = events.host_slab(thr.reshape(-1), table, o, slab)
      with np.errstate(invalid='ignore'):
        k, obs = (x >= hv[None]).sum(axis=0), tv >= hv
      yield ti, o, k, obs, bad


def _twcrps_truth_not_clamped(real):
  def mutant(x, y, thr, lower=False):
    a, b, bad = real(x, y, thr, lower)
    # A again, against the truth as it is
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    t = np.asarray(thr).astype(np.float64)
    xs = np.sort(np.where(bad[None], 0.0, x), axis=0)
    yv, tv = np.where(bad, 0.0, y), np.where(bad, 0.0, t)
    clamp = (lambda z: np.where(z > tv, tv, z)) if lower else (
        lambda z: np.where(z < tv, tv, z))
    a = np.zeros(y.shape)
    for m in range(x.shape[0]):
      a = a + np.abs(clamp(xs[m]) - yv)
    a[bad] = 0.0
    return a, b, bad
  return mutant


def _drops_the_first_column_of_a_class_at_a_tile_border(real, cls_at):
  """A host_sums that loses column j where j is a multiple of 64 and the
  class changes there (`cls_at`: the position of col_class in its
  arguments)."""
  def mutant(*args):
    args = list(args)
    cls = np.asarray(args[cls_at])
    truth = np.array(args[4], copy=True)
    n_col = cls.size
    for j in range(64, n_col, 64):
      if cls[j] != cls[j - 1]:
        truth.reshape(-1, n_col)[:, j] = np.nan
    args[4] = truth
    return real(*args)
  return mutant


def _counts_the_invalid_points(real):
  def mutant(*args):
    sums, cnt = real(*args)
    cls, n_class = np.asarray(args[9]), args[10]
    cnt = cnt.copy()
    cnt[..., 2] = np.bincount(cls, minlength=n_class)
    return sums, cnt
  return mutant


def _bins_closed_on_the_right(v, edges):
  """conditional.host_bins with #{k : edges[k] < v}."""
  with np.errstate(invalid='ignore'):
    return (np.asarray(edges, np.float64).reshape(-1, 1) < v[None]
            ).sum(axis=0).astype(np.int64)


def _pool_without_the_wrap(x, windows, kind='mean'):
  """pooling.host_pool with the columns clamped to the row."""
  x = np.asarray(x)
  n_col = x.shape[-1]
  h = max(int(n) // 2 for n in windows)
  padded = np.concatenate([np.repeat(x[..., :1], h, axis=-1), x,
                           np.repeat(x[..., -1:], h, axis=-1)], axis=-1)
  # (the windows of the middle columns never reach the padded row's own wrap)
  out = _REAL_POOL(padded, windows, kind)
  return np.ascontiguousarray(out[..., h:h + n_col])


_REAL_POOL = pooling.host_pool

MUTANTS = {
    'fss-wrap-off-by-one': ('k19', lambda: [
        (neighborhood, '_box', _box_wrap_off_by_one)]),
    'fss-pole-clip': ('k19', lambda: [
        (neighborhood, '_box', _box_pole_clip_one_more)]),
    'event-greater-or-equal': ('k18', lambda: [
        (events, 'host_exceedance', _exceedance_or_equal)]),
    'twcrps-truth-not-clamped': ('k21', lambda: [
        (threshold_weighted, 'host_point_terms',
         _twcrps_truth_not_clamped(threshold_weighted.host_point_terms))]),
    'tile-border-k20': ('k20', lambda: [
        (crps_decomposition, 'host_sums',
         _drops_the_first_column_of_a_class_at_a_tile_border(
             crps_decomposition.host_sums, 9))]),
    'tile-border-k21': ('k21', lambda: [
        (threshold_weighted, 'host_sums',
         _drops_the_first_column_of_a_class_at_a_tile_border(
             threshold_weighted.host_sums, 11))]),
    'tile-border-k24': ('k24', lambda: [
        (conditional, 'host_sums',
         _drops_the_first_column_of_a_class_at_a_tile_border(
             conditional.host_sums, 9))]),
    'crps-count-with-invalid': ('k20', lambda: [
        (crps_decomposition, 'host_sums',
         _counts_the_invalid_points(crps_decomposition.host_sums))]),
    'conditional-edge-side': ('k24', lambda: [
        (conditional, 'host_bins', _bins_closed_on_the_right)]),
    'pool-no-wrap': ('k22', lambda: [
        (pooling, 'host_pool', _pool_without_the_wrap)]),
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_the_cases_catch_a_planted_mutant(name, monkeypatch):
  family, patches = MUTANTS[name]
  for module, attr, mutant in patches():
    monkeypatch.setattr(module, attr, mutant)
  caught = []
  for case in fc.BY_FAMILY[family]:
    try:
      checks.against_definition(case, checks.run(case, device=False))
    except AssertionError:
      caught.append(case.id)
      if len(caught) >= 2:
        break
  assert caught, f'no case of {family} sees {name}'
