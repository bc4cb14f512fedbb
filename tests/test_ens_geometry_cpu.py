"""What the ensemble-reduction geometry sweep (tests/ens_geometry_cases.py, run
on the GPU by test_ens_geometry_gpu.py) reaches, asserted on the CPU from the
plans of its cases: every K3 kernel family with and without NaN skipping, at
every column count, the row-end tile, odd tile counts, segment edges on and
inside tiles, chunks longer than one 64-row block, grids past 32767 slabs, both
layouts and the weight-field instantiations."""
import collections

import pytest

from tests import ens_geometry_cases as eg
from tests import helpers


def family_of(dtype, m, gather, exact):
  """Which K3 instantiation runs (ensemble.hip launch_ens_npad), restated."""
  if m == 50 and not gather:
    return 'exact50'
  if dtype == 'float32':
    if not gather and m in exact:
      return 'exact'
    if 2 <= m <= max(exact):
      return 'hosted_gather' if gather else 'hosted'
    if m == 1:
      return 'f32_m1'
    if m <= 128:
      return 'pad128_gather' if gather else 'pad128'
    return 'stream_f32'
  if m <= 64:
    return 'f64pad_gather' if gather else 'f64pad'
  return 'stream_f64'


@pytest.fixture(scope='module')
def plans():
  from weatherbench2_amd import plan as plan_lib
  out = []
  for case in eg.CASES:
    res = eg.resolve(case)
    pl = plan_lib.build_plan(
        res.lat, res.lon,
        plan_lib.LATLON if case.layout == 'latlon' else plan_lib.LONLAT,
        {k: helpers.to_gpu_region(v) for k, v in res.regions.items()}, 'cpu',
        rows_per_chunk=case.rows_per_chunk)
    assert (pl.n_row, pl.n_col) == (res.n_row, res.n_col)
    out.append((res, pl))
  return out


def _k3(plans):
  return [(r, p) for r, p in plans if r.case.kernel == 'k3']


def test_the_families_are_what_the_dispatch_runs():
  from weatherbench2_amd import build
  exact = {m for m, _ in build.exact_sizes()}
  for case in eg.CASES:
    if case.kernel == 'k3':
      assert family_of(case.dtype, case.n_member, case.gather,
                       exact) == case.family, case.id
  for fam, (_, ms, gather) in eg.FAMILIES.items():
    assert gather == fam.endswith('_gather'), fam
  # 70 gathered members: a second lane of member addresses
  assert any(c.gather and c.n_member > 64 and c.dtype == 'float32'
             for c in eg.CASES if c.kernel == 'k3')


def test_every_n_col_per_family_and_skipna(plans):
  seen = collections.defaultdict(set)
  for res, _ in _k3(plans):
    seen[(res.case.family, res.case.skipna)].add(res.n_col)
  for fam in eg.FAMILIES:
    for skipna in (False, True):
      assert seen[(fam, skipna)] >= set(eg.N_COL), (fam, skipna)


def test_k3t_and_k3e_see_every_n_col(plans):
  seen = collections.defaultdict(set)
  members = set()
  wf = set()
  for res, pl in plans:
    c = res.case
    if c.kernel == 'k3t':
      seen[(c.kernel, c.dtype, c.skipna)].add(res.n_col)
    if c.kernel == 'k3e':
      seen[(c.kernel, c.skipna)].add(res.n_col)
      members.add(c.n_member)
    if c.kernel != 'k3' and pl.wfield is not None:
      wf.add((c.kernel, c.skipna))
  for dtype in ('float32', 'float64'):
    for skipna in (False, True):
      assert seen[('k3t', dtype, skipna)] >= set(eg.N_COL), (dtype, skipna)
  for skipna in (False, True):
    assert seen[('k3e', skipna)] >= set(eg.N_COL), skipna
  assert members >= set(eg.ENERGY_M)
  assert wf >= {(k, s) for k in ('k3t', 'k3e') for s in (False, True)}, wf


def test_row_end_tile_in_every_family_and_odd_tile_counts(plans):
  row_end = collections.defaultdict(bool)
  tiles = set()
  for res, _ in plans:
    key = res.case.family if res.case.kernel == 'k3' else res.case.kernel
    row_end[key] |= res.n_col % eg.T != 0 and res.n_col > eg.T
    tiles.add(-(-res.n_col // eg.T))
  assert all(row_end[f] for f in eg.FAMILIES), dict(row_end)
  assert row_end['k3t'] and row_end['k3e']
  assert {1, 2, 3, 6} <= tiles, tiles
  assert any(n > 2 and n % 2 for n in tiles), tiles


def test_segment_edges_on_inside_and_in_the_last_tile(plans):
  on_edge = inside = last = 0
  for res, pl in plans:
    c = pl.seg_col0_host.astype(int)
    last_tile = (res.n_col - 1) // eg.T * eg.T
    for c0 in c[1:-1]:
      on_edge += c0 % eg.T == 0
      inside += c0 >= eg.T and c0 % eg.T != 0
      last += c0 > last_tile and last_tile > 0
  assert on_edge and inside and last, (on_edge, inside, last)


def test_long_chunks_for_each_two_pass_family(plans):
  """A chunk of more than 64 rows (the skipna loop's second 64-row block) in
  a skipna case of every two-pass family: the GPU test puts NaNs past row 64
  of such chunks, and in both blocks."""
  seen = set()
  for res, pl in _k3(plans):
    if res.case.skipna and (pl.chunk_nrow_host > 64).any():
      seen.add(res.case.family)
  assert seen >= set(eg.TWO_PASS), seen


def test_grid_z_for_every_kernel():
  kernels = {c.kernel for c in eg.CASES if c.slabs == 'zgrid'}
  assert kernels == {'k3', 'k3t', 'k3e'}
  for c in eg.CASES:
    if c.slabs == 'zgrid':
      assert c.n_outer > 32768 and c.n_row == 1 and c.n_col == eg.T + 1


def test_layouts_fields_and_slab_forms(plans):
  layouts = {(r.case.kernel, r.case.layout) for r, _ in plans}
  assert layouts == {(k, l) for k in ('k3', 'k3t', 'k3e')
                     for l in ('latlon', 'lonlat')}
  fields = set()
  for res, pl in plans:
    if pl.wfield is not None:
      fields.add((res.case.kernel, 'f32' if pl.wfield32 is not None
                  else 'f64'))
  assert {('k3', 'f32'), ('k3', 'f64'), ('k3t', 'f32'),
          ('k3t', 'f64')} <= fields, fields
  slabs = {c.slabs for c in eg.CASES if c.kernel == 'k3'}
  assert set(eg.STRIDED_SLABS) | {'gather', 'zgrid'} <= slabs


def test_cases_are_unique_and_small(plans):
  ids = [res.case.id for res, _ in plans]
  assert len(ids) == len(set(ids))
  for res, _ in plans:
    assert res.n_row * res.n_col <= eg.LONG_ROWS * (2 * eg.T + 1), res.case.id
