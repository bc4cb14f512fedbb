"""What the streaming-reduction geometry sweep (tests/stream_geometry_cases.py,
run on the GPU by test_stream_geometry_gpu.py) reaches, asserted on the CPU
from the plans of its cases: every tile, row-end and segment edge that K1, K1p
and the K2 fold (csrc/reduce_common.hpp fold_tile_to_segs, plan.seg_entries)
have to get right."""
import collections

import numpy as np
import pytest

from tests import helpers
from tests import stream_geometry_cases as sg


@pytest.fixture(scope='module')
def lib():
  from weatherbench2_amd import build
  build.build(verbose=False)
  from weatherbench2_amd import _lib
  return _lib.load()


@pytest.fixture(scope='module')
def plans(lib):
  from weatherbench2_amd import plan as plan_lib
  out = []
  for case in sg.CASES:
    res = sg.resolve(lib, case)
    pl = plan_lib.build_plan(
        res.lat, res.lon,
        plan_lib.LATLON if case.layout == 'latlon' else plan_lib.LONLAT,
        {k: helpers.to_gpu_region(v) for k, v in res.regions.items()}, 'cpu',
        rows_per_chunk=case.rows_per_chunk or plan_lib.DEFAULT_ROWS_PER_CHUNK)
    assert (pl.n_row, pl.n_col) == (res.n_row, res.n_col)
    out.append((res, pl))
  return out


def _tiles(res, pl):
  """(launch tile width, tile count, [(c0, c1)] segments)."""
  tile = 64 * sg.launch_vec(res)
  c = pl.seg_col0_host.astype(int)
  return tile, -(-res.n_col // tile), list(zip(c[:-1], c[1:]))


def test_every_residue_of_n_col_mod_vec_for_both_dtypes(plans):
  seen = collections.defaultdict(set)
  vec = {}
  for res, _ in plans:
    seen[res.case.dtype].add(res.n_col % res.vec)
    vec[res.case.dtype] = res.vec
  assert set(seen) == {'float32', 'float64'}
  for dtype, residues in seen.items():
    assert residues == set(range(vec[dtype])), (dtype, residues)


def test_the_row_end_shift_back_crosses_a_tile_edge(plans):
  hits = []
  for res, _ in plans:
    v = sg.launch_vec(res)
    tile = 64 * v
    k = (res.n_col - 1) // tile
    if v > 1 and k >= 1 and res.n_col - v < k * tile:
      hits.append((res.case.dtype, res.n_col))
  assert {d for d, _ in hits} == {'float32', 'float64'}, hits


def test_segment_edges_on_and_inside_later_tiles(plans):
  on_edge = inside = 0
  for res, pl in plans:
    tile, _, segs = _tiles(res, pl)
    for c0, _ in segs:
      if c0 >= tile and c0 % tile == 0:
        on_edge += 1
      if c0 >= tile and c0 % tile != 0:
        inside += 1
  assert on_edge > 0 and inside > 0, (on_edge, inside)


def test_segments_over_three_tiles_and_tiles_with_three_segments(plans):
  long_seg = crowded = False
  for res, pl in plans:
    tile, n_tile, segs = _tiles(res, pl)
    long_seg |= any((c1 - 1) // tile - c0 // tile + 1 >= 3 for c0, c1 in segs)
    per_tile = collections.Counter()
    for c0, c1 in segs:
      for k in range(c0 // tile, (c1 - 1) // tile + 1):
        per_tile[k] += 1
    crowded |= max(per_tile.values()) >= 3
    # the host's entry table agrees with the tiles each segment touches
    eoff, n_ts = pl.seg_entries(tile)
    assert n_ts == sum(per_tile.values())
    assert np.array_equal(
        np.diff(eoff.numpy()),
        [(c1 - 1) // tile - c0 // tile + 1 for c0, c1 in segs])
  assert long_seg and crowded


def test_tile_counts_including_odd_ones_above_two(plans):
  counts = {_tiles(res, pl)[1] for res, pl in plans}
  assert {1, 2, 3, 4, 6} <= counts, counts
  assert any(c > 2 and c % 2 for c in counts), counts


def test_chunk_row_counts(plans):
  rows = set()
  for _, pl in plans:
    rows |= set(pl.chunk_nrow_host[pl.chunk_nrow_host > 0].tolist())
  assert {1, 3, 7, 9} <= rows, rows


def test_float32_and_float64_only_weight_fields(plans):
  kinds = set()
  for res, pl in plans:
    if pl.wfield is None:
      continue
    if pl.wfield32 is not None:
      # the float32 field is read by float32 launches only
      kinds.add('f32' if res.case.dtype == 'float32' else 'f32-unused')
    else:
      kinds.add('f64')
  assert {'f32', 'f64'} <= kinds, kinds


def test_cases_are_unique_and_small(plans):
  ids = [res.case.id for res, _ in plans]
  assert len(ids) == len(set(ids))
  for res, _ in plans:
    assert res.n_row <= 37 and res.n_col <= 5 * res.tile + 3
