"""What the rank-histogram sweep (tests/rank_geometry_cases.py, run on the GPU
by test_rank_geometry_gpu.py) reaches, asserted on the CPU: every trip count of
the member loads, every class of bin count against the wave with a last wave of
1, 63 and 64 points, grid.z in all three launch forms, every slab layout in
every form, every stream layout and base offset, every data recipe in both
dtypes under the seeded ties.  Also the plain references of tests/rank_np.py
against hand-written answers, and what the references themselves leave open:
per seeded case at most 5 % of the samples."""
import collections

import numpy as np
import pytest

from tests import rank_geometry_cases as rc
from tests import rank_np

CASES = rc.CASES
OPEN_CAP = 0.05
TINY = np.float32(rc.TINY)


@pytest.fixture(scope='module')
def seeded():
  """expected() of every case under numpy ties, computed once."""
  return {c.id: rc.expected(c) for c in CASES if c.ties == 'numpy'}


def test_constants_come_from_the_source():
  assert rc.GROUPS == (16, 4) and rc.BLOCK == 256 and rc.WAVE == 64
  assert rc.SPLIT == 32768 and rc.ROW_SPLIT == 32768 and rc.MAX_BINS == 256
  src = rc._read(rc.RANK_SRC)
  # what Case restates: the store loop's steps, the LDS bound behind MAX_BINS
  assert 'const int dq = kWave / p.n_bins, dr = kWave % p.n_bins;' in src
  assert 'const size_t lds = (size_t)kWave * n_bins * sizeof(unsigned);' in src
  assert 'WB2_REQUIRE(lds <= 64 * 1024' in src
  assert rc.WAVE * rc.MAX_BINS * 4 == 64 * 1024
  assert rc.BLOCK % rc.WAVE == 0


def test_the_list_is_small_and_unique():
  ids = [c.id for c in CASES]
  assert len(set(ids)) == len(ids)
  assert 200 <= len(CASES) <= 270
  for c in CASES:
    # what a case's reference draws element by element stays small: the large
    # cases are dense in the stream and drawn in one call
    index = rc.make_stream(c).index if c.ties == 'numpy' else None
    if index is not None and index.size > 20000:
      assert int(index.max()) - int(index.min()) + 1 == index.size, c.id
  assert {c.dtype for c in CASES} == set(rc.DTYPES)
  for group in rc.GROUP_NAMES:
    assert {c.dtype for c in CASES if c.group == group} == set(rc.DTYPES)


def test_member_axis():
  members = {c.n_member for c in CASES if c.group == 'members'}
  assert members == set(rc.MEMBERS)
  for m in rc.MEMBERS:
    bins = {c.n_bins for c in CASES if c.group == 'members'
            and c.n_member == m and c.form == 'onehot'}
    assert {1, m + 1} <= bins and bins == set(rc.bins_for(m)), m
    proper = [d for d in range(2, m + 1) if (m + 1) % d == 0]
    assert bool(proper) == bool(bins - {1, m + 1}), m
  assert {min(c.groups16, 2) for c in CASES} == {0, 1, 2}
  seen = {(min(c.groups16, 2), c.groups4, c.tail) for c in CASES}
  assert {g4 for _, g4, _ in seen} == {0, 1, 2, 3}
  assert {t for _, _, t in seen} == {0, 1, 2, 3}
  # every remainder after one whole group of 16, and with none
  for g16 in (0, 1):
    assert {(g4, t) for g, g4, t in seen if g == g16} >= {
        (0, 0) if g16 else (1, 0), (0, 1), (0, 3), (1, 0), (1, 1)}, g16
  assert {4, 16, 20, 32} <= members
  # the exact multiples in every form
  for form in rc.FORMS:
    assert {c.n_member for c in CASES if c.form == form
            and c.tail == 0} & {4, 16, 20, 32}, form


def test_bins_against_the_wave():
  assert {c.n_bins for c in CASES if c.group == 'bins'} == set(rc.WAVE_BINS)
  want = {'1', 'divides', 'below', 'wave', 'above', 'many'}
  onehot = [c for c in CASES if c.form == 'onehot']
  for occupancy in (1, 63, 64):
    got = {c.bin_class for c in onehot if c.last_wave == occupancy}
    assert got == want, occupancy
    assert any(c.n_bins == 256 for c in onehot if c.last_wave == occupancy)
  for nb in rc.WAVE_BINS:
    assert {c.last_wave for c in onehot if c.n_bins == nb} >= {1, 63, 64}, nb
  # store-loop steps: dq = 0 (more bins than lanes), dr = 0 and dr > 0
  assert {(rc.WAVE // c.n_bins == 0, rc.WAVE % c.n_bins == 0)
          for c in onehot} == {(True, False), (False, True), (False, False)}


def test_point_axis():
  pts = {c.n_point for c in CASES if c.group == 'points'}
  assert pts == set(rc.POINTS)
  assert {c.last_wave for c in CASES} >= {1, 2, 63, 64}
  assert {c.waves_per_block for c in CASES} >= {1, 2, 4}
  assert any(c.n_point > rc.BLOCK for c in CASES if c.form == 'onehot')
  for form in rc.FORMS:
    assert {c.last_wave for c in CASES if c.form == form} >= {1, 63, 64}, form


def test_grid_split():
  for form in ('onehot', 'counts'):
    big = [c for c in CASES if c.form == form and c.grid_z > 1]
    assert {c.dtype for c in big} == set(rc.DTYPES), form
    assert all(c.n_outer == rc.SPLIT + 70 and c.n_point == 3 and
               c.n_member == 3 for c in big)
    assert {c.ties for c in big} >= {'numpy', 'first'}
  big = [c for c in CASES if c.form in ('mean', 'sum') and c.grid_z > 1]
  assert {c.dtype for c in big} == set(rc.DTYPES)
  assert {c.form for c in big} == {'mean', 'sum'}
  assert all(c.shape[0] * c.shape[2] == rc.ROW_SPLIT + 5 and c.shape[1] == 2
             and c.n_point == 2 and c.n_member == 1 for c in big)
  assert {c.shape[0] for c in big} == {1, rc.ROW_SPLIT + 5}


def test_mean_kernel_axes():
  for form in ('mean', 'sum'):
    mine = [c for c in CASES if c.form == form]
    assert {c.shape for c in mine if c.group == 'mean'} >= set(rc.MEAN_SHAPES)
    assert any(c.n_bins == rc.MAX_BINS for c in mine)
    assert {c.dtype for c in mine if c.n_bins == rc.MAX_BINS} == set(rc.DTYPES)
    assert {c.ties for c in mine} >= {'first', 'numpy', 'none'}


def test_layouts_and_recipes():
  for form in rc.FORMS:
    assert {c.slab for c in CASES if c.form == form} == set(rc.SLABS), form
  for slab in rc.SLABS:
    assert {c.dtype for c in CASES if c.slab == slab} == set(rc.DTYPES), slab
  seeded_cases = [c for c in CASES if c.ties == 'numpy']
  assert {c.stream for c in seeded_cases} == set(rc.STREAMS)
  for stream in rc.STREAMS:
    assert {c.dtype for c in seeded_cases
            if c.stream == stream} == set(rc.DTYPES), stream
  for name, base in rc.BASES.items():
    for c in (c for c in seeded_cases if c.stream == name):
      s = rc.make_stream(c)
      assert int(s.off.min()) == base and c.n_sample <= 100
      assert int(s.index.max()) < 2**63
  for c in seeded_cases:
    s = rc.make_stream(c)
    # every element has a place of its own in the stream
    assert np.unique(s.index).size == s.index.size, c.id
    if c.stream in ('rowmajor', 'transposed') and c.n_point > 1:
      assert 1 <= c.n_col < c.n_point
  assert any(c.n_col > 1 for c in seeded_cases if c.stream == 'transposed')
  fast = {c.stream == 'member1' for c in seeded_cases}
  assert fast == {True, False}
  for recipe in rc.RECIPES:
    dtypes = {c.dtype for c in seeded_cases if c.recipe == recipe}
    assert dtypes == ({'float32'} if recipe == 'subnormal_gap'
                      else set(rc.DTYPES)), recipe
    assert {c.ties for c in CASES if c.recipe == recipe} >= (
        {'numpy', 'none'} if recipe == 'plain' else {'numpy', 'hash', 'first'})
  uniform = [c for c in CASES if c.group == 'uniform']
  assert {c.n_member for c in uniform} == {1, 2, 3, 4, 5}
  assert all(c.n_sample >= 20000 and c.recipe == 'all_equal' and
             c.ties == 'hash' for c in uniform)


def test_buffers_hold_the_logical_arrays():
  """make_buffers read back the way the kernel addresses them."""
  for c in CASES:
    if c.group != 'slabs':
      continue
    data = rc.make_data(c)
    b = rc.make_buffers(c, data)
    o = np.arange(c.n_outer)
    es = o if b.ens_slab is None else b.ens_slab
    ts = o if b.truth_slab is None else b.truth_slab
    pt = np.arange(c.n_point)
    at = (es[:, None, None] * c.n_point + pt[None, :, None] +
          np.arange(c.n_member)[None, None, :] * b.member_stride)
    assert at.max() < b.ens.size
    np.testing.assert_array_equal(b.ens[at], data.ens)
    np.testing.assert_array_equal(
        b.truth[ts[:, None] * c.n_point + pt[None, :]], data.truth)
    if c.slab == 'padded':
      assert b.member_stride == c.n_outer * c.n_point + rc.PAD
    if c.slab == 'member_inner':
      assert b.member_stride == c.n_point
      np.testing.assert_array_equal(b.ens_slab, o * c.n_member)
    if c.slab == 'shared_truth':
      np.testing.assert_array_equal(b.truth_slab, o // rc.SHARE)
      assert b.truth.size < data.truth.size


# ---- the references against hand-written answers ----------------------------
def test_counts_and_first_rank_by_hand():
  nan, inf = np.nan, np.inf
  ens = np.array([[1, 2, 3], [2, 2, nan], [nan, nan, nan], [inf, -inf, 0],
                  [5, 1, nan]], dtype=np.float32)
  truth = np.array([2.5, 2, nan, inf, nan], dtype=np.float32)
  lo, eq, nn = rank_np.counts(ens, truth)
  np.testing.assert_array_equal(lo, [2, 0, 0, 2, 0])
  np.testing.assert_array_equal(eq, [0, 2, 0, 1, 0])
  np.testing.assert_array_equal(nn, [3, 2, 0, 3, 2])
  np.testing.assert_array_equal(rank_np.first_rank(ens, truth),
                                [2, 0, 0, 2, 2])


def test_bin_of_and_one_hot_by_hand():
  np.testing.assert_array_equal(rank_np.bin_of(np.arange(6), 5, 3),
                                [0, 0, 1, 1, 2, 2])
  np.testing.assert_array_equal(rank_np.bin_of(np.arange(6), 5, 1), [0] * 6)
  np.testing.assert_array_equal(rank_np.bin_of(np.arange(6), 5, 6),
                                np.arange(6))
  np.testing.assert_array_equal(rank_np.bin_of([0, 127, 128, 255], 255, 2),
                                [0, 0, 1, 1])
  with pytest.raises(ValueError):
    rank_np.bin_of([0], 5, 4)
  hot = rank_np.one_hot(np.array([2, 0, 1, 1]), 3)
  assert hot.dtype == np.float64
  np.testing.assert_array_equal(hot, [[0, 0, 1], [1, 0, 0], [0, 1, 0],
                                      [0, 1, 0]])
  np.testing.assert_array_equal(rank_np.sum_over(hot, 0), [1, 2, 1])
  third = rank_np.mean_over(hot[:3], 0)
  np.testing.assert_array_equal(third, [1 / 3, 1 / 3, 1 / 3])
  np.testing.assert_array_equal(rank_np.mean_over(hot, 0), [0.25, 0.5, 0.25])


def test_perturbation_size_by_hand():
  nan, inf = np.nan, np.inf
  f32 = np.float32
  v = np.array([[0, 0, 1], [1, 1, 1], [nan, 0, 1], [inf, inf, 0], [inf, 0, 3],
                [-inf, 5, 5], [0.5, 0.75, 0.5]])
  for dtype in (np.float32, np.float64):
    size = rank_np.perturbation_size(v, dtype)
    assert size.dtype == dtype
    np.testing.assert_array_equal(size[:, 0], [0.5, 1, 1, 1, 1.5, 1, 0.125])
  # in float32 half an odd subnormal gap is rounded (to even)
  gaps = np.array([[0, 4], [0, 5], [0, 6], [0, 7], [3, 67]]) * TINY
  np.testing.assert_array_equal(
      rank_np.perturbation_size(gaps, np.float32)[:, 0],
      np.array([2, 2, 3, 4, 32], dtype=f32) * TINY)
  np.testing.assert_array_equal(
      rank_np.perturbation_size(gaps, np.float32, np.float64)[:, 0],
      np.array([2, 2.5, 3, 3.5, 32]) * float(TINY))
  # a gap beyond the float32 range is infinite there: no positive gap left
  wide = np.array([[-3e38, 3e38, 3e38]])
  assert rank_np.perturbation_size(wide, np.float32)[0, 0] == 1
  assert rank_np.perturbation_size(wide, np.float64)[0, 0] == 3e38


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_numpy_rank_is_the_reference_on_a_whole_array(dtype):
  """The reference perturbs the whole concatenated array with one uniform()
  call and sorts along the ensemble axis; numpy_rank, given each element's
  C-order index in that array, does the same sample by sample -- for the
  ensemble axis last, first and in the middle."""
  rs = np.random.RandomState(3)
  n, m1 = 40, 5
  values = (np.round(rs.standard_normal((n, m1)) * 2) / 2).astype(dtype)
  values[3, 2] = np.nan
  values[5, 0] = np.nan
  values[7, 1] = values[7, 3] = np.inf
  for seed, axis, shape in ((5, 1, (n, m1)), (802701, 0, (m1, n)),
                            (0, 1, (8, m1, 5))):
    da = np.moveaxis(values.reshape(8, 5, m1), -1, axis).reshape(shape) if (
        len(shape) == 3) else (values if axis == 1 else values.T.copy())
    # the reference, restated on the whole array
    with np.errstate(invalid='ignore'):
      diffs = np.diff(np.sort(da, axis=axis), axis=axis)
      diffs = np.where(diffs == 0, np.inf, diffs)
      min_diff = diffs.min(axis=axis, keepdims=True)
      size = np.where(min_diff < np.inf, min_diff / 2, 1)
      perturbed = da + np.random.default_rng(seed).uniform(
          size=da.shape, low=-size / 2, high=size / 2)
    want = np.argsort(perturbed, axis=axis).argmin(axis=axis)
    index = np.arange(da.size).reshape(da.shape)
    rank, mine = rank_np.numpy_rank(np.moveaxis(da, axis, -1),
                                    np.moveaxis(index, axis, -1), seed, dtype)
    np.testing.assert_array_equal(mine, np.moveaxis(perturbed, axis, -1))
    sure = ~rank_np.ambiguous(mine)
    assert sure.mean() > 0.9
    np.testing.assert_array_equal(rank[sure], want[sure])


def test_numpy_rank_by_hand_and_far_along_the_stream():
  # truth 0 tied with member 0, the other member 1 away: size 1/2, draws in
  # +-1/4 from positions 30, 31, 32 of default_rng(5)
  u = np.random.default_rng(5).uniform(-0.25, 0.25, size=40)[30:33]
  rank, perturbed = rank_np.numpy_rank(
      np.array([[0.0, 0.0, 1.0]]), np.array([[30, 31, 32]]), 5, np.float64)
  np.testing.assert_array_equal(perturbed[0], np.array([0, 0, 1]) + u)
  assert rank[0] == int(u[1] < u[0])
  # the same draws one by one (a span too wide to draw at once), and a jump
  # beyond 2**32: the advanced generator continues an ordinary stream
  far = 2**33 + 7
  bg = np.random.PCG64(5)
  bg.advance(far)
  want = np.random.Generator(bg).uniform(-0.25, 0.25, size=3)
  index = np.array([[far, far + 1, far + 2], [30, 31, 32]])
  rank, perturbed = rank_np.numpy_rank(
      np.array([[0.0, 0.0, 1.0]] * 2), index, 5, np.float64)
  np.testing.assert_array_equal(perturbed[0], np.array([0, 0, 1]) + want)
  np.testing.assert_array_equal(perturbed[1], np.array([0, 0, 1]) + u)
  np.testing.assert_array_equal(rank, [int(want[1] < want[0]),
                                       int(u[1] < u[0])])


def test_ambiguous_and_bounds_by_hand():
  nan = np.nan
  p = np.array([[1, 1, 2], [nan, nan, 0], [nan, 1, 2], [1, 2, 3],
                [1, 1, 0.5], [np.inf, np.inf, 0]])
  np.testing.assert_array_equal(rank_np.ambiguous(p),
                                [True, True, False, False, True, True])
  less, equal = rank_np.perturbed_bounds(p)
  np.testing.assert_array_equal(less, [0, 1, 2, 0, 1, 1])
  np.testing.assert_array_equal(equal, [1, 1, 0, 0, 1, 1])


# ---- what the data does -----------------------------------------------------
def test_the_references_leave_few_samples_open(seeded):
  """A cap, not a measurement: the share of samples whose order the reference
  itself leaves open, from the reference alone, per seeded case."""
  worst = collections.defaultdict(float)
  for c in CASES:
    if c.ties != 'numpy':
      continue
    e = seeded[c.id]
    share = e.open.mean()
    worst[(c.recipe, c.n_member)] = max(worst[(c.recipe, c.n_member)], share)
    assert share <= OPEN_CAP, (c.id, share)
    # there the kernel is held to the bounds, which must themselves be sound
    assert (e.less <= e.rank).all() and (e.rank <= e.less + e.equal).all()
    sure = ~e.open
    np.testing.assert_array_equal(e.rank[sure], e.less[sure])
    if c.form != 'onehot':
      # sums of one-hots are compared exactly: nothing may be open
      assert not e.open.any(), c.id
  # the NaN and infinity rates reach the large ensembles
  assert (('specials', 255) in worst and ('specials', 50) in worst and
          ('specials', 1) in worst and ('specials', 7) in worst)


def test_the_data_really_ties(seeded):
  for c in CASES:
    e = seeded[c.id] if c.ties == 'numpy' else rc.expected(c)
    tied = (e.eq > 0).mean()
    if c.recipe == 'plain':
      assert tied == 0, c.id
    if c.recipe in ('quantised', 'specials') and c.n_sample >= 100:
      assert tied > 0.2, (c.id, tied)
    if c.recipe == 'all_equal':
      assert (e.eq == c.n_member).all()
    if c.recipe == 'specials' and c.n_sample >= 500:
      t = e.data.truth
      assert np.isnan(t).any() and (t == np.inf).any() and (t == -np.inf).any()
      assert np.isnan(e.data.ens).any() and np.isinf(e.data.ens).any()
    if c.recipe == 'one_ulp':
      assert 0 < tied < 0.05
      gap = np.abs(e.data.ens - e.data.truth[..., None])
      ulp = np.spacing(np.abs(e.data.truth))[..., None]
      assert (gap <= 3 * ulp).all() and (gap[e.eq == 0] > 0).all()
    if c.recipe == 'subnormal_gap':
      v = np.concatenate([e.data.truth[..., None], e.data.ens], -1)
      d = np.diff(np.sort(v.astype(np.float64), -1), axis=-1)
      smallest = np.where(d > 0, d, np.inf).min(-1) / float(TINY)
      gaps = smallest[np.isfinite(smallest)]
      assert gaps.min() >= 4 and gaps.size > 0.25 * smallest.size
      assert (gaps <= 64).mean() > 0.6, c.id
      assert tied > 0.2


def test_subnormal_gaps_can_tell_the_size_dtype(seeded):
  """The perturbation's size only scales the draws, so between tied values the
  order is that of the draws whatever the size -- unless the float64 sum
  rounds the perturbed values to a few levels.  The subnormal_gap recipe has
  such samples: on them a size computed in float64 (2.5 instead of 2 smallest
  subnormals) gives another rank than the float32 size the reference uses,
  where the reference's own order is not open."""
  c, = [c for c in CASES if c.recipe == 'subnormal_gap' and c.ties == 'numpy'
        and c.n_sample >= 4000]
  e = seeded[c.id]
  v = np.concatenate([e.data.truth[..., None], e.data.ens], -1)
  other, _ = rank_np.numpy_rank(v, e.stream.index, c.seed, np.float32,
                                size_dtype=np.float64)
  differ = (other != e.rank) & ~e.open
  assert differ.sum() >= 5, differ.sum()


def test_hash_cases_share_their_data_across_slab_layouts():
  pairs = collections.defaultdict(list)
  for c in CASES:
    if c.group == 'slabs' and c.ties == 'hash':
      pairs[c.dtype].append(c)
  assert set(pairs) == set(rc.DTYPES)
  for a, b in pairs.values():
    assert {a.slab, b.slab} == {'identity', 'permuted'}
    da, db = rc.make_data(a), rc.make_data(b)
    np.testing.assert_array_equal(da.ens, db.ens)
    np.testing.assert_array_equal(da.truth, db.truth)
    tb = rc.make_buffers(b, db)
    assert (tb.ens_slab != np.arange(b.n_outer)).any()
    assert (tb.ens_slab != tb.truth_slab).any()
