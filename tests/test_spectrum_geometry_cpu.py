"""What the spectrum geometry sweep (tests/spectrum_geometry_cases.py, run on
the GPU by test_spectrum_geometry_gpu.py) reaches, asserted on the CPU: every
instantiated length of K4f in both dtypes and all three modes, output-row
counts on both sides of the persistent grid, the 16-bit sample counts of the
fused time mean and the step count past them, every kind of latitude split,
and the hipFFT path's transforms and power_kernel loops."""
import collections
import re

from tests import spectrum_geometry_cases as sc

CASES = sc.CASES


def test_constants_come_from_the_source():
  with open(sc._SRC) as f:
    src = f.read()
  assert len(sc.FUSED_N2) == 22 and len(set(sc.FUSED_N2)) == 22
  assert 720 in sc.FUSED_N2 and 1800 in sc.FUSED_N2
  # the dispatch and the launch cap that the cases are built around
  assert 'blocks = WB2_FFT_MAX_BLOCKS * 4 / WB2_FFT_NWAVE' in src
  assert re.search(r'stride = \(long long\)gridDim\.x \* NWAVE', src)
  assert sc.WAVES == 8192, sc.WAVES


def test_the_time_switch_is_where_the_cases_put_it():
  """wb2_zonal_spectrum takes K4f up to n_time = 65535 (spectrum.hip)."""
  with open(sc._SRC.replace('spectrum_fused.hip', 'spectrum.hip')) as f:
    src = f.read()
  assert re.search(r'% 16 == 0 && n_time < 65536\)', src)
  assert sc.MAX_FUSED_TIME == 65535


def test_every_length_in_both_dtypes_and_every_fused_mode():
  seen = collections.defaultdict(set)
  for c in CASES:
    if c.fused:
      key = c.mode if c.mode != 'time' else ('time', c.skipna)
      seen[key].add((c.n_lon, c.dtype))
  want = {(n, d) for n in sc.FUSED_N_LON for d in ('float32', 'float64')}
  for key in ('mat', ('time', False), ('time', True), 'latseg'):
    assert seen[key] >= want, (key, sorted(want - seen[key]))


def test_output_row_counts_in_every_mode():
  seen = collections.defaultdict(set)
  for c in CASES:
    if c.fused and c.rows_out is not None:
      seen[(c.mode, c.n_lon, c.dtype)].add(c.rows_out)
  for n_lon, dtype in sc.ROW_LENGTHS:
    for mode in ('mat', 'time', 'latseg'):
      assert seen[(mode, n_lon, dtype)] >= set(sc.ROWS_OUT), (mode, n_lon)
  assert {1, 2, 3, 5, 8191, 8192, 8193, 16385} <= set(sc.ROWS_OUT)
  # past one task per wave at the long rows, float32 and float64
  big = {(c.n_lon, c.dtype) for c in CASES
         if c.fused and (c.rows_out or 0) > sc.WAVES}
  assert {(1440, 'float32'), (3600, 'float32')} <= big, big
  assert any(d == 'float64' and n >= 1440 for n, d in big), big


def test_time_steps_and_the_16_bit_counts():
  fused_t = collections.defaultdict(set)
  for c in CASES:
    if c.mode == 'time' and c.fused:
      fused_t[c.n_time].add(c.skipna)
  for nt in (1, 2, 5, 65535):
    assert fused_t[nt] == {False, True}, nt
  full = [c for c in CASES if c.mode == 'time' and c.n_time == 65535]
  assert all(c.n_lat == 1 and c.n_lon == 64 for c in full)
  # every count field full: no NaN in some of them
  assert any(not c.nan for c in full) and any(c.nan for c in full)
  late = [c for c in CASES if c.mode == 'time' and c.n_time == 65536]
  assert late and all(not c.fused and c.n_lon // 2 in sc.FUSED_N2
                      for c in late)
  assert {c.skipna for c in late} == {False, True}


def test_nan_rows_with_and_without_skipna():
  seen = {(c.skipna, c.fused) for c in CASES
          if c.mode == 'time' and c.nan and c.n_time >= 2 and
          c.rows_out >= 4}
  assert seen == {(s, f) for s in (False, True) for f in (False, True)}, seen


def test_latitude_splits():
  lats = {c.n_lat for c in CASES if c.mode == 'latseg'}
  assert {1, 2, 7, 721} <= lats, lats
  kinds = collections.defaultdict(set)
  for c in CASES:
    if c.mode != 'latseg':
      continue
    s, n = c.n_seg, c.n_lat
    if s == 'auto':
      kinds[n].add('auto')
      continue
    if s == 1:
      kinds[n].add('one')
    if s == 2:
      kinds[n].add('two')
    if s == n - 1:
      kinds[n].add('n_lat-1')
    if s == n:
      kinds[n].add('n_lat')
    if n % s and all(s % p for p in range(2, s)):
      kinds[n].add('prime')
  for n in (7, 721):
    assert kinds[n] == {'one', 'two', 'n_lat-1', 'n_lat', 'auto', 'prime'}, (
        n, kinds[n])
  assert {'one', 'two', 'n_lat-1', 'n_lat', 'auto'} <= kinds[2]
  assert {'one', 'n_lat', 'auto'} <= kinds[1]
  # segments of unequal length, and tasks that a prefetch takes into another
  # field (a wave's next task is WAVES tasks on)
  assert any(c.mode == 'latseg' and isinstance(c.n_seg, int) and
             c.n_lat % c.n_seg for c in CASES)
  assert any(c.mode == 'latseg' and (c.rows_out or 0) > sc.WAVES and
             c.n_seg < sc.WAVES for c in CASES)
  assert {c.scale for c in CASES if c.mode == 'latseg'} >= set(sc.SCALES)
  assert len([c for c in CASES if c.mode == 'latseg' and c.n_lat >= 3]) > 10


def test_the_hipfft_path():
  hip = [c for c in CASES if not c.fused]
  assert all(c.mode in ('mat', 'time') for c in hip)
  # odd: real-to-complex, with an even and an odd bin count
  odd = {(c.dtype, c.n_bins % 2) for c in hip if c.n_lon % 2}
  assert {('float32', 0), ('float64', 1)} <= odd, odd
  # even lengths K4f has no plan for: power_kernel's paired (n_lon/2 even)
  # and scalar (odd) loops, float32 and float64
  packed = {(c.n_lon // 2 % 2, c.dtype) for c in hip
            if c.n_lon % 2 == 0 and c.n_lon // 2 not in sc.FUSED_N2}
  assert {(0, 'float32'), (1, 'float32'), (0, 'float64')} <= packed, packed
  offsets = {c.offset for c in hip if c.n_lon // 2 in sc.FUSED_N2}
  assert {4, 8} <= offsets
  assert any(c.rows_out > 65536 for c in hip)
  for c in hip:
    assert {h.mode for h in hip if (h.dtype, h.n_lon, h.n_rows) ==
            (c.dtype, c.n_lon, c.n_rows)} >= {'time'}
  # about 8 distinct plans, each one's cases together
  plans = [(c.dtype, c.n_lon, c.n_rows) for c in CASES if not c.fused]
  assert len(set(plans)) <= 8, sorted(set(plans))
  runs = [p for i, p in enumerate(plans) if i == 0 or plans[i - 1] != p]
  assert len(runs) == len(set(runs)), runs


def test_cases_are_unique_and_bounded():
  ids = [c.id for c in CASES]
  assert len(ids) == len(set(ids))
  for c in CASES:
    assert c.n_rows * c.n_lon * (4 if c.dtype == 'float32' else 8) <= 2 ** 27
    if c.mode == 'latseg':
      assert c.n_seg == 'auto' or 1 <= c.n_seg <= c.n_lat
      assert c.fused
