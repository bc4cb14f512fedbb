"""The geometry sweep of the zonal energy spectrum: K4f (fused_spectrum_kernel
in its MATERIALISE, TIME_MEAN and LATSEG modes, plus latseg_combine_kernel) and
the hipFFT path of spectrum.hip (rocFFT, then power_kernel).

One case list for test_spectrum_geometry_gpu.py, which runs it against a plain
float64 reference, and test_spectrum_geometry_cpu.py, which asserts on the CPU
that the list reaches every length, output-row count, time-step count, segment
split and hipFFT loop it is meant to reach.

K4f's geometry is read from its source, so the cases cannot drift from it: the
instantiated half-lengths (WB2_FUSED_SIZES), the waves per workgroup
(WB2_FFT_NWAVE) and the cap on workgroups (WB2_FFT_MAX_BLOCKS, counted in
4-wave workgroups).  A wave owns output rows o, o + WAVES, o + 2 WAVES, ... and
prefetches the task of the next one.
"""
import dataclasses
import os
import re
import typing as t

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    'weatherbench2_amd', 'csrc', 'spectrum_fused.hip')


def _source_constants():
  with open(_SRC) as f:
    src = f.read()
  body = re.search(r'#define WB2_FUSED_SIZES\(X\)\s*\\\n((?:.*\\\n)*.*)\n',
                   src).group(1)
  sizes = tuple(int(v) for v in re.findall(r'X\((\d+)\)', body))
  nwave = int(re.search(r'#define WB2_FFT_NWAVE (\d+)', src).group(1))
  blocks = int(re.search(r'#define WB2_FFT_MAX_BLOCKS (\d+)', src).group(1))
  return sizes, nwave, blocks


FUSED_N2, NWAVE, MAX_BLOCKS = _source_constants()
FUSED_N_LON = tuple(2 * n for n in FUSED_N2)
# waves of the largest grid: launch() caps it at MAX_BLOCKS * 4 / NWAVE
# workgroups of NWAVE waves; each wave then strides by WAVES output rows
WAVES = MAX_BLOCKS * 4 // NWAVE * NWAVE
MAX_FUSED_TIME = 65535  # the fused time mean counts samples in 16 bits

# output-row counts: a partly idle last workgroup, both sides of one task per
# wave, and a third task for some waves
ROWS_OUT = (1, 2, 3, 5, WAVES - 1, WAVES, WAVES + 1, 2 * WAVES + 1)
# (n_field, n_lat) of each row count for the per-row modes (rows = n_field *
# n_lat; WAVES - 1 = 8191 is prime: one field of 8191 latitudes)
_ROW_GEOMETRY = {1: (1, 1), 2: (1, 2), 3: (1, 3), 5: (1, 5),
                 WAVES - 1: (1, WAVES - 1), WAVES: (WAVES // 16, 16),
                 WAVES + 1: (3, (WAVES + 1) // 3),
                 2 * WAVES + 1: ((2 * WAVES + 1) // 5, 5)}
# (n_field, n_lat, n_seg) of each row count (n_field * n_seg) for LATSEG;
# WAVES + 1 = 3 x 2731 segments of 2800 latitudes are of unequal length
_SEG_GEOMETRY = {1: (1, 7, 1), 2: (1, 7, 2), 3: (1, 3, 3), 5: (1, 7, 5),
                 WAVES - 1: (1, WAVES - 1, WAVES - 1), WAVES: (WAVES // 2, 7, 2),
                 WAVES + 1: (3, 2800, (WAVES + 1) // 3),
                 2 * WAVES + 1: ((2 * WAVES + 1) // 5, 7, 5)}
ROW_LENGTHS = ((64, 'float32'), (96, 'float32'), (128, 'float64'))


@dataclasses.dataclass(frozen=True)
class Case:
  mode: str              # 'mat' | 'time' | 'latseg'
  dtype: str
  n_lon: int
  n_lat: int
  n_field: int           # rows: [n_time,] n_field, n_lat (time leading)
  n_time: int = 0        # time: time steps averaged
  skipna: bool = False   # time
  nan: bool = False      # time: a row NaN at one step, a row NaN at every step
                         # (test_spectrum_geometry_gpu.make_inputs)
  n_seg: t.Union[int, str] = 0  # latseg: segments per field, or 'auto'
  scale: float = 1.0     # latseg
  offset: int = 0        # bytes past a 256-byte boundary where x starts

  @property
  def n_rows(self):
    """Input rows (the plan's batch)."""
    return max(self.n_time, 1) * self.n_field * self.n_lat

  @property
  def fused(self):
    """Whether wb2_zonal_spectrum runs K4f (else rocFFT + power_kernel)."""
    return (self.n_lon % 2 == 0 and self.n_lon // 2 in FUSED_N2 and
            self.offset % 16 == 0 and self.n_time <= MAX_FUSED_TIME)

  @property
  def rows_out(self):
    """Output rows as the kernel counts them (LATSEG: (field, segment) tasks;
    None where the library picks n_seg)."""
    if self.mode == 'latseg':
      return None if self.n_seg == 'auto' else self.n_field * self.n_seg
    return self.n_field * self.n_lat

  @property
  def n_bins(self):
    return self.n_lon // 2 + 1

  @property
  def id(self):
    s = f'{self.mode}-{self.dtype}-L{self.n_lon}-lat{self.n_lat}-f{self.n_field}'
    if self.mode == 'time':
      s += f'-t{self.n_time}-{"skipna" if self.skipna else "strict"}'
      s += '-nan' if self.nan else ''
    if self.mode == 'latseg':
      s += f'-seg{self.n_seg}-s{self.scale:g}'
    return s + (f'-off{self.offset}' if self.offset else '')


def prime_not_dividing(n):
  """The smallest prime >= 3 below n that does not divide n (None if none)."""
  for p in (3, 5, 7, 11, 13, 17, 19, 23):
    if p < n and n % p:
      return p
  return None


def seg_choices(n_lat):
  """n_seg values of a latitude count: 1, 2, n_lat - 1, n_lat, the library's
  pick and a prime that leaves segments of unequal length."""
  out = [1, 2, n_lat - 1, n_lat, 'auto', prime_not_dividing(n_lat)]
  seen, keep = set(), []
  for s in out:
    if s is not None and s not in seen and (s == 'auto' or 1 <= s <= n_lat):
      seen.add(s)
      keep.append(s)
  return keep


SCALES = (1.0, 0.37, 2.5)


def _every_length():
  """Every instantiated length in both dtypes and every fused mode, on small
  and varied geometry."""
  out = []
  i = 0
  mat_geo = ((1, 1), (1, 2), (1, 3), (1, 5), (2, 3), (3, 1))
  time_geo = ((1, 1, 1), (2, 1, 3), (5, 2, 2), (3, 1, 5), (2, 3, 1))
  for n_lon in FUSED_N_LON:
    for dtype in ('float32', 'float64'):
      nf, nl = mat_geo[i % len(mat_geo)]
      out.append(Case('mat', dtype, n_lon, nl, nf))
      for skipna in (False, True):
        nt, nf, nl = time_geo[(i + skipna) % len(time_geo)]
        out.append(Case('time', dtype, n_lon, nl, nf, n_time=nt, skipna=skipna,
                        nan=True))
      nl = (1, 2, 7)[i % 3]
      segs = seg_choices(nl)
      out.append(Case('latseg', dtype, n_lon, nl, (1, 3)[i % 2],
                      n_seg=segs[i % len(segs)], scale=SCALES[i % 3]))
      i += 1
  return out


def _row_counts():
  """Every output-row count of ROWS_OUT in each mode at a few cheap lengths."""
  out = []
  for n_lon, dtype in ROW_LENGTHS:
    for j, rows in enumerate(ROWS_OUT):
      nf, nl = _ROW_GEOMETRY[rows]
      out.append(Case('mat', dtype, n_lon, nl, nf))
      out.append(Case('time', dtype, n_lon, nl, nf, n_time=2,
                      skipna=bool(j % 2), nan=True))
      nf, nl, ns = _SEG_GEOMETRY[rows]
      out.append(Case('latseg', dtype, n_lon, nl, nf, n_seg=ns,
                      scale=SCALES[j % 3]))
  # long rows past one task per wave
  r = WAVES + 1
  out.append(Case('mat', 'float32', 1440, _ROW_GEOMETRY[r][1],
                  _ROW_GEOMETRY[r][0]))
  out.append(Case('time', 'float32', 3600, _ROW_GEOMETRY[r][1],
                  _ROW_GEOMETRY[r][0], n_time=1, skipna=True, nan=True))
  nf, nl, ns = _SEG_GEOMETRY[r]
  out.append(Case('latseg', 'float32', 3600, nl, nf, n_seg=ns, scale=0.37))
  out.append(Case('latseg', 'float64', 1440, nl, nf, n_seg=ns, scale=2.5))
  return out


def _time_steps():
  """The fused time mean at every 16-bit count, and the first step count
  past it (the hipFFT path: rocFFT through a plan made late)."""
  out = []
  for nt in (1, 2, 5):
    for skipna in (False, True):
      out.append(Case('time', 'float32', 96, 3, 2, n_time=nt, skipna=skipna,
                      nan=True))
  out.append(Case('time', 'float32', 64, 1, 1, n_time=MAX_FUSED_TIME))
  out.append(Case('time', 'float32', 64, 1, 1, n_time=MAX_FUSED_TIME,
                  skipna=True))
  out.append(Case('time', 'float32', 64, 1, 2, n_time=MAX_FUSED_TIME,
                  skipna=True, nan=True))
  return out


def _latitude_segments():
  """Every n_seg of seg_choices at 1, 2, 7 and 721 latitudes; many fields of
  short segments put a wave's prefetched task into another field."""
  out = []
  j = 0
  for n_lat, n_lon, dtype, n_field in ((1, 64, 'float32', 2),
                                       (2, 96, 'float64', 3),
                                       (7, 240, 'float32', 3),
                                       (721, 1440, 'float32', 2),
                                       (721, 256, 'float64', 1)):
    for s in seg_choices(n_lat):
      out.append(Case('latseg', dtype, n_lon, n_lat, n_field, n_seg=s,
                      scale=SCALES[j % 3]))
      j += 1
  return out


# The hipFFT path, grouped by plan (dtype, n_lon, n_rows): every plan costs a
# rocFFT compile of seconds, and the engine's cache holds 8 of them.
HIPFFT_PLANS = (
    # odd lengths: rocFFT's real-to-complex transform, power_kernel unpacked
    # (38 bins: all in pairs; 39 bins: pairs and one more)
    ('float32', 75, ((1, 5, 3), (3, 5, 1), (5, 3, 1))),
    ('float64', 77, ((1, 7, 2), (2, 7, 1), (7, 1, 2))),
    # even lengths K4f has no plan for: n_lon / 2 = 18 (power_kernel's paired
    # loop, and 65540 output rows: a 2-D grid) and 45 (its scalar loop)
    ('float32', 36, ((1, 5, 13108), (4, 5, 3277), (2, 5, 6554))),
    ('float32', 90, ((1, 3, 4), (3, 2, 2), (4, 3, 1))),
    ('float64', 100, ((1, 3, 4), (3, 2, 2), (4, 3, 1))),
)
HIPFFT_OFFSET_PLANS = (
    # instantiated lengths whose rows do not start on 16 bytes: late plans
    ('float32', 240, 4, ((1, 4, 3), (3, 2, 2), (2, 3, 2))),
    ('float64', 128, 8, ((1, 4, 3), (3, 2, 2), (2, 3, 2))),
)


def _hipfft():
  """(n_time, n_lat, n_field) of each plan's calls: n_time = 1 materialises,
  otherwise the time mean, strict and with NaN rows skipped."""
  out = []
  for dtype, n_lon, calls in HIPFFT_PLANS:
    for nt, nl, nf in calls:
      if nt == 1:
        out.append(Case('mat', dtype, n_lon, nl, nf))
        continue
      for skipna in (False, True):
        out.append(Case('time', dtype, n_lon, nl, nf, n_time=nt,
                        skipna=skipna, nan=skipna))
  for dtype, n_lon, off, calls in HIPFFT_OFFSET_PLANS:
    for nt, nl, nf in calls:
      if nt == 1:
        out.append(Case('mat', dtype, n_lon, nl, nf, offset=off))
      else:
        out.append(Case('time', dtype, n_lon, nl, nf, n_time=nt,
                        skipna=nt % 2 == 1, nan=True, offset=off))
  for skipna in (False, True):
    out.append(Case('time', 'float32', 64, 1, 1, n_time=MAX_FUSED_TIME + 1,
                    skipna=skipna, nan=skipna))
  return out


def _cases():
  fused = (_every_length() + _row_counts() + _time_steps() +
           _latitude_segments())
  out, seen = [], set()
  for c in fused + _hipfft():
    if c.id not in seen:
      seen.add(c.id)
      out.append(c)
  return out


CASES = _cases()
