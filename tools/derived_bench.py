"""The derived-variable kernels alone (csrc/derived_fields.hip) at the size of
one 13-level unit, 13 x 721 x 1440 points, over a pool of distinct units much
larger than the 256 MiB Infinity Cache (no re-use between launches).

  python tools/derived_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/derived_bench.py --reps 20

One JSON line per kernel: ms per launch (a HIP event pair around every launch,
median and min), GB/s of the ALGORITHMIC bytes per point (every input once +
the output once, in their dtypes) and that as a share of 8 TB/s.  The
project's own plain map (wb2_spatial_maps, all three maps) runs in the same
call as the yardstick, and `torch.sqrt(u * u + v * v)` on the WindSpeed
tensors.  A last line checks that the resource report of the build shows no
scratch (CPU side; needs hipcc)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from weatherbench2_amd import _lib, build, engine, plan

N_LEVEL, N_LAT, N_LON = 13, 721, 1440


def resource_report() -> dict:
  """{kernel: (VGPRs, scratch bytes per lane, waves per SIMD)} of every
  instantiation in derived_fields.hip, from hipcc's own remarks."""
  import re
  src = os.path.join(build.CSRC, 'derived_fields.hip')
  cmd = [build._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17',
         '-ffp-contract=off', '-fPIC', '-I' + os.path.join(build.ROOT, 'include'),
         '-I' + build.CSRC, '-Rpass-analysis=kernel-resource-usage',
         '--cuda-device-only', '-c', src, '-o', os.devnull]
  text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
  out, name = {}, None
  for line in text.splitlines():
    m = re.search(r'Function Name: (\S+)', line)
    if m:
      name = subprocess.run(['c++filt', m.group(1)], capture_output=True,
                            text=True).stdout.strip() or m.group(1)
      name = name.replace('wb2::(anonymous namespace)::', '').split('(')[0]
      out[name] = {}
    for key, pat in (('vgprs', r' VGPRs: (\d+)'),
                     ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)')):
      m = re.search(pat, line)
      if m and name:
        out[name][key] = int(m.group(1))
  return out


def timed(launch, n_units, reps, warmup=5):
  for i in range(warmup):
    launch(i % n_units)
  torch.cuda.synchronize()
  pairs = []
  for i in range(reps):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    launch(i % n_units)
    b.record()
    pairs.append((a, b))
  torch.cuda.synchronize()
  ms = np.array([a.elapsed_time(b) for a, b in pairs])
  return float(np.median(ms)), float(ms.min())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=60)
  ap.add_argument('--pool-bytes', type=float, default=3e9)
  ap.add_argument('--only', default=None)
  ap.add_argument('--no-report', action='store_true')
  args = ap.parse_args()
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  n_point = N_LAT * N_LON
  n_total = N_LEVEL * n_point
  gen = torch.Generator(device=dev).manual_seed(0)
  lat = np.linspace(-90, 90, N_LAT)
  lon = np.arange(N_LON) * 0.25

  def fields(n_units, n_fields, dtype, lo=0.0, scale=10.0):
    return [[torch.randn((N_LEVEL, N_LAT, N_LON), device=dev, dtype=dtype,
                         generator=gen) * scale + lo for _ in range(n_fields)]
            for _ in range(n_units)]

  def units_for(bytes_per_unit):
    return max(3, int(args.pool_bytes // bytes_per_unit))

  def report(name, bytes_per_point, ms, extra=None):
    med, best = ms
    gbps = n_total * bytes_per_point / med / 1e6
    line = {'kernel': name, 'ms_median': round(med, 4), 'ms_min': round(best, 4),
            'bytes_per_point': bytes_per_point, 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 3)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med

  want = lambda name: args.only is None or args.only in name

  for dtype, code, size in ((torch.float32, _lib.WB2_F32, 4),
                            (torch.float64, _lib.WB2_F64, 8)):
    tag = 'f32' if size == 4 else 'f64'
    # -- the yardstick: the project's plain map kernel ---------------------
    if want('spatial_maps'):
      n = units_for(5 * size * n_total)
      pool = fields(n, 2, dtype)
      outs = [torch.empty((3, n_total), device=dev, dtype=dtype)
              for _ in range(n)]
      def launch(i):
        f, t = pool[i]
        _lib.check(lib.wb2_spatial_maps(
            code, f.data_ptr(), None, t.data_ptr(), None, 1, n_total,
            outs[i][0].data_ptr(), outs[i][1].data_ptr(),
            outs[i][2].data_ptr(), stream), 'wb2_spatial_maps')
      report(f'spatial_maps_{tag}', 5 * size, timed(launch, n, args.reps))
      del pool, outs
    # -- WindSpeed and the torch expression on the same tensors ------------
    if want('wind_speed'):
      n = units_for(3 * size * n_total)
      pool = fields(n, 2, dtype)
      outs = [torch.empty((n_total,), device=dev, dtype=dtype)
              for _ in range(n)]
      def launch(i):
        u, v = pool[i]
        _lib.check(lib.wb2_derived_pointwise(
            0, code, code, u.data_ptr(), None, v.data_ptr(), None, None, 1,
            n_total, outs[i].data_ptr(), stream), 'wb2_derived_pointwise')
      ours = report(f'wind_speed_{tag}', 3 * size,
                    timed(launch, n, args.reps))
      def launch_torch(i):
        u, v = pool[i]
        torch.sqrt(u * u + v * v)
      theirs = timed(launch_torch, n, args.reps)
      report(f'torch_sqrt_uu_vv_{tag}', 3 * size, theirs,
             {'torch_over_hip': round(theirs[0] / ours, 2)})
      u, v = pool[0]
      launch(0)
      same = torch.equal(outs[0].view(u.shape), torch.sqrt(u * u + v * v))
      print(json.dumps({'wind_speed_equals_torch_' + tag: bool(same)}))
      del pool, outs
    # -- RelativeHumidity (float32 exp, float64 divisions per point) -------
    if want('relative_humidity'):
      n = units_for((2 * size + 8) * n_total)
      pool = [[torch.rand((N_LEVEL, N_LAT, N_LON), device=dev, dtype=dtype,
                          generator=gen) * 80 + 220,
               torch.rand((N_LEVEL, N_LAT, N_LON), device=dev, dtype=dtype,
                          generator=gen) * 9e-3 + 1e-3] for _ in range(n)]
      outs = [torch.empty((n_total,), device=dev, dtype=torch.float64)
              for _ in range(n)]
      pressure = torch.linspace(50, 1000, N_LEVEL, dtype=torch.float64,
                                device=dev)
      def launch(i):
        t, q = pool[i]
        _lib.check(lib.wb2_derived_pointwise(
            1, code, _lib.WB2_F64, t.data_ptr(), None, q.data_ptr(), None,
            pressure.data_ptr(), N_LEVEL, n_point, outs[i].data_ptr(), stream),
                   'wb2_derived_pointwise')
      report(f'relative_humidity_{tag}', 2 * size + 8,
             timed(launch, n, args.reps))
      del pool, outs
    # -- the stencil kernel, both layouts ----------------------------------
    for layout in ('latlon', 'lonlat'):
      rows, cols = (lat, lon) if layout == 'latlon' else (lon, lat)
      (rt, ru), (ct, cu) = plan.gradient_tables(rows), plan.gradient_tables(cols)
      row_coef = engine.upload_f64_table(rt, dev)
      col_coef = engine.upload_f64_table(ct, dev)
      lat_tab = engine.upload_f64_table(plan.latitude_tables(lat), dev)
      for mode, n_in in (('divergence', 2), ('geostrophic_speed', 1),
                         ('ageostrophic_speed', 3)):
        name = f'stencil_{mode}_{layout}_{tag}'
        if not want(name):
          continue
        bytes_pp = n_in * size + 8
        n = units_for(bytes_pp * n_total)
        shape = (N_LEVEL, len(rows), len(cols))
        pool = [[torch.randn(shape, device=dev, dtype=dtype, generator=gen)
                 for _ in range(n_in)] for _ in range(n)]
        outs = [torch.empty(shape, device=dev, dtype=torch.float64)
                for _ in range(n)]
        def launch(i):
          x = pool[i]
          ins = ([x[0], x[1]] if mode == 'divergence' else
                 [x[0], x[0]] if n_in == 1 else [x[0], x[0], x[1], x[2]])
          ins = ins + [None] * (4 - len(ins))
          _lib.check(lib.wb2_derived_stencil(
              engine.STENCIL_MODES[mode], code, int(layout == 'latlon'),
              _lib.ptr_array(ins), _lib.ptr_array([None] * 4), N_LEVEL,
              shape[1], shape[2], row_coef.data_ptr(), int(ru),
              col_coef.data_ptr(), int(cu), lat_tab[0].data_ptr(),
              lat_tab[1].data_ptr(), plan.METERS_PER_DEGREE,
              outs[i].data_ptr(), stream), 'wb2_derived_stencil')
        report(name, bytes_pp, timed(launch, n, args.reps))
        del pool, outs
  if not args.no_report:
    try:
      rep = resource_report()
      spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
      print(json.dumps({'instantiations': len(rep), 'with_scratch': spills,
                        'max_vgprs': max(v['vgprs'] for v in rep.values()),
                        'min_occupancy': min(v['occupancy']
                                             for v in rep.values())}))
      assert not spills, spills
    except (OSError, subprocess.CalledProcessError) as e:
      print(json.dumps({'resource_report': f'not available: {e}'}))


if __name__ == '__main__':
  main()
