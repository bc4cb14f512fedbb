"""The level-column kernels alone (csrc/derived_column.hip) at the size of one
official unit, 13 x 721 x 1440 float32 points, over a pool of distinct units
much larger than the 256 MiB Infinity Cache (no re-use between launches).

  python tools/column_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/column_bench.py --reps 20

One JSON line per class: ms per evaluation (a HIP event pair around every
evaluation, median and min), GB/s of the ALGORITHMIC bytes (every selected
input level once + the output once, in their dtypes) and that as a share of
8 TB/s.  In the same call, alternating with the classes:

  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before every class);
  * for every class the straightforward torch expression a user would write
    today (torch.trapezoid, torch.gradient, torch.cumulative_trapezoid,
    mean(-1, keepdim=True)) on the same tensors, with `torch_over_hip`.

A last line checks that the resource report of the build shows no scratch
(CPU side; needs hipcc)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.derived_bench import timed
from weatherbench2_amd import _lib, build, engine, plan

N_LEVEL, N_LAT, N_LON = 13, 721, 1440
LEVELS = np.array([50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925,
                   1000])
G = 9.81


def resource_report(source: str = 'derived_column.hip') -> dict:
  """{kernel: VGPRs, scratch bytes per lane, waves per SIMD} of every
  instantiation in `source`, from hipcc's own remarks."""
  import re
  src = os.path.join(build.CSRC, source)
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
      name = name.replace('void ', '')
      out[name] = {}
    for key, pat in (('vgprs', r' VGPRs: (\d+)'),
                     ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)')):
      m = re.search(pat, line)
      if m and name:
        out[name][key] = int(m.group(1))
  return out


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
  shape = (N_LEVEL, N_LAT, N_LON)
  f32, f64 = _lib.WB2_F32, _lib.WB2_F64

  def pool_of(n_fields, bytes_per_unit):
    n = max(3, int(args.pool_bytes // bytes_per_unit))
    return n, [[torch.randn(shape, device=dev, dtype=torch.float32,
                            generator=gen) for _ in range(n_fields)]
               for _ in range(n)]

  def report(name, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'kernel': name, 'ms_median': round(med, 4), 'ms_min': round(best, 4),
            'MB': round(n_bytes / 1e6, 1), 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 3)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med

  # the yardstick's own pool
  n_ws, ws_pool = pool_of(2, 12 * n_total)
  ws_out = [torch.empty((n_total,), device=dev) for _ in range(n_ws)]

  def yardstick(before):
    def launch(i):
      u, v = ws_pool[i]
      _lib.check(lib.wb2_derived_pointwise(
          0, f32, f32, u.data_ptr(), None, v.data_ptr(), None, None, 1,
          n_total, ws_out[i].data_ptr(), stream), 'wb2_derived_pointwise')
    report('wind_speed_f32', 12 * n_total, timed(launch, n_ws, args.reps),
           {'before': before})

  table = engine.upload_table(np.arange(N_LEVEL, dtype=np.int64), dev)
  tables = _lib.ptr_array([table, table, table])
  spacing = engine.upload_f64_table(np.diff(LEVELS).astype(np.float64), dev)
  pascal = engine.upload_f64_table(np.diff(100 * LEVELS).astype(np.float64),
                                   dev)
  coef_host, uniform = plan.gradient_tables(LEVELS)
  coef = engine.upload_f64_table(coef_host, dev)
  lev64 = torch.as_tensor(LEVELS, dtype=torch.float64, device=dev)
  lev32 = lev64.float()
  pa64 = 100 * lev64

  def column(mode, ins, out, begin=0, end=N_LEVEL, dtype=f32, out_dtype=f64,
             means=(), scale=1 / G, space=spacing):
    ptrs = _lib.ptr_array((list(ins) + list(means) + [None] * 4)[:4])
    _lib.check(lib.wb2_derived_column(
        engine.COLUMN_MODES[mode], dtype, out_dtype, ptrs, tables, 1, N_LEVEL,
        n_point, begin, end, space.data_ptr(), coef.data_ptr(), int(uniform),
        N_LON, N_LAT, scale, out.data_ptr(), stream), 'wb2_derived_column')

  want = lambda name: args.only is None or args.only in name

  def both(name, n_bytes, launch, launch_torch, n):
    yardstick(name)
    ours = report(name, n_bytes, timed(launch, n, args.reps))
    theirs = timed(launch_torch, n, args.reps)
    report('torch_' + name, n_bytes, theirs,
           {'torch_over_hip': round(theirs[0] / ours, 2)})

  if want('total_column_water'):
    n, pool = pool_of(1, 4 * n_total)
    outs = [torch.empty((N_LAT, N_LON), device=dev, dtype=torch.float64)
            for _ in range(n)]
    both('total_column_water', 4 * n_total + 8 * n_point,
         lambda i: column('integral', pool[i], outs[i]),
         lambda i: 1 / G * torch.trapezoid(pool[i][0], lev64[:, None, None],
                                           dim=0), n)
    del pool, outs
  if want('integrated_water_transport'):
    b, e = 5, N_LEVEL  # 300 ... 1000 hPa: 8 of the 13 levels
    n, pool = pool_of(3, 12 * n_total)
    outs = [torch.empty((N_LAT, N_LON), device=dev, dtype=torch.float64)
            for _ in range(n)]
    x = lev64[b:e, None, None]

    def ivt_torch(i):
      q, u, v = pool[i]
      iu = torch.trapezoid((q * u)[b:e], x, dim=0)
      iv = torch.trapezoid((q * v)[b:e], x, dim=0)
      return 1 / G * torch.sqrt(iu ** 2 + iv ** 2)
    both('integrated_water_transport', 12 * (e - b) * n_point + 8 * n_point,
         lambda i: column('transport', pool[i], outs[i], b, e), ivt_torch, n)
    del pool, outs
  if want('lapse_rate'):
    n, pool = pool_of(2, 12 * n_total)
    outs = [torch.empty(shape, device=dev) for _ in range(n)]

    def lapse_torch(i):
      t, z = pool[i]
      dt = torch.gradient(t, spacing=(lev32,), dim=0)[0]
      dz = torch.gradient(z, spacing=(lev32,), dim=0)[0]
      return dt / ((1 / G) * dz)
    both('lapse_rate', 12 * n_total,
         lambda i: column('gradient_ratio', pool[i], outs[i], out_dtype=f32),
         lapse_torch, n)
    del pool, outs
  if want('eddy_kinetic_energy'):
    n, pool = pool_of(2, 8 * n_total)
    outs = [torch.empty((N_LAT, N_LON), device=dev, dtype=torch.float64)
            for _ in range(n)]
    bars = [torch.empty((N_LEVEL, N_LAT), device=dev) for _ in range(2)]

    def eke(i):
      for x, bar in zip(pool[i], bars):
        _lib.check(lib.wb2_derived_zonal_mean(
            f32, 1, x.data_ptr(), None, N_LEVEL, N_LAT, N_LON, bar.data_ptr(),
            stream), 'wb2_derived_zonal_mean')
      column('eddy', pool[i], outs[i], means=bars, scale=0.5)

    def eke_torch(i):
      u, v = pool[i]
      du = u - u.mean(-1, keepdim=True)
      dv = v - v.mean(-1, keepdim=True)
      return 0.5 * torch.trapezoid(du ** 2 + dv ** 2, lev64[:, None, None],
                                   dim=0)
    both('eddy_kinetic_energy', 8 * n_total + 8 * n_point, eke, eke_torch, n)
    del pool, outs
  if want('vertical_velocity'):
    lat = np.linspace(-90, 90, N_LAT)
    lon = np.arange(N_LON) * 0.25
    (rt, ru), (ct, cu) = plan.gradient_tables(lat), plan.gradient_tables(lon)
    row_coef = engine.upload_f64_table(rt, dev)
    col_coef = engine.upload_f64_table(ct, dev)
    lat_tab = engine.upload_f64_table(plan.latitude_tables(lat), dev)
    n, pool = pool_of(2, 8 * n_total + 8 * n_total)
    outs = [torch.empty(shape, device=dev, dtype=torch.float64)
            for _ in range(n)]
    none4 = _lib.ptr_array([None] * 4)

    def divergence(i):
      u, v = pool[i]
      _lib.check(lib.wb2_derived_stencil(
          0, f32, 1, _lib.ptr_array([u, v, None, None]), none4, N_LEVEL, N_LAT,
          N_LON, row_coef.data_ptr(), int(ru), col_coef.data_ptr(), int(cu),
          lat_tab[0].data_ptr(), lat_tab[1].data_ptr(), plan.METERS_PER_DEGREE,
          outs[i].data_ptr(), stream), 'wb2_derived_stencil')

    def cumulative(i):
      column('cumulative', [], outs[i], dtype=f64, space=pascal)

    def omega(i):
      divergence(i)
      cumulative(i)

    def omega_torch(i):
      divergence(i)
      w = torch.cumulative_trapezoid(-outs[i], x=pa64[:, None, None], dim=0)
      return torch.cat([torch.zeros_like(w[:1]), w])
    # 16 B per point for the divergence (two float32 in, one float64 out), 16 B
    # for the integral in place
    both('vertical_velocity', 32 * n_total, omega, omega_torch, n)
    yardstick('column_cumulative')
    report('column_cumulative', 16 * n_total, timed(cumulative, n, args.reps))
    del pool, outs
  yardstick('end')
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
