"""The regridding kernels alone (csrc/regrid.hip) on official shapes, over a
pool of distinct units much larger than the 256 MiB Infinity Cache (no re-use
between launches):

  cons_1p5     13 x 1440 x 721 float32 -> 240 x 121, conservative, (lat, lon)
               and (lon, lat) slabs
  cons_5p625   the same -> 64 x 32
  bilinear_up  13 x 64 x 32 float32 -> 240 x 121, bilinear, both layouts
  nearest_1p5  13 x 1440 x 721 float32 -> 240 x 121, nearest
  cons_1p5_x16 16 such chunks in one launch (208 slabs, 864 MB): a 13-level
               launch lasts about as long as the launch path itself, this one
               shows the kernel

  python tools/regrid_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/regrid_bench.py --reps 20

One JSON line per shape and layout: ms per launch (a HIP event pair around
every launch, median and min), GB/s against the kernel's roofline -- sizeof(T)
bytes per source element when downsampling (every source element read once),
the output bytes when upsampling, the gathered elements read and written for
nearest -- and that as a share of 8 TB/s.  In the same call, alternating with
the kernel, the torch expression a user would write today on the same tensors
(`isnan`, `where`, two `einsum` with the dense weights -- latitude first, then
longitude: the reference's one three-operand einsum is some tens of times
slower in torch --, a divide), with `torch_over_hip`.

A last line is the resource report of the build: registers, scratch and
occupancy per instantiation, and the dynamic LDS a workgroup asks for at the
official shapes; no instantiation may use scratch (CPU side; needs hipcc)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.column_bench import resource_report
from tools.derived_bench import timed
from weatherbench2_amd import engine
from weatherbench2_amd import regridding as rg

N_LEVEL = 13


def grid(n_lon, n_lat, poles=True) -> rg.Grid:
  spacing = (rg.LatitudeSpacing.EQUIANGULAR_WITH_POLES if poles
             else rg.LatitudeSpacing.EQUIANGULAR_WITHOUT_POLES)
  return rg.Grid(
      longitudes=rg.longitude_values(rg.LongitudeScheme.START_AT_ZERO, n_lon),
      latitudes=rg.latitude_values(spacing, n_lat), periodic=True,
      includes_poles=poles)


# name -> (class, source, target, what bounds the kernel, slabs)
SHAPES = {
    'cons_1p5': (rg.ConservativeRegridder, (1440, 721, True),
                 (240, 121, True), 'source', N_LEVEL),
    'cons_5p625': (rg.ConservativeRegridder, (1440, 721, True),
                   (64, 32, False), 'source', N_LEVEL),
    'bilinear_up': (rg.BilinearRegridder, (64, 32, False), (240, 121, True),
                    'target', N_LEVEL),
    'nearest_1p5': (rg.NearestRegridder, (1440, 721, True), (240, 121, True),
                    'gather', N_LEVEL),
    'cons_1p5_x16': (rg.ConservativeRegridder, (1440, 721, True),
                     (240, 121, True), 'source', 16 * N_LEVEL),
    'cons_5p625_x16': (rg.ConservativeRegridder, (1440, 721, True),
                       (64, 32, False), 'source', 16 * N_LEVEL),
}


def torch_conservative(x, lon_w, lat_w, lat_rows):
  """What a user writes today (the reference's expression on the device)."""
  nulls = x.isnan()
  filled = torch.where(nulls, 0.0, x)
  present = (~nulls).to(x.dtype)
  if lat_rows:
    mean = lambda f: torch.einsum('ab,lcb->lca', lon_w,
                                  torch.einsum('cd,ldb->lcb', lat_w, f))
  else:
    mean = lambda f: torch.einsum('ab,lbc->lac', lon_w,
                                  torch.einsum('cd,lbd->lbc', lat_w, f))
  return mean(filled) / mean(present)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=40)
  ap.add_argument('--pool-bytes', type=float, default=3e9)
  ap.add_argument('--only', default=None)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  dev = engine.require_gpu()
  gen = torch.Generator(device=dev).manual_seed(0)

  def report(name, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'kernel': name, 'ms_median': round(med, 4), 'ms_min': round(best, 4),
            'MB': round(n_bytes / 1e6, 2), 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med

  lds = {}
  for name, (cls, src, tgt, bound, n_level) in SHAPES.items():
    if args.only is not None and args.only not in name:
      continue
    source, target = grid(*src), grid(*tgt)
    regridder = cls(source, target)
    n_src = source.shape[0] * source.shape[1]
    n_tgt = target.shape[0] * target.shape[1]
    n_bytes = 4 * n_level * {'source': n_src, 'target': n_tgt,
                             'gather': 2 * n_tgt}[bound]
    n = max(3, min(64, int(args.pool_bytes // (4 * n_level * n_src))))
    for lat_rows in (True, False):
      shape = ((n_level, source.shape[1], source.shape[0]) if lat_rows
               else (n_level,) + source.shape)
      pool = []
      for _ in range(n):
        x = torch.randn(shape, device=dev, generator=gen) * 10 + 280
        x[torch.rand(shape, device=dev, generator=gen) < 0.01] = float('nan')
        pool.append(x)
      layout = 'latlon' if lat_rows else 'lonlat'
      label = f'{name}_{layout}'
      holder = [None]
      regridder._run(pool[0], lat_rows)  # tables built and uploaded

      def launch(i):
        holder[0] = regridder._run(pool[i], lat_rows)
      extra = {'roofline': bound, 'slabs': n_level}
      if cls is not rg.NearestRegridder:
        lon_t, lat_t = regridder.axis_tables
        extra = {'roofline': bound, 'slabs': n_level,
                 'longest_lon_band': lon_t.longest,
                 'longest_lat_band': lat_t.longest}
        geo = engine.regrid_geometry(torch.float32, lat_rows, True)
        lds[label] = (16 * source.shape[0] if lat_rows
                      else geo['band'] * 4 * source.shape[1])
      ours = report(label, n_bytes, timed(launch, n, args.reps), extra)
      if cls is rg.ConservativeRegridder and not args.no_torch:
        lon_w, lat_w = (torch.from_numpy(w).to(dev, torch.float32)
                        for w in regridder.weights)
        want = torch_conservative(pool[0], lon_w, lat_w, lat_rows)
        launch(0)
        same = torch.equal(holder[0].isnan(), want.isnan())
        close = torch.allclose(holder[0], want, rtol=1e-4, atol=1e-3,
                               equal_nan=True)
        del want

        def launch_torch(i):
          holder[0] = torch_conservative(pool[i], lon_w, lat_w, lat_rows)
        theirs = timed(launch_torch, n, max(5, args.reps // 4))
        report('torch_' + label, n_bytes, theirs,
               {'torch_over_hip': round(theirs[0] / ours, 2),
                'same_nan': same, 'allclose': close})
      holder[0] = None
      del pool
  if not args.no_report:
    try:
      rep = resource_report('regrid.hip')
      spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
      for k, v in rep.items():
        print(json.dumps({'instantiation': k, **v}))
      print(json.dumps({'instantiations': len(rep), 'with_scratch': spills,
                        'max_vgprs': max(v['vgprs'] for v in rep.values()),
                        'min_occupancy': min(v['occupancy']
                                             for v in rep.values()),
                        'dynamic_lds_bytes': lds}))
      assert not spills, spills
    except (OSError, subprocess.CalledProcessError) as e:
      print(json.dumps({'resource_report': f'not available: {e}'}))


if __name__ == '__main__':
  main()
