"""The quantile kernels alone (csrc/quantile.hip) on three shapes, over a
pool of distinct inputs larger than the 256 MiB Infinity Cache (no re-use
between launches):

  era5_year   1 464 six-hourly samples of 13 x 32 x 64 float32, 5 quantiles:
              the example of scripts/compute_quantiles.py; resident regime
  ensemble    50 members of 121 x 240 float32, 3 quantiles; resident regime
  era5_16y    23 376 samples of 32 x 64 float32, 5 quantiles; streaming regime

  python tools/quantile_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/quantile_bench.py --reps 20

Each shape runs with `skipna` off and on.  One JSON line per run: ms per
launch (a HIP event pair around every launch, median and min), GB/s against
the roofline of n_red * sizeof(T) input bytes per point (the input read once)
and that as a share of 8 TB/s; for the streaming regime also how often the
kernel reads the input (1 + ceil(n_q / targets_per_pass) * (passes + 1), the
passes worked out from the data as the kernel does).  In the same call:

  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before every shape);
  * the torch expression a user would write today on the same tensors
    (`torch.sort` along the axis, the gather of both neighbours and the same
    interpolation), with `torch_over_hip` and whether the two agree.

The last lines are the resource report of the build: registers, LDS, scratch
and occupancy per instantiation; no instantiation may use scratch (CPU side;
needs hipcc)."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.derived_bench import timed
from weatherbench2_amd import _lib, build, engine

# name -> (n_red, n_point, quantiles, mean, spread)
SHAPES = {
    'era5_year': (1464, 13 * 32 * 64, [0.01, 0.1, 0.5, 0.9, 0.99], 280.0, 8.0),
    'ensemble': (50, 121 * 240, [0.1, 0.5, 0.9], 0.0, 1.0),
    'era5_16y': (23376, 32 * 64, [0.01, 0.1, 0.5, 0.9, 0.99], 280.0, 8.0),
}


def torch_expression(x, q, skipna):
  """What a user writes today: [n_red, n_point] -> float64 [n_q, n_point]."""
  s, _ = torch.sort(x, dim=0)  # NaN last
  n = x.shape[0]
  n_nan = x.isnan().sum(0)
  m = n - n_nan if skipna else torch.full_like(n_nan, n)
  none = (m == 0) | ((n_nan > 0) & (not skipna))
  m1 = (m.clamp(min=1) - 1)
  v = q[:, None] * m1.double()[None]
  lo = v.floor()
  t = v - lo
  lo = lo.long()
  hi = torch.minimum(lo + 1, m1[None])
  a, b = s.gather(0, lo), s.gather(0, hi)
  d = b - a
  res = torch.where(t < 0.5, a.double() + d.double() * t,
                    b.double() - d.double() * (1.0 - t))
  return torch.where(none[None], float('nan'), res)


def input_reads(x, n_q, geo):
  """How often the streaming kernel reads a float32 input [n_red, n_point]:
  the mean over its workgroup tiles of 1 + groups * (passes + 1)."""
  bits = x.view(torch.int32).long() & 0xFFFFFFFF
  key = torch.where(bits >= 2**31, bits ^ 0xFFFFFFFF, bits | 2**31)
  nan = x.isnan()
  kmin = torch.where(nan, 2**32 - 1, key).amin(0)
  kmax = torch.where(nan, 0, key).amax(0)
  diff = (kmin ^ kmax).double()
  n_bits = torch.where(diff > 0, diff.clamp(min=1).log2().floor() + 1, 0.0)
  step = geo['key_bits_per_pass']
  passes = (n_bits / step).ceil()
  tile = geo['tile_points']
  pad = (-passes.numel()) % tile
  passes = torch.cat([passes, passes.new_zeros(pad)]).reshape(-1, tile).amax(1)
  groups = -(-n_q // geo['targets_per_pass'])
  return float((1 + groups * (passes + 1)).mean())


def resource_report(source='quantile.hip') -> dict:
  """{kernel: VGPRs, static LDS bytes, scratch bytes per lane, waves per SIMD}
  of every instantiation, from hipcc's own remarks."""
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
                     ('lds_static', r'LDS Size \[bytes/block\]: (\d+)'),
                     ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)')):
      m = re.search(pat, line)
      if m and name:
        out[name][key] = int(m.group(1))
  for name, v in out.items():
    if 'resident' in name:
      v['lds_dynamic'] = '64 bytes per sample: n_red * 64, at most 163840'
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool-bytes', type=float, default=3e9)
  ap.add_argument('--only', default=None)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  geo = engine.quantile_geometry(torch.float32)
  print(json.dumps({'geometry_f32': geo}), flush=True)

  def report(name, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'kernel': name, 'ms_median': round(med, 4), 'ms_min': round(best, 4),
            'MB': round(n_bytes / 1e6, 1), 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med

  n_ws = 13 * 721 * 1440
  ws = [[torch.randn(n_ws, device=dev, generator=gen) for _ in range(3)]
        for _ in range(max(3, int(args.pool_bytes // (12 * n_ws))))]

  def yardstick(before):
    def launch(i):
      u, v, out = ws[i]
      _lib.check(lib.wb2_derived_pointwise(
          0, _lib.WB2_F32, _lib.WB2_F32, u.data_ptr(), None, v.data_ptr(), None,
          None, 1, n_ws, out.data_ptr(), stream), 'wb2_derived_pointwise')
    report('wind_speed_f32', 12 * n_ws, timed(launch, len(ws), args.reps),
           {'before': before})

  for name, (n_red, n_point, q, mean, spread) in SHAPES.items():
    if args.only is not None and args.only not in name:
      continue
    n_bytes = 4 * n_red * n_point
    n = min(64, max(3, int(args.pool_bytes // n_bytes)))
    pool = [torch.randn((n_red, n_point), device=dev, generator=gen) * spread
            + mean for _ in range(n)]
    regime = 'resident' if n_red <= geo['max_resident'] else 'streaming'
    q_dev = torch.tensor(q, dtype=torch.float64, device=dev)
    yardstick(name)
    for skipna in (False, True):
      label = f'{name}_{"skipna" if skipna else "keepna"}'
      holder = [None]

      def launch(i):
        holder[0] = engine.quantile_select(pool[i], None, 1, n_red, n_point, q,
                                           skipna)
      extra = {'regime': regime, 'n_red': n_red, 'n_point': n_point,
               'n_q': len(q), 'roofline_bytes_per_point': 4 * n_red}
      if regime == 'streaming':
        extra['input_reads'] = round(input_reads(pool[0], len(q), geo), 2)
      ours = report(label, n_bytes, timed(launch, n, args.reps), extra)
      if not args.no_torch:
        want = torch_expression(pool[0], q_dev, skipna)
        launch(0)
        got = holder[0][:, 0]
        same = (torch.equal(got.isnan(), want.isnan())
                and torch.equal(got.nan_to_num(), want.nan_to_num()))
        del want

        def launch_torch(i):
          holder[0] = torch_expression(pool[i], q_dev, skipna)
        theirs = timed(launch_torch, n, max(5, args.reps // 4), warmup=2)
        report('torch_' + label, n_bytes, theirs,
               {'torch_over_hip': round(theirs[0] / ours, 2), 'equal': same})
      holder[0] = None
    del pool
  yardstick('end')
  if not args.no_report:
    try:
      rep = resource_report()
      spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
      for k, v in rep.items():
        print(json.dumps({'instantiation': k, **v}))
      print(json.dumps({'instantiations': len(rep), 'with_scratch': spills,
                        'max_vgprs': max(v['vgprs'] for v in rep.values()),
                        'min_occupancy': min(v['occupancy']
                                             for v in rep.values())}))
      assert not spills, spills
    except (OSError, subprocess.CalledProcessError) as e:
      print(json.dumps({'resource_report': f'not available: {e}'}))


if __name__ == '__main__':
  main()
