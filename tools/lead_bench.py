"""The lead-window kernel alone (csrc/derived_lead.hip) on official shapes,
over a pool of distinct units much larger than the 256 MiB Infinity Cache (no
re-use between launches):

  era5_6h     41 six-hourly leads of 721 x 1440 float32, windows 1 and 4
              (total_precipitation_6hr / _24hr) and the plain sum over 4
              (total_precipitation_24hr_from_6hr)
  era5_1h     49 hourly leads of 721 x 1440 float32, windows 6 and 24
  ens_50      50 members x 41 leads of 240 x 121 float32, window 4
  era5_6h_f64 the first shape as float64, window 4

  python tools/lead_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/lead_bench.py --reps 20

One JSON line per shape and window: ms per launch (a HIP event pair around
every launch, median and min), GB/s against the kernel's roofline of
2 * sizeof(T) bytes per element (every input element read once, every output
element written once) and that as a share of 8 TB/s.  In the same call,
alternating with the kernel:

  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before every shape);
  * the torch expression a user would write today on the same tensors
    (`diff`, `unfold(...).sum(-1)`, `where`, a NaN block in front), with
    `torch_over_hip`.

A last line is the resource report of the build: registers, scratch and
occupancy per instantiation; no instantiation may use scratch (CPU side; needs
hipcc)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.column_bench import resource_report
from tools.derived_bench import timed
from weatherbench2_amd import _lib, engine

# name -> (n_outer, n_lead, n_point, dtype, [(mode, window)])
SHAPES = {
    'era5_6h': (1, 41, 721 * 1440, torch.float32,
                [('diff_sum', 1), ('diff_sum', 4), ('sum', 4)]),
    'era5_1h': (1, 49, 721 * 1440, torch.float32,
                [('diff_sum', 6), ('diff_sum', 24)]),
    'ens_50': (50, 41, 240 * 121, torch.float32, [('diff_sum', 4)]),
    'era5_6h_f64': (1, 41, 721 * 1440, torch.float64, [('diff_sum', 4)]),
}


def torch_expression(x, mode, w):
  """What a user writes today: [n_outer, n_lead, n_point] -> the same."""
  if mode == 'diff_sum':
    acc = x.diff(dim=1).unfold(1, w, 1).sum(-1)
    acc = torch.where((acc >= 0) | acc.isnan(), acc, 0.0)
    n_nan = w
  else:
    acc = x.unfold(1, w, 1).sum(-1)
    n_nan = w - 1
  pad = torch.full((x.shape[0], n_nan, x.shape[2]), float('nan'),
                   dtype=x.dtype, device=x.device)
  return torch.cat([pad, acc], dim=1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=40)
  ap.add_argument('--pool-bytes', type=float, default=3e9)
  ap.add_argument('--only', default=None)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)

  def report(name, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'kernel': name, 'ms_median': round(med, 4), 'ms_min': round(best, 4),
            'MB': round(n_bytes / 1e6, 1), 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 3)}
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

  for name, (n_outer, n_lead, n_point, dtype, runs) in SHAPES.items():
    if args.only is not None and args.only not in name:
      continue
    size = torch.empty((), dtype=dtype).element_size()
    n_elem = n_outer * n_lead * n_point
    n_bytes = 2 * size * n_elem
    n = max(3, int(args.pool_bytes // n_bytes))
    # cumulative series with negative steps mixed in, so that the clamp acts
    pool = []
    for _ in range(n):
      steps = torch.rand((n_outer, n_lead, n_point), device=dev, dtype=dtype,
                         generator=gen) - 0.3
      pool.append(steps.cumsum(dim=1))
      del steps
    yardstick(name)
    for mode, w in runs:
      label = f'{name}_{mode}_w{w}'
      holder = [None]

      def launch(i):
        holder[0] = engine.derived_lead_window(mode, pool[i], None, n_outer,
                                               n_lead, n_point, w, True)
      ours = report(label, n_bytes, timed(launch, n, args.reps),
                    {'roofline_bytes_per_element': 2 * size})
      if not args.no_torch:
        want = torch_expression(pool[0], mode, w)
        launch(0)
        same = torch.equal(holder[0].isnan(), want.isnan())
        close = torch.allclose(holder[0], want, rtol=1e-4, atol=1e-4,
                               equal_nan=True)
        del want

        def launch_torch(i):
          holder[0] = torch_expression(pool[i], mode, w)
        theirs = timed(launch_torch, n, max(5, args.reps // 4))
        report('torch_' + label, n_bytes, theirs,
               {'torch_over_hip': round(theirs[0] / ours, 2),
                'same_nan': same, 'allclose': close})
      holder[0] = None
    del pool
  yardstick('end')
  if not args.no_report:
    try:
      rep = resource_report('derived_lead.hip')
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
