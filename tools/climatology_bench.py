"""The climatology kernels alone (csrc/climatology.hip) on two shapes, one
process per shape, distinct inputs per launch (no re-use between launches):

  hourly_31y  31 years (1990-2020) six-hourly of 13 x 64 x 32 float32, hourly
              climatology (4 hours x 366 days)
  daily_10y   10 years (2011-2020) daily of 1440 x 721 float32, daily
              climatology (366 days)

  python tools/climatology_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/climatology_bench.py --only daily_10y

One JSON line per run: ms per launch (a HIP event pair around every launch,
median and min), GB/s against the roofline of (n_selected * sizeof(T) + 24 *
n_group + 8) bytes per point (every selected sample read once, the three
float64 moment planes written once, the pivot read once) and that as a share
of 8 TB/s.  In the same process:

  * the moments kernel with the explicit plan (the fill of day 366 included),
    the pivot kernel and the smoothing kernel (both modes), each on its own;
  * K13's `mean` over contiguous bins of the same input and as many outputs
    as there are groups: the project's streaming reduction over time;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape);
  * the torch expression a user would write today: `index_add_` of the count,
    x and x * x (NaN as 0) into float64 planes, with `torch_over_hip` and
    whether the moments agree to rounding.

The last lines are the resource report of the build: registers, LDS, scratch
and occupancy per instantiation; no instantiation may use scratch (CPU side;
needs hipcc)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.derived_bench import timed
from tools.quantile_bench import resource_report
from weatherbench2_amd import _lib, climatology, engine

# name -> (first day, last day (exclusive), step hours, n_point, hours)
SHAPES = {
    'hourly_31y': ('1990-01-01', '2021-01-01', 6, 13 * 64 * 32, (0, 6, 12, 18)),
    'daily_10y': ('2011-01-01', '2021-01-01', 24, 1440 * 721, None),
}
WINDOW = 61


def run_shape(name, args):
  start, stop, step, n_point, hours = SHAPES[name]
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  times = np.arange(np.datetime64(start, 'h'), np.datetime64(stop, 'h'),
                    np.timedelta64(step, 'h')).astype('datetime64[ns]')
  n_time = len(times)
  plan = climatology.plan_groups(times, np.arange(n_time), 'explicit', hours)
  n_group = plan.n_cycle * plan.n_pos
  print(json.dumps({'shape': name, 'n_time': n_time, 'n_point': n_point,
                    'n_group': n_group, 'n_member': int(plan.member.size),
                    'geometry_f32':
                    engine.climatology_geometry(torch.float32, True)}),
        flush=True)

  def report(kernel, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'shape': name, 'kernel': kernel, 'ms_median': round(med, 4),
            'ms_min': round(best, 4), 'MB': round(n_bytes / 1e6, 1),
            'GBps': round(gbps, 1), 'frac_of_8TBps': round(gbps / 8000.0, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med

  n_ws = 13 * 721 * 1440
  ws = [[torch.randn(n_ws, device=dev, generator=gen) for _ in range(3)]
        for _ in range(3)]

  def yardstick(before):
    def launch(i):
      u, v, out = ws[i]
      _lib.check(lib.wb2_derived_pointwise(
          0, _lib.WB2_F32, _lib.WB2_F32, u.data_ptr(), None, v.data_ptr(), None,
          None, 1, n_ws, out.data_ptr(), stream), 'wb2_derived_pointwise')
    report('wind_speed_f32', 12 * n_ws, timed(launch, len(ws), args.reps),
           {'before': before})

  in_bytes = 4 * n_time * n_point
  n = min(8, max(2, int(args.pool_bytes // in_bytes)))
  pool = []
  for _ in range(n):
    x = torch.randn((1, n_time, n_point), device=dev, generator=gen)
    x.mul_(8.0).add_(280.0)
    x[:, :, ::977][torch.rand(x[:, :, ::977].shape, device=dev,
                              generator=gen) < 0.5] = float('nan')
    pool.append(x)
  member = torch.from_numpy(plan.member).to(dev)
  fill = torch.from_numpy(plan.fill).to(dev)
  holder = [None]
  yardstick(name)

  pivots = [engine.first_finite(x, None, 1, n_time, n_point, member)
            for x in pool]
  report('first_finite_f32', 12 * n_point, timed(
      lambda i: holder.__setitem__(0, engine.first_finite(
          pool[i], None, 1, n_time, n_point, member)), n, args.reps))
  roofline = 4 * n_time + 24 * n_group + 8
  extra = {'n_time': n_time, 'n_group': n_group,
           'roofline_bytes_per_point': roofline}

  # the entry point itself: the offsets uploaded and the planes allocated once
  import ctypes
  begin_dev = torch.from_numpy(plan.group_begin).to(dev)
  begin_host = plan.group_begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
  planes = [torch.empty((1, n_group, n_point), dtype=torch.float64, device=dev)
            for _ in range(3)]

  def launch(i):
    _lib.check(lib.wb2_group_moments(
        _lib.WB2_F32, pool[i].data_ptr(), None, 1, n_time, n_point,
        begin_dev.data_ptr(), begin_host, n_group, member.data_ptr(),
        fill.data_ptr(), int(member.numel()), pivots[i].data_ptr(),
        planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
        stream), 'wb2_group_moments')
  ours = report('group_moments_f32', roofline * n_point,
                timed(launch, n, args.reps), extra)

  # K13: the mean of as many contiguous bins as there are groups
  k = -(-n_time // n_group)
  begin = np.arange(0, n_time, k)
  ranges = np.stack([begin, np.minimum(begin + k, n_time)], 1).astype(np.int32)
  bins = torch.from_numpy(ranges).to(dev)

  def launch_k13(i):
    holder[0] = engine.time_bin_stats(pool[i], None, 1, n_time, n_point, bins,
                                      ['mean'], True, 1)
  k13_bytes = 4 * n_point * (n_time + len(ranges))
  report('time_bin_mean_f32', k13_bytes, timed(launch_k13, n, args.reps),
         {'n_bin': len(ranges), 'steps_per_bin': k})
  holder[0] = None

  # the smoothing kernel on its own
  moments = engine.group_moments(pool[0], None, 1, n_time, n_point,
                                 plan.group_begin, member, fill, pivots[0])
  weights = torch.from_numpy(
      climatology.create_window_weights(WINDOW).values).to(dev)
  for mode in engine.SMOOTH_MODES:
    def launch_smooth(i):
      holder[0] = engine.cycle_smooth(mode, moments, pivots[0], plan.n_cycle,
                                      plan.n_pos, weights)
    report(f'cycle_smooth_{mode}', 8 * n_point * (5 * n_group + 1),
           timed(launch_smooth, 1, args.reps), {'window': WINDOW})
  holder[0] = None

  if not args.no_torch:
    # the torch expression: no fill, no pivot
    group_of = np.zeros(n_time, dtype=np.int64)
    for g in range(n_group):
      mine = plan.member[plan.group_begin[g]:plan.group_begin[g + 1]]
      group_of[mine[mine >= 0]] = g
    index = torch.from_numpy(group_of).to(dev)

    def torch_moments(x):
      out = torch.zeros((3, 1, n_group, n_point), dtype=torch.float64,
                        device=dev)
      nan = x.isnan()
      v = torch.where(nan, 0.0, x.double())
      out[0].index_add_(1, index, (~nan).double())
      out[1].index_add_(1, index, v)
      out[2].index_add_(1, index, v * v)
      return out
    want = torch_moments(pool[0])
    got = engine.group_moments(pool[0], None, 1, n_time, n_point,
                               plan.group_begin, member, None, None)
    same = all(bool(((g - w).abs() <= 1e-12 * w.abs().max()).all())
               for g, w in zip(got, want))
    del want, got

    def launch_torch(i):
      holder[0] = torch_moments(pool[i])
    theirs = timed(launch_torch, n, max(5, args.reps // 4), warmup=2)
    report('torch_index_add_f32', roofline * n_point, theirs,
           {'torch_over_hip': round(theirs[0] / ours, 2), 'agree': same})
    holder[0] = None
  yardstick('end')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool-bytes', type=float, default=3e10)
  ap.add_argument('--only', default=None)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  if args.only is not None:
    if args.only not in SHAPES:
      raise SystemExit(f'--only must be one of {list(SHAPES)}')
    run_shape(args.only, args)
    return
  # one fresh process per shape: nothing of one shape's pool, allocator state
  # or clocks carries into the next
  for name in SHAPES:
    cmd = [sys.executable, os.path.abspath(__file__), '--only', name,
           '--reps', str(args.reps), '--pool-bytes', str(args.pool_bytes)]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    try:
      rep = resource_report('climatology.hip')
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
