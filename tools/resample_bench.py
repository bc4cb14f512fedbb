"""The time-statistics kernel alone (csrc/time_window.hip) on three shapes,
one process per shape, over a pool of distinct inputs larger than the 256 MiB
Infinity Cache where one input is not (no re-use between launches):

  hourly_daily    720 hourly steps of 1440 x 721 float32 into 30 days
  weekly          1 464 six-hourly steps of 13 x 64 x 32 float32 into weeks
                  of 28 (the last one short: non-uniform bins)
  ensemble_leads  50 members x 40 six-hourly leads of 240 x 121 float32 into
                  10 days (the time axis in the middle)

  python tools/resample_bench.py [--reps R] [--pool-bytes B] [--only NAME]
  rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py --only weekly

Variants per shape: `mean` alone and `mean+min+max` in one launch, each with
`skipna` off and on, and rolling means with w = 4 and 28.  One JSON line per
run: ms per launch (a HIP event pair around every launch, median and min),
GB/s against the roofline of (n_time + n_stat * n_bin) * sizeof(T) bytes per
point (the input read once, every output written once) and that as a share of
8 TB/s.  In the same process:

  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape);
  * the torch expression a user would write today on the same tensors: for
    uniform bins `x.view(n_bin, k, P).mean(1)`, `.amin(1)`, `.amax(1)`, one
    launch each (nanmean and NaN-masked forms with skipna); for non-uniform
    bins `index_reduce_`; for rolling `unfold(...).mean(-1)`; with
    `torch_over_hip` and whether the two agree to rounding.

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
from weatherbench2_amd import _lib, engine, resampling

# name -> (n_outer, n_time, n_point, steps per bin, mean, spread)
SHAPES = {
    'hourly_daily': (1, 720, 1440 * 721, 24, 280.0, 8.0),
    'weekly': (1, 1464, 13 * 64 * 32, 28, 280.0, 8.0),
    'ensemble_leads': (50, 40, 240 * 121, 4, 0.0, 1.0),
}
VARIANTS = (('mean', ['mean']), ('mean_min_max', ['mean', 'min', 'max']))


def resample_ranges(n_time: int, k: int) -> np.ndarray:
  begin = np.arange(0, n_time, k)
  return np.stack([begin, np.minimum(begin + k, n_time)], 1).astype(np.int32)


def torch_resample(x, k, statistics, skipna):
  """[n_outer, n_time, P] -> {statistic: [n_outer, n_bin, P]}, one torch
  launch (or a few) per statistic."""
  n_outer, n_time, n_point = x.shape
  out = {}
  if n_time % k == 0:
    v = x.view(n_outer, n_time // k, k, n_point)
    for s in statistics:
      if s == 'mean':
        out[s] = v.nanmean(2) if skipna else v.mean(2)
      elif not skipna:
        out[s] = v.amin(2) if s == 'min' else v.amax(2)
      else:
        fill = float('inf') if s == 'min' else float('-inf')
        r = torch.where(v.isnan(), fill, v)
        r = r.amin(2) if s == 'min' else r.amax(2)
        out[s] = torch.where(v.isnan().all(2), float('nan'), r)
    return out
  if skipna:
    raise NotImplementedError('index_reduce_ has no NaN-skipping form')
  n_bin = -(-n_time // k)
  index = torch.arange(n_time, device=x.device) // k
  for s in statistics:
    res = torch.empty((n_outer, n_bin, n_point), dtype=x.dtype, device=x.device)
    res.index_reduce_(1, index, x, {'mean': 'mean', 'min': 'amin',
                                    'max': 'amax'}[s], include_self=False)
    out[s] = res
  return out


def torch_rolling_mean(x, w):
  out = torch.full_like(x, float('nan'))
  out[:, w - 1:] = x.unfold(1, w, 1).mean(-1)
  return out


def agree(got, want, rtol):
  """NaN in the same places; elsewhere within `rtol` of the largest value (two
  orders of summation: a mean near zero has no relative accuracy)."""
  a, b = got.nan_to_num(), want.nan_to_num()
  return bool(torch.equal(got.isnan(), want.isnan())
              and (a - b).abs().max() <= rtol * b.abs().max())


def run_shape(name, args):
  n_outer, n_time, n_point, k, mean, spread = SHAPES[name]
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  print(json.dumps({'shape': name, 'geometry_f32':
                    engine.time_window_geometry(torch.float32, True)}),
        flush=True)

  def report(kernel, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'kernel': kernel, 'ms_median': round(med, 4),
            'ms_min': round(best, 4), 'MB': round(n_bytes / 1e6, 1),
            'GBps': round(gbps, 1), 'frac_of_8TBps': round(gbps / 8000.0, 4)}
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

  in_bytes = 4 * n_outer * n_time * n_point
  n = min(32, max(2, int(args.pool_bytes // in_bytes)))
  pool = [torch.randn((n_outer, n_time, n_point), device=dev, generator=gen)
          * spread + mean for _ in range(n)]
  for x in pool:  # one value in a thousand missing
    x[torch.rand(x.shape, device=dev, generator=gen) < 1e-3] = float('nan')
  ranges = resample_ranges(n_time, k)
  bins = torch.from_numpy(ranges).to(dev)
  group = resampling._bins_per_group('resample', ranges)
  holder = [None]
  yardstick(name)
  for label, statistics in VARIANTS:
    for skipna in (False, True):
      n_bytes = 4 * n_outer * n_point * (n_time + len(statistics) * len(ranges))
      full = f'{name}_{label}_{"skipna" if skipna else "keepna"}'

      def launch(i):
        holder[0] = engine.time_bin_stats(pool[i], None, n_outer, n_time,
                                          n_point, bins, statistics, skipna,
                                          group)
      extra = {'n_outer': n_outer, 'n_time': n_time, 'n_point': n_point,
               'n_bin': len(ranges), 'n_stat': len(statistics),
               'bins_per_group': group, 'roofline_bytes_per_point':
               4 * (n_time + len(statistics) * len(ranges))}
      ours = report(full, n_bytes, timed(launch, n, args.reps), extra)
      if args.no_torch:
        continue
      try:
        want = torch_resample(pool[0], k, statistics, skipna)
      except NotImplementedError as e:
        print(json.dumps({'kernel': 'torch_' + full, 'not_run': str(e)}),
              flush=True)
        continue
      launch(0)
      same = all(agree(holder[0][s], want[s], 1e-5) for s in statistics)
      del want

      def launch_torch(i):
        holder[0] = torch_resample(pool[i], k, statistics, skipna)
      theirs = timed(launch_torch, n, max(5, args.reps // 4), warmup=2)
      report('torch_' + full, n_bytes, theirs,
             {'torch_over_hip': round(theirs[0] / ours, 2), 'agree': same,
              'form': 'view' if n_time % k == 0 else 'index_reduce'})
      holder[0] = None
  for w in (4, 28):
    rolling = torch.from_numpy(resampling.plan_rolling(n_time, w)).to(dev)
    n_bytes = 4 * n_outer * n_point * 2 * n_time
    full = f'{name}_rolling_{w}_mean'

    def launch(i):
      holder[0] = engine.time_bin_stats(
          pool[i], None, n_outer, n_time, n_point, rolling, ['mean'], False,
          resampling._ROLLING_BINS_PER_GROUP)
    ours = report(full, n_bytes, timed(launch, n, args.reps),
                  {'window': w, 'roofline_bytes_per_point': 8 * n_time})
    if not args.no_torch:
      want = torch_rolling_mean(pool[0], w)
      launch(0)
      same = agree(holder[0]['mean'], want, 1e-5)
      del want

      def launch_torch(i):
        holder[0] = torch_rolling_mean(pool[i], w)
      theirs = timed(launch_torch, n, max(5, args.reps // 4), warmup=2)
      report('torch_' + full, n_bytes, theirs,
             {'torch_over_hip': round(theirs[0] / ours, 2), 'agree': same})
    holder[0] = None
  yardstick('end')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool-bytes', type=float, default=3e9)
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
      rep = resource_report('time_window.hip')
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
