"""The window-quantile kernel alone (csrc/climatology_quantile.hip, K15) on
three shapes, one process per shape:

  seeps_64x32     31 years (1990-2020) six-hourly of 64 x 32 float32
                  total_precipitation_24hr, W = 61, into 4 hours x 366 days:
                  SEEPS threshold and dry fraction
  seeps_240x121   the same at 240 x 121
  quantile_64x32  the first shape, three quantiles, no dry threshold

  python tools/seeps_climatology_bench.py [--reps R] [--only NAME]

One JSON line per measurement: ms per launch (a HIP event pair around every
launch, median and min; two inputs alternate).  The work model: the kernel is
not bound by memory; per output (position, point, quantile) it visits the N =
W * n_year rows of the window in LDS once per pass: one pass for the sums,
`passes` counting passes (6 key compares per row: 3 candidates for each of the
two ends; at most key bits / key_bits_per_pass of them, fewer by the leading
bits the window's keys share) and one last pass.  Reported are the rows
visited per second with the upper count of passes, and the time the input
alone would need at 8 TB/s.  In the same process:

  * K14's moments launch on the same input and plan (what mean and std cost);
  * the torch expression a user would write today (`unfold`, `sort`, `cumsum`:
    xarray's weighted quantile per point) on a slice of the points small
    enough to fit, no leap day and no fill, scaled to the whole grid as
    `torch_over_hip`, and whether it agrees with the kernel on that slice.

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
from weatherbench2_amd import climatology, engine

# name -> (n_point, quantiles, dry threshold in m or None)
SHAPES = {
    'seeps_64x32': (64 * 32, (2 / 3,), 0.25e-3),
    'seeps_240x121': (240 * 121, (2 / 3,), 0.25e-3),
    'quantile_64x32': (64 * 32, (0.1, 0.5, 0.9), None),
}
WINDOW = 61
HOURS = (0, 6, 12, 18)
TORCH_POINTS = 64


def precipitation(shape, dev, gen):
  """Gamma-like amounts in metres, about 45 % below 0.25 mm."""
  wet = torch.empty(shape, device=dev).exponential_(1 / 0.006, generator=gen)
  wet = wet + 0.25e-3
  dry = torch.rand(shape, device=dev, generator=gen) < 0.45
  return torch.where(dry, torch.zeros_like(wet), wet)


def torch_window_quantile(table, weights, qs, threshold):
  """xarray's weighted quantile of table [n_year, n_pos, n_point] over the
  cyclic window: float64 [n_q, n_pos, n_point]."""
  n_year, n_pos, n_point = table.shape
  half = weights.numel() // 2
  padded = torch.cat([table[:, -half:], table, table[:, :half]], dim=1)
  win = padded.unfold(1, weights.numel(), 1)       # [y, a, i, k]
  x = win.permute(1, 2, 0, 3).reshape(n_pos, n_point, -1).double()
  w = weights.double().expand(n_year, -1).reshape(-1).expand_as(x)
  drop = x.isnan() | (w == 0)
  if threshold is not None:
    drop = drop | (win.permute(1, 2, 0, 3).reshape(n_pos, n_point, -1)
                   < threshold)
  x = torch.where(drop, torch.full_like(x, float('inf')), x)
  w = torch.where(drop, torch.zeros_like(w), w)
  x, order = torch.sort(x, dim=-1)
  w = torch.gather(w, -1, order)
  w = w / w.sum(-1, keepdim=True)
  cum = torch.cat([torch.zeros_like(w[..., :1]), w.cumsum(-1)], dim=-1)
  n = 1.0 / (w * w).sum(-1, keepdim=True)
  x = torch.where(w == 0, torch.zeros_like(x), x)
  out = []
  for q in qs:
    h = (n - 1.0) * q + 1.0
    u = torch.maximum((h - 1.0) / n, torch.minimum(h / n, cum))
    v = u * n - h + 1.0
    out.append((x * v.diff(dim=-1)).sum(-1))
  return torch.stack(out)


def run_shape(name, args):
  n_point, qs, threshold = SHAPES[name]
  dev = engine.require_gpu()
  gen = torch.Generator(device=dev).manual_seed(0)
  times = np.arange(np.datetime64('1990-01-01', 'h'),
                    np.datetime64('2021-01-01', 'h'),
                    np.timedelta64(6, 'h')).astype('datetime64[ns]')
  n_time = len(times)
  plan = climatology.plan_groups(times, np.arange(n_time), 'explicit', HOURS)
  n_group = plan.n_cycle * plan.n_pos
  n_year = plan.n_year[0]
  geo = engine.window_quantile_geometry(torch.float32, n_year, WINDOW)
  print(json.dumps({'shape': name, 'n_time': n_time, 'n_point': n_point,
                    'n_group': n_group, 'n_year': n_year, 'window': WINDOW,
                    'geometry_f32': geo}), flush=True)
  pool = [precipitation((1, n_time, n_point), dev, gen) for _ in range(2)]
  member = torch.from_numpy(plan.member).to(dev)
  fill = torch.from_numpy(plan.fill).to(dev)
  m = np.ascontiguousarray(climatology._integer_weights(  # pylint: disable=protected-access
      climatology.create_window_weights(WINDOW).values))
  holder = [None]

  def launch(i):
    holder[0] = engine.window_quantile(
        pool[i], None, 1, n_time, n_point, plan.group_begin, plan.n_cycle,
        plan.n_pos, member, fill, m, qs, threshold,
        None if threshold is None else WINDOW * n_year)
  med, best = timed(launch, 2, args.reps, warmup=2)
  rows = WINDOW * n_year
  outputs = n_group * n_point * len(qs)
  passes_max = 2 + 32 // geo['key_bits_per_pass']
  in_bytes = 4 * n_time * n_point
  print(json.dumps({
      'shape': name, 'kernel': 'window_quantile_f32', 'ms_median': round(med, 3),
      'ms_min': round(best, 3), 'outputs': outputs, 'window_rows': rows,
      'rows_visited_per_s_at_most': round(outputs * rows * passes_max
                                          / med * 1e3, 0),
      'outputs_per_s': round(outputs / med * 1e3, 0),
      'input_MB': round(in_bytes / 1e6, 1),
      'ms_for_the_input_at_8TBps': round(in_bytes / 8e12 * 1e3, 5)}),
        flush=True)
  ours = med
  holder[0] = None

  pivots = [engine.first_finite(x, None, 1, n_time, n_point, member)
            for x in pool]

  def launch_moments(i):
    holder[0] = engine.group_moments(pool[i], None, 1, n_time, n_point,
                                     plan.group_begin, member, fill, pivots[i])
  med14, best14 = timed(launch_moments, 2, args.reps, warmup=2)
  print(json.dumps({'shape': name, 'kernel': 'group_moments_f32',
                    'ms_median': round(med14, 3), 'ms_min': round(best14, 3),
                    'window_quantile_over_moments': round(ours / med14, 1)}),
        flush=True)
  holder[0] = None

  if not args.no_torch:
    # a slice without leap day and fill: [n_year, 365, TORCH_POINTS] of hour 0
    n_pos = 365
    table = precipitation((n_year, n_pos, TORCH_POINTS), dev, gen)
    weights = torch.from_numpy(m.astype(np.float32)).to(dev)
    want = torch_window_quantile(table, weights, qs, threshold)
    begin = (np.arange(n_pos + 1) * n_year).astype(np.int32)
    mem = (np.arange(n_year)[None, :] * n_pos
           + np.arange(n_pos)[:, None]).astype(np.int32).ravel()
    got, _ = engine.window_quantile(
        table.reshape(1, n_year * n_pos, TORCH_POINTS), None, 1,
        n_year * n_pos, TORCH_POINTS, begin, 1, n_pos,
        torch.from_numpy(mem).to(dev), None, m, qs, threshold)
    agree = bool(((got[:, 0] - want).abs() <= 1e-9 * want.abs().max()).all())

    def launch_torch(i):
      holder[0] = torch_window_quantile(table, weights, qs, threshold)
    theirs = timed(launch_torch, 1, max(3, args.reps // 4), warmup=1)
    scale = (n_group * n_point) / (n_pos * TORCH_POINTS)
    print(json.dumps({'shape': name, 'kernel': 'torch_unfold_sort_cumsum',
                      'slice_points': TORCH_POINTS, 'slice_positions': n_pos,
                      'ms_median_slice': round(theirs[0], 3),
                      'ms_scaled_to_the_shape': round(theirs[0] * scale, 1),
                      'torch_over_hip': round(theirs[0] * scale / ours, 1),
                      'agree': agree}), flush=True)
    holder[0] = None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=10)
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
           '--reps', str(args.reps)]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    try:
      rep = resource_report('climatology_quantile.hip')
      spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
      for k, v in rep.items():
        v['lds_dynamic'] = ('(positions + n_w - 1) * n_year * tile * sizeof(T)'
                            ' + 4 * n_w * n_year, at most 163840')
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
