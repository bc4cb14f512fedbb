"""The neighbourhood kernels alone (csrc/neighborhood.hip, K19), one process
per shape, with the 13 evaluation regions' column classes:

  det    a deterministic forecast (M = 1), 13 levels of 721 x 1440 float32,
         3 thresholds, windows (1, 5, 9, 17, 33, 65)
  ens50  50 members x 13 levels of 121 x 240 float32, 3 thresholds, windows
         (1, 3, 5, 9)

  python tools/fss_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/fss_bench.py --only det

One JSON line per run, printed and appended to --out (default
profiles/fss_bench.jsonl): ms per call (a HIP event pair around every call,
median and min of --reps >= 10 calls over alternating inputs, enough of them to
exceed the 256 MiB Infinity Cache) of

  * wb2_event_codes against the (M + 1 + T) * sizeof + 2 T B/point it moves,
    and wb2_event_counts (K18) on the same operands beside it;
  * wb2_fss_sums (all its launches) against 2 T B/point of codes read once
    plus the sums written;
  * wb2_fss_fold (one wave per (cell, window, region); untuned);
  * a torch expression on the same operands: indicator, circular pad,
    avg_pool2d per window, the weighted sums of one region;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch
(expected 0) and occupancy per instantiation (CPU side; needs hipcc); the LDS
of the box sum is dynamic: lds_bytes of the geometry line."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.derived_bench import timed
from tools.event_bench import evaluation_regions
from tools.quantile_bench import resource_report
from weatherbench2_amd import _lib, engine, events
from weatherbench2_amd import neighborhood as nb

SHAPES = {'det': (1, 13, 721, 1440, 3, (1, 5, 9, 17, 33, 65)),
          'ens50': (50, 13, 121, 240, 3, (1, 3, 5, 9))}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'fss_bench.jsonl')


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col, n_thr, windows = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class, n_region, n_window = mult.shape[1], len(regions), len(windows)
  slab = n_row * n_col
  n_point = n_outer * slab
  n_cell = n_thr * n_outer
  moved = ((n_member + 1 + n_thr) * 4 + 2 * n_thr) * n_point
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  def report(kernel, ms, nbytes, extra=None):
    med, best = ms
    gbps = nbytes / med / 1e6
    line = {'shape': name, 'kernel': kernel, 'ms_median': round(med, 4),
            'ms_min': round(best, 4), 'GBps': round(gbps, 1),
            'frac_of_8TBps': round(gbps / 8000.0, 4)}
    line.update(extra or {})
    emit(line)
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
    med, best = timed(launch, len(ws), args.reps)
    gbps = 12 * n_ws / med / 1e6
    emit({'shape': name, 'kernel': 'wind_speed_f32', 'before': before,
          'ms_median': round(med, 4), 'ms_min': round(best, 4),
          'GBps': round(gbps, 1), 'frac_of_8TBps': round(gbps / 8000.0, 4)})

  # alternating inputs, together larger than the Infinity Cache
  n = max(args.pool, -(-600_000_000 // moved))
  pool = []
  for _ in range(n):
    ens = torch.randn((n_member, n_outer, n_row, n_col), device=dev,
                      generator=gen)
    truth = torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
    thrs = [torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
            * 0.3 + q for q in np.linspace(0.0, 1.5, n_thr)]
    pool.append((ens, truth, thrs))
  geo = engine.fss_sums_geometry(n_col, n_class, n_window)
  sums_bytes = n_cell * n_window * n_row * n_class * 6 * 8
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'thresholds': n_thr, 'windows': list(windows),
        'classes': n_class, 'pool': n, 'codes_moved_MB': round(moved / 1e6, 1),
        'bytes_per_point': (n_member + 1 + n_thr) * 4 + 2 * n_thr,
        'sums_MB': round(sums_bytes / 1e6, 1), 'geometry': geo,
        'sums_launches': -(-n_window // geo['windows_per_launch'])})
  yardstick(name)

  # (checks the tables once and gives the codes the other kernels read)
  member_stride = n_outer * slab
  codes = [engine.event_codes(p[0], member_stride, n_member, None, p[1], None,
                              p[2], None, n_outer, n_row, n_col) for p in pool]
  ptrs = [_lib.ptr_array(p[2]) for p in pool]
  code_out = [torch.empty_like(codes[0]) for _ in range(2)]

  def launch_codes(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_event_codes(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, ptrs[i],
        None, n_thr, n_member, member_stride, n_outer, n_row, n_col,
        code_out[i % 2].data_ptr(), stream), 'wb2_event_codes')
  ours = report('event_codes', timed(launch_codes, n, args.reps), moved)

  cls_dev = torch.from_numpy(col_class).to(dev)
  cnt = [torch.empty((n_thr, n_outer, n_row, n_class,
                      events.n_codes(n_member)), dtype=torch.int32,
                     device=dev) for _ in range(2)]

  def launch_counts(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_event_counts(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, ptrs[i],
        None, n_thr, n_member, member_stride, n_outer, n_row, n_col,
        cls_dev.data_ptr(), n_class, cnt[i % 2].data_ptr(), stream),
               'wb2_event_counts')
  counts = timed(launch_counts, n, args.reps)
  report('event_counts', counts, (n_member + 1 + n_thr) * 4 * n_point,
         extra={'codes_over_counts': round(ours / counts[0], 2)})

  win = (np.asarray(windows, dtype=np.int32))
  win_p = win.ctypes.data_as(_lib._c.POINTER(_lib._i32))
  sums = [torch.empty((n_cell, n_window, n_row, n_class, 6),
                      dtype=torch.int64, device=dev) for _ in range(2)]

  def launch_sums(i):
    _lib.check(lib.wb2_fss_sums(
        codes[i].data_ptr(), n_cell, n_row, n_col, n_member, win_p, n_window,
        cls_dev.data_ptr(), n_class, sums[i % 2].data_ptr(), stream),
               'wb2_fss_sums')
  box_ms = timed(launch_sums, n, args.reps)
  box = report('fss_sums', box_ms, 2 * n_thr * n_point + sums_bytes,
               extra={'ns_per_point_and_window': round(
                   box_ms[0] * 1e6 / (n_thr * n_point * n_window), 5)})

  # the pseudo-region rides along, as in the metric
  mult1 = np.concatenate([mult, np.ones((1, n_class), np.int32)])
  wrow1 = np.concatenate([wrow, np.ones((1, n_row))])
  w = nb.window_weights(wrow1, n_member, windows)
  w_dev = torch.from_numpy(w).to(dev)
  mult_dev = torch.from_numpy(mult1).to(dev)
  table = torch.empty((n_cell, n_window, n_region + 1, 6),
                      dtype=torch.float64, device=dev)
  launch_sums(0)

  def launch_fold(i):
    _lib.check(lib.wb2_fss_fold(
        sums[0].data_ptr(), n_cell, n_window, n_row, n_class,
        w_dev.data_ptr(), mult_dev.data_ptr(), n_region + 1, table.data_ptr(),
        stream), 'wb2_fss_fold')
  fold = report('fss_fold', timed(launch_fold, 1, args.reps), sums_bytes,
                extra={'note': 'one wave per (cell, window, region), untuned'})
  emit({'shape': name, 'kernel': 'codes + sums + fold',
        'ms_median': round(ours + box + fold, 4)})
  comp = nb.components(table.cpu().numpy(), slab, True)
  comp = comp.reshape(n_thr, n_outer, n_window, n_region, 4)
  same = None
  if name == 'ens50':  # (the host path at the large grid takes minutes)
    host = nb.host_fold(nb.host_sums(codes[0].cpu().numpy(), windows, n_member,
                                     col_class, n_class), w, mult1)
    same = bool(np.array_equal(table.cpu().numpy(), host))

  if not args.no_torch:
    weight = torch.from_numpy(
        wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)
    total = weight.sum()
    holder = [None]
    pool2d = torch.nn.functional.avg_pool2d

    def torch_form(ens, truth, thrs):
      out = []
      for thr in thrs:
        p_f = (ens > thr).float().mean(0)[:, None]
        p_o = (truth > thr).float()[:, None]
        per = []
        for n_ in windows:
          h = n_ // 2
          f, o = (pool2d(torch.nn.functional.pad(x, (h, h, 0, 0),
                                                 mode='circular'),
                         (n_, n_), stride=1, padding=(h, 0),
                         count_include_pad=False)[:, 0].double()
                  for x in (p_f, p_o))
          per.append(torch.stack(
              [((f - o) ** 2 * weight).sum((-2, -1)),
               ((f * f + o * o) * weight).sum((-2, -1)),
               (f * weight).sum((-2, -1)), (o * weight).sum((-2, -1))],
              -1) / total)
        out.append(torch.stack(per, 1))
      return torch.stack(out)  # [T, outer, window, 4]
    got = torch_form(*pool[0]).cpu().numpy()
    agree = bool(np.allclose(got, comp[:, :, :, 0], rtol=1e-4, atol=1e-7))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, moved, extra={
        'expression': 'indicator, circular pad, avg_pool2d per window, '
                      'weighted sums (one region)',
        'torch_over_hip': round(tt[0] / (ours + box + fold), 2),
        'agree': agree, 'table_bit_equal_to_host': same})
    holder[0] = None
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def report_resources(out):
  try:
    rep = resource_report('neighborhood.hip')
  except (OSError, subprocess.CalledProcessError) as e:
    print(json.dumps({'resource_report': f'not available: {e}'}))
    return
  spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
  with open(out, 'a') as f:
    for k, v in rep.items():
      line = json.dumps({'instantiation': k, **v})
      print(line)
      f.write(line + '\n')
  print(json.dumps({'instantiations': len(rep), 'with_scratch': spills,
                    'max_vgprs': max(v['vgprs'] for v in rep.values())}))
  assert not spills, spills


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool', type=int, default=2)
  ap.add_argument('--only', default=None)
  ap.add_argument('--out', default=DEFAULT_OUT)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--report-only', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  if args.reps < 10:
    raise SystemExit('--reps must be at least 10')
  if args.report_only:
    report_resources(args.out)
    return
  if args.only is not None:
    if args.only not in SHAPES:
      raise SystemExit(f'--only must be one of {list(SHAPES)}')
    run_shape(args.only, args)
    return
  # one fresh process per shape: nothing of one shape's pool, allocator state
  # or clocks carries into the next
  for name in SHAPES:
    cmd = [sys.executable, os.path.abspath(__file__), '--only', name,
           '--reps', str(args.reps), '--pool', str(args.pool), '--out',
           args.out]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    report_resources(args.out)


if __name__ == '__main__':
  main()
