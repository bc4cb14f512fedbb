"""The event-count kernel alone (csrc/event_table.hip, K18), one process per
shape, with the 13 evaluation regions' column classes:

  ens50_t1  50 members x 13 levels of 121 x 240 float32, 1 threshold
  ens50_t3  the same, 3 thresholds: ONE read of the members
  det_t3    a deterministic forecast (M = 1), 13 levels of 721 x 1440 float32,
            3 thresholds

  python tools/event_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/event_bench.py --only ens50_t3

One JSON line per run, printed and appended to --out (default
profiles/event_bench.jsonl): ms per launch of wb2_event_counts (a HIP event
pair around every launch, median and min of --reps >= 10 launches over
alternating inputs, enough of them to exceed the 256 MiB Infinity Cache), GB/s
against the (M + 1 + T) * sizeof B/point it has to read, and that as a share
of 8 TB/s.  In the same process, on the same operands:

  * wb2_event_fold on the counts (the simple path: no speed claim);
  * engine.ensemble_threshold_reduce, the existing exceedance kernel + fold:
    one launch per threshold, each reading the members again;
  * a torch expression: (ens > thr).sum(0), one-hot, weighted sum;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch
(expected 0) and occupancy per instantiation (CPU side; needs hipcc); the LDS
is dynamic: lds_bytes of the geometry line."""
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
from weatherbench2_amd import _lib, engine, events
from weatherbench2_amd import plan as plan_lib
from weatherbench2_amd import regions as regions_lib

SHAPES = {'ens50_t1': (50, 13, 121, 240, 1), 'ens50_t3': (50, 13, 121, 240, 3),
          'det_t3': (1, 13, 721, 1440, 3)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'event_bench.jsonl')


def evaluation_regions() -> dict:
  """scripts/evaluate.py:345-374 (the 13 slice regions)."""
  R = regions_lib.SliceRegion
  return {
      'global': R(),
      'tropics': R(lat_slice=slice(-20, 20)),
      'extra-tropics': R(lat_slice=[slice(None, -20), slice(20, None)]),
      'northern-hemisphere': R(lat_slice=slice(20, None)),
      'southern-hemisphere': R(lat_slice=slice(None, -20)),
      'europe': R(lat_slice=slice(35, 75),
                  lon_slice=[slice(360 - 12.5, None), slice(0, 42.5)]),
      'north-america': R(lat_slice=slice(25, 60),
                         lon_slice=slice(360 - 120, 360 - 75)),
      'north-atlantic': R(lat_slice=slice(25, 65),
                          lon_slice=slice(360 - 70, 360 - 10)),
      'north-pacific': R(lat_slice=slice(25, 60),
                         lon_slice=slice(145, 360 - 130)),
      'east-asia': R(lat_slice=slice(25, 60), lon_slice=slice(102.5, 150)),
      'ausnz': R(lat_slice=slice(-45, -12.5), lon_slice=slice(120, 175)),
      'arctic': R(lat_slice=slice(60, 90)),
      'antarctic': R(lat_slice=slice(-90, -60)),
  }


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col, n_thr = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class = mult.shape[1]
  n_code = events.n_codes(n_member)
  slab = n_row * n_col
  n_point = n_outer * slab
  read = (n_member + 1 + n_thr) * 4 * n_point
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  def report(kernel, ms, nbytes=read, extra=None):
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
  n = max(args.pool, -(-600_000_000 // read))
  pool = []
  for _ in range(n):
    ens = torch.randn((n_member, n_outer, n_row, n_col), device=dev,
                      generator=gen)
    truth = torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
    thrs = [torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
            * 0.3 + q for q in np.linspace(0.0, 1.5, n_thr)]
    pool.append((ens, truth, thrs))
  geo = engine.event_counts_geometry(torch.float32, n_member, n_class, n_thr,
                                     wide=True)
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'thresholds': n_thr, 'classes': n_class,
        'codes': n_code, 'pool': n, 'read_MB': round(read / 1e6, 1),
        'bytes_per_point': (n_member + 1 + n_thr) * 4, 'geometry': geo})
  yardstick(name)

  # (checks the tables once and gives the counts the other paths are held to)
  member_stride = n_outer * slab
  cnt = engine.event_counts(pool[0][0], member_stride, n_member, None,
                            pool[0][1], None, pool[0][2], None, n_outer, n_row,
                            n_col, col_class, n_class)
  cls_dev = torch.from_numpy(col_class).to(dev)
  outs = [torch.empty_like(cnt) for _ in range(2)]
  ptrs = [_lib.ptr_array(p[2]) for p in pool]

  def launch(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_event_counts(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, ptrs[i],
        None, n_thr, n_member, member_stride, n_outer, n_row, n_col,
        cls_dev.data_ptr(), n_class, outs[i % 2].data_ptr(), stream),
               'wb2_event_counts')
  ours = report('event_counts', timed(launch, n, args.reps))

  wrow_dev = torch.from_numpy(wrow).to(dev)
  mult_dev = torch.from_numpy(mult).to(dev)
  table = torch.empty((n_thr, n_outer, len(regions), n_code),
                      dtype=torch.float64, device=dev)

  def launch_fold(i):
    _lib.check(lib.wb2_event_fold(
        cnt.data_ptr(), n_thr * n_outer, n_row, n_class, n_code,
        wrow_dev.data_ptr(), mult_dev.data_ptr(), len(regions),
        table.data_ptr(), stream), 'wb2_event_fold')
  report('event_fold', timed(launch_fold, 1, args.reps),
         nbytes=cnt.numel() * 4, extra={'note': 'the simple path, untuned'})
  want = events.host_fold(cnt.cpu().numpy(), wrow, mult)
  fold_same = bool(np.array_equal(table.cpu().numpy(), want))

  # the existing exceedance kernel + fold: one pass per threshold
  pl = plan_lib.cached_plan(lat, lon, plan_lib.LATLON, regions, dev,
                            plan_lib.ENSEMBLE_ROWS_PER_CHUNK)

  def launch_existing(i):
    ens, truth, thrs = pool[i]
    for thr in thrs:
      engine.ensemble_threshold_reduce(pl, ens, member_stride, n_member, None,
                                       truth, None, thr, None, n_outer, False)
  theirs = timed(launch_existing, n, args.reps, warmup=2)
  report('ensemble_threshold_reduce', theirs,
         nbytes=n_thr * (n_member + 2) * 4 * n_point,
         extra={'launches': n_thr, 'existing_over_event_counts':
                round(theirs[0] / ours, 2),
                'note': 'partials + region fold per threshold, Python '
                        'launch layer included'})

  if not args.no_torch:
    w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)
    holder = [None]

    def torch_form(ens, truth, thrs):
      out = []
      for thr in thrs:
        k = (ens > thr).sum(0)
        code = (truth > thr) * (n_member + 1) + k
        onehot = torch.nn.functional.one_hot(code, n_code - 1).double()
        out.append(torch.einsum('oijc,ij->oc', onehot, w))
      return torch.stack(out)
    got = torch_form(*pool[0])
    ref = table[:, :, 0, :n_code - 1]
    agree = bool(torch.allclose(got, ref, rtol=1e-9, atol=0))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, extra={
        'expression': '(ens > thr).sum(0), one_hot, einsum with the weights '
                      '(one region)',
        'torch_over_hip': round(tt[0] / ours, 2), 'agree': agree,
        'fold_bit_equal_to_host': fold_same})
    holder[0] = None
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def report_resources(out):
  try:
    rep = resource_report('event_table.hip')
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
