"""The CRPS bin-sum kernel alone (csrc/crps_bins.hip, K20), one process per
shape, with the 13 evaluation regions' column classes:

  ens50_240   50 members x 13 levels of 121 x 240 float32
  ens50_64    50 members x 13 levels of 32 x 64 float32

  python tools/crps_decomposition_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/crps_decomposition_bench.py \
      --only ens50_240

One JSON line per run, printed and appended to --out (default
profiles/crps_decomposition_bench.jsonl): ms per launch of wb2_crps_bin_sums
(a HIP event pair around every launch, median and min of --reps >= 10 launches
over alternating inputs, enough of them to exceed the 256 MiB Infinity Cache),
GB/s against the (M + 1) * sizeof B/point it has to read, and that as a share
of 8 TB/s.  In the same process, on the same operands:

  * wb2_crps_bin_fold + wb2_event_fold on the sums (the simple path: no speed
    claim);
  * wb2_ens_partials (K3), the existing kernel that does the same read and the
    same register sort with a much shorter reduction: `sums_over_k3`;
  * a torch expression: sort, diff, clamp, the weighted sums of one region;
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
from tools.event_bench import evaluation_regions
from tools.quantile_bench import resource_report
from weatherbench2_amd import _lib, crps_decomposition, engine, events
from weatherbench2_amd import plan as plan_lib

SHAPES = {'ens50_240': (50, 13, 121, 240), 'ens50_64': (50, 13, 32, 64)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'crps_decomposition_bench.jsonl')


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class = mult.shape[1]
  class_cols = np.bincount(col_class, minlength=n_class)
  slab = n_row * n_col
  n_point = n_outer * slab
  read = (n_member + 1) * 4 * n_point
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
    pool.append((ens, truth))
  geo = engine.crps_bins_geometry(torch.float32, n_member, n_class)
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'classes': n_class, 'pool': n,
        'read_MB': round(read / 1e6, 1),
        'bytes_per_point': (n_member + 1) * 4, 'geometry': geo})
  yardstick(name)

  # (checks the tables once and gives the sums the other paths are held to)
  member_stride = n_outer * slab
  sums, cnt = engine.crps_bin_sums(pool[0][0], member_stride, n_member, None,
                                   pool[0][1], None, n_outer, n_row, n_col,
                                   col_class, n_class)
  cls_dev = torch.from_numpy(col_class).to(dev)
  outs = [(torch.empty_like(sums), torch.empty_like(cnt)) for _ in range(2)]

  def launch(i):
    ens, truth = pool[i]
    _lib.check(lib.wb2_crps_bin_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
        member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
        outs[i % 2][0].data_ptr(), outs[i % 2][1].data_ptr(), stream),
               'wb2_crps_bin_sums')
  ours = report('crps_bin_sums', timed(launch, n, args.reps), extra={
      'written_MB': round((sums.numel() * 8 + cnt.numel() * 4) / 1e6, 2)})

  holder = [None]

  def launch_fold(i):
    holder[0] = engine.crps_bin_fold(sums, cnt, class_cols, wrow, mult)
  report('crps_bin_fold', timed(launch_fold, 1, args.reps, warmup=2),
         nbytes=sums.numel() * 8 + cnt.numel() * 4,
         extra={'note': 'sums fold + count fold, the simple path, untuned, '
                        'Python launch layer included'})
  table, counts = (x.cpu().numpy() for x in holder[0])
  want = crps_decomposition.host_fold(sums.cpu().numpy(), cnt.cpu().numpy(),
                                      class_cols, wrow, mult)
  fold_same = bool(np.array_equal(table, want[0]) and
                   np.array_equal(counts, want[1]))

  # K3 on the same operands: the same read and sort, six slots per point
  pl = plan_lib.cached_plan(lat, lon, plan_lib.LATLON, regions, dev,
                            plan_lib.ENSEMBLE_ROWS_PER_CHUNK)
  prep = engine.PreparedLaunch(pl, lib.wb2_ens_tile_cols(pl.n_col),
                               lib.wb2_ens_num_slots(0), n_outer, pl.wfield)

  def launch_k3(i):
    ens, truth = pool[i]
    _lib.check(lib.wb2_ens_partials_maps(
        _lib.WB2_F32, 0, ens.data_ptr(), None, truth.data_ptr(), None,
        n_member, member_stride, n_outer, *prep.ens_args(),
        _lib.ptr(prep.partials), None, stream), 'wb2_ens_partials_maps')
  k3 = timed(launch_k3, n, args.reps)
  report('ens_partials_k3', k3, extra={
      'sums_over_k3': round(ours / k3[0], 2),
      'note': 'the K3 launch alone (no fold), same operands'})

  if not args.no_torch:
    w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)

    def torch_form(ens, truth):
      xs = torch.sort(ens, dim=0).values.double()
      y = truth.double()[None]
      c = torch.minimum(torch.maximum(y, xs[:-1]), xs[1:])
      alpha = torch.cat([torch.zeros_like(y), c - xs[:-1],
                         torch.clamp(y - xs[-1:], min=0)])
      beta = torch.cat([torch.clamp(xs[:1] - y, min=0), xs[1:] - c,
                        torch.zeros_like(y)])
      return torch.stack([torch.einsum('boij,ij->ob', alpha, w),
                          torch.einsum('boij,ij->ob', beta, w)], dim=1)
    got = torch_form(*pool[0])
    ref = torch.from_numpy(table[:, 0]).to(dev)
    agree = bool(torch.allclose(got, ref, rtol=1e-9, atol=0))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, extra={
        'expression': 'sort, diff, clamp, einsum with the weights (one '
                      'region)',
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
    rep = resource_report('crps_bins.hip')
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
