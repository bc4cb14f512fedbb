"""The conditional sums kernel alone (csrc/conditional_sums.hip, K24), one
process per shape, with the 13 evaluation regions' column classes, binned by
the spread and by the truth into B = 10 bins:

  ens50_240   50 members x 13 levels of 121 x 240 float32
  ens50_64    50 members x 13 levels of 32 x 64 float32

  python tools/conditional_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/conditional_bench.py \
      --only ens50_240

One JSON line per run, printed and appended to --out (default
profiles/conditional_bench.jsonl): ms per launch of wb2_conditional_sums (a HIP
event pair around every launch, median and min of --reps >= 10 launches over
alternating inputs, enough of them to exceed the 256 MiB Infinity Cache), GB/s
against the (M + 1) * sizeof B/point it has to read, and that as a share of
8 TB/s.  In the same process, on the same operands:

  * wb2_ens_partials (K3), the existing kernel that does the same read:
    `sums_over_k3`;
  * wb2_twcrps_sums (K21) with one threshold: `sums_over_k21`;
  * wb2_crps_bin_fold (n_slot = 4 B) + wb2_event_fold on the sums (the simple
    path: no speed claim);
  * the torch expression: mean, var, bucketize and a weighted index_add_ of the
    five terms for ONE region;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch
(expected 0), LDS and occupancy per instantiation (CPU side; needs hipcc)."""
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
from weatherbench2_amd import _lib, conditional, engine, events
from weatherbench2_amd import plan as plan_lib

SHAPES = {'ens50_240': (50, 13, 121, 240), 'ens50_64': (50, 13, 32, 64)}
N_BIN = 10
# nine edges in standard deviations about the spread of N(0, 1) members, and
# nine in the units of an N(0, 1) truth
CONFIGS = {'spread': tuple(0.8 + 0.05 * k for k in range(N_BIN - 1)),
           'truth': tuple(-1.6 + 0.4 * k for k in range(N_BIN - 1))}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'conditional_bench.jsonl')


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
  read = (n_member + 1) * 4 * n_point
  n = max(args.pool, -(-600_000_000 // read))
  pool = []
  for _ in range(n):
    ens = torch.randn((n_member, n_outer, n_row, n_col), device=dev,
                      generator=gen)
    truth = torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
    thr = 0.4 + 0.1 * torch.randn((n_outer, n_row, n_col), device=dev,
                                  generator=gen)
    pool.append((ens, truth, thr))
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'classes': n_class, 'bins': N_BIN, 'pool': n,
        'geometry': engine.conditional_geometry(torch.float32, n_member,
                                                n_class, N_BIN - 1)})
  yardstick(name)
  member_stride = n_outer * slab
  cls_dev = torch.from_numpy(col_class).to(dev)

  # K3 on the same operands: the same read, six slots per point
  pl = plan_lib.cached_plan(lat, lon, plan_lib.LATLON, regions, dev,
                            plan_lib.ENSEMBLE_ROWS_PER_CHUNK)
  prep = engine.PreparedLaunch(pl, lib.wb2_ens_tile_cols(pl.n_col),
                               lib.wb2_ens_num_slots(0), n_outer, pl.wfield)

  def launch_k3(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_ens_partials_maps(
        _lib.WB2_F32, 0, ens.data_ptr(), None, truth.data_ptr(), None,
        n_member, member_stride, n_outer, *prep.ens_args(),
        _lib.ptr(prep.partials), None, stream), 'wb2_ens_partials_maps')
  k3 = timed(launch_k3, n, args.reps)
  report('ens_partials_k3', k3, read,
         extra={'note': 'the K3 launch alone (no fold), same operands'})

  # K21 with one threshold on the same operands
  s21, c21 = engine.twcrps_sums(pool[0][0], member_stride, n_member, None,
                                pool[0][1], None, [pool[0][2]], None, n_outer,
                                n_row, n_col, col_class, n_class)
  ptrs = [_lib.ptr_array([p[2]]) for p in pool]

  def launch_k21(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_twcrps_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, ptrs[i],
        None, 1, n_member, member_stride, n_outer, n_row, n_col,
        cls_dev.data_ptr(), n_class, 0, s21.data_ptr(), c21.data_ptr(),
        stream), 'wb2_twcrps_sums')
  k21 = timed(launch_k21, n, args.reps)
  report('twcrps_sums_T1_k21', k21, (n_member + 2) * 4 * n_point)

  holder = [None]
  for by, given in CONFIGS.items():
    edges = conditional.kernel_edges(given, by)
    mode = engine.CONDITIONAL_MODES[by]
    # (checks the tables once and gives the sums the other paths are held to)
    sums, cnt = engine.conditional_sums(
        pool[0][0], member_stride, n_member, None, pool[0][1], None, n_outer,
        n_row, n_col, col_class, n_class, by, edges)
    outs = [(torch.empty_like(sums), torch.empty_like(cnt)) for _ in range(2)]
    edges_dev = torch.from_numpy(edges).to(dev)

    def launch(i):
      ens, truth, _ = pool[i]
      _lib.check(lib.wb2_conditional_sums(
          _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
          member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
          mode, edges_dev.data_ptr(), edges.size, outs[i % 2][0].data_ptr(),
          outs[i % 2][1].data_ptr(), stream), 'wb2_conditional_sums')
    ours = report(f'conditional_sums_{by}', timed(launch, n, args.reps), read,
                  extra={
        'by': by, 'bins': N_BIN, 'bytes_per_point': (n_member + 1) * 4,
        'read_MB': round(read / 1e6, 1),
        'written_MB': round((sums.numel() * 8 + cnt.numel() * 4) / 1e6, 2),
        'occupied_bins': int((cnt.sum(dim=(0, 1, 2)) > 0).sum()),
        'sums_over_k3': None, 'sums_over_k21': None})
    # (the ratios need the launch's own time: filled in before the file is
    # written, and printed once more)
    lines[-1]['sums_over_k3'] = round(ours / k3[0], 2)
    lines[-1]['sums_over_k21'] = round(ours / k21[0], 2)
    print(json.dumps({'shape': name, 'by': by,
                      'sums_over_k3': lines[-1]['sums_over_k3'],
                      'sums_over_k21': lines[-1]['sums_over_k21']}),
          flush=True)

    def launch_fold(i):
      holder[0] = engine.conditional_fold(sums, cnt, class_cols, wrow, mult)
    report(f'conditional_fold_{by}',
           timed(launch_fold, 1, args.reps, warmup=2),
           sums.numel() * 8 + cnt.numel() * 4,
           extra={'note': 'sums fold + count fold, the simple path, untuned, '
                          'Python launch layer included'})
    table, counts = (x.cpu().numpy() for x in holder[0])
    want = conditional.host_fold(sums.cpu().numpy(), cnt.cpu().numpy(),
                                 class_cols, wrow, mult)
    fold_same = bool(np.array_equal(table, want[0]) and
                     np.array_equal(counts, want[1]))

    if not args.no_torch:
      w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]
                           ).to(dev)
      wflat = w[None].expand(n_outer, n_row, n_col).reshape(-1)
      base = (torch.arange(n_outer, device=dev) * N_BIN)[:, None, None]

      def torch_form(ens, truth, _):
        x = ens.double()
        y = truth.double()
        mu = x.mean(0)
        s2 = x.var(0, unbiased=True)
        se = (mu - y) ** 2
        v = s2 if by == 'spread' else y
        which = (torch.bucketize(v, edges_dev, right=True) + base).reshape(-1)
        out = torch.zeros((n_outer * N_BIN, 5), dtype=torch.float64,
                          device=dev)
        terms = torch.stack([torch.ones_like(mu), mu, y, s2, se], dim=-1
                            ).reshape(-1, 5) * wflat[:, None]
        out.index_add_(0, which, terms)
        return out.reshape(n_outer, N_BIN, 5)
      got = torch_form(*pool[0])
      ref = torch.from_numpy(np.concatenate(
          [counts[:, 0, :N_BIN, None], table[:, 0]], axis=-1)).to(dev)
      agree = bool(torch.allclose(got, ref, rtol=1e-9, atol=1e-9))
      del got

      def launch_torch(i):
        holder[0] = torch_form(*pool[i])
      tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
      report(f'torch_{by}', tt, read, extra={
          'expression': 'mean, var, bucketize, weighted index_add_ of the '
                        'five terms (one region)',
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
    rep = resource_report('conditional_sums.hip')
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
