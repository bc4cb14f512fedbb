"""The joint-count kernel alone (csrc/joint_counts.hip, K26), one process per
shape, with the 13 evaluation regions' column classes:

  ens50_b4, ens50_b10  50 members x 13 levels of 121 x 240 float32, B = 4 and
                       B = 10 categories
  det_b4, det_b10      a deterministic forecast (M = 1), 13 levels of 721 x
                       1440 float32

The forecast is the truth plus noise of half its spread, so that most points
lie on or next to the diagonal of the table, as a useful forecast has them:
the LDS adds of a wave then meet in few addresses.

  python tools/joint_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/joint_bench.py --only det_b10

One JSON line per run, printed and appended to --out (default
profiles/joint_bench.jsonl): ms per launch of wb2_joint_counts (a HIP event
pair around every launch, median and min of --reps >= 10 launches over
alternating inputs, enough of them to exceed the 256 MiB Infinity Cache), GB/s
against the (M + 1) * sizeof B/point it has to read, and that as a share of 8
TB/s.  In the same process, on the same operands:

  * wb2_event_counts (K18) with ONE threshold: the existing counting kernel,
    the yardstick ((M + 2) elements per point: it reads a threshold field);
  * wb2_event_fold on the joint counts (n_code = B * B + 1; the simple path:
    no speed claim);
  * a torch expression: bucketize, then one weighted bincount of ONE region;
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
from weatherbench2_amd import _lib, distribution, engine, events

SHAPES = {'ens50_b4': (50, 13, 121, 240, 4), 'ens50_b10': (50, 13, 121, 240, 10),
          'det_b4': (1, 13, 721, 1440, 4), 'det_b10': (1, 13, 721, 1440, 10)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'joint_bench.jsonl')


def category_edges(n_bin: int) -> np.ndarray:
  """B - 1 edges of equal standard-normal mass steps, roughly: -1.6 .. 1.6."""
  return np.linspace(-1.6, 1.6, n_bin + 1)[1:-1].astype(np.float64)


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col, n_bin = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class = mult.shape[1]
  edges = category_edges(n_bin)
  n_code = distribution.n_codes(edges.size)
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
    truth = torch.randn((n_outer, n_row, n_col), device=dev, generator=gen)
    ens = truth[None] + 0.5 * torch.randn(
        (n_member, n_outer, n_row, n_col), device=dev, generator=gen)
    thr = torch.zeros((n_outer, n_row, n_col), device=dev)
    pool.append((ens, truth, thr))
  geo = engine.joint_geometry(torch.float32, n_member, n_class, edges.size,
                              wide=True)
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'categories': n_bin, 'classes': n_class,
        'codes': n_code, 'pool': n, 'read_MB': round(read / 1e6, 1),
        'bytes_per_point': (n_member + 1) * 4, 'geometry': geo})
  yardstick(name)

  # (checks the tables once and gives the counts the other paths are held to)
  member_stride = n_outer * slab
  cnt = engine.joint_counts(pool[0][0], member_stride, n_member, None,
                            pool[0][1], None, n_outer, n_row, n_col, col_class,
                            n_class, edges, 'right')
  diagonal = float(cnt[..., :n_code - 1].reshape(-1, n_bin, n_bin).sum(0)
                   .diagonal().sum() / cnt[..., :n_code - 1].sum())
  cls_dev = torch.from_numpy(col_class).to(dev)
  edges_dev = torch.from_numpy(edges).to(dev)
  outs = [torch.empty_like(cnt) for _ in range(2)]

  def launch(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_joint_counts(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
        member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
        edges_dev.data_ptr(), edges.size, 0, outs[i % 2].data_ptr(), stream),
               'wb2_joint_counts')
  ours = report('joint_counts', timed(launch, n, args.reps),
                extra={'diagonal_share': round(diagonal, 3)})

  # K18 with one threshold on the same operands: the existing code
  ev_cnt = [torch.empty((1, n_outer, n_row, n_class,
                         events.n_codes(n_member)), dtype=torch.int32,
                        device=dev) for _ in range(2)]
  ptrs = [_lib.ptr_array([p[2]]) for p in pool]

  def launch_k18(i):
    ens, truth, _ = pool[i]
    _lib.check(lib.wb2_event_counts(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, ptrs[i],
        None, 1, n_member, member_stride, n_outer, n_row, n_col,
        cls_dev.data_ptr(), n_class, ev_cnt[i % 2].data_ptr(), stream),
               'wb2_event_counts')
  k18 = timed(launch_k18, n, args.reps)
  report('event_counts_t1', k18, nbytes=(n_member + 2) * 4 * n_point,
         extra={'joint_over_k18': round(ours / k18[0], 2),
                'note': 'K18, one threshold, the same members and truth'})

  wrow_dev = torch.from_numpy(wrow).to(dev)
  mult_dev = torch.from_numpy(mult).to(dev)
  table = torch.empty((n_outer, len(regions), n_code), dtype=torch.float64,
                      device=dev)

  def launch_fold(i):
    _lib.check(lib.wb2_event_fold(
        cnt.data_ptr(), n_outer, n_row, n_class, n_code, wrow_dev.data_ptr(),
        mult_dev.data_ptr(), len(regions), table.data_ptr(), stream),
               'wb2_event_fold')
  report('event_fold', timed(launch_fold, 1, args.reps),
         nbytes=cnt.numel() * 4, extra={'note': 'the simple path, untuned'})
  want = distribution.host_fold(cnt.cpu().numpy(), wrow, mult)
  fold_same = bool(np.array_equal(table.cpu().numpy(), want))

  if not args.no_torch:
    w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)
    holder = [None]
    edges32 = edges_dev
    offset = (torch.arange(n_outer, device=dev) * (n_bin * n_bin)
              ).reshape(1, n_outer, 1, 1)

    def torch_form(ens, truth, _):
      yb = torch.bucketize(truth.double(), edges32, right=True)
      xb = torch.bucketize(ens.double(), edges32, right=True)
      code = (yb[None] * n_bin + xb + offset).reshape(-1)
      weights = w.expand(n_member, n_outer, n_row, n_col).reshape(-1)
      return torch.bincount(code, weights=weights,
                            minlength=n_outer * n_bin * n_bin
                            ).reshape(n_outer, n_bin * n_bin)
    got = torch_form(*pool[0])
    agree = bool(torch.allclose(got, table[:, 0, :n_code - 1], rtol=1e-9,
                                atol=0))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, extra={
        'expression': 'bucketize(truth), bucketize(ens), bincount with the '
                      'weights (one region)',
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
    rep = resource_report('joint_counts.hip')
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
