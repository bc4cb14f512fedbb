"""The variogram-sums kernel alone (csrc/variogram.hip, K27), one process per
shape, with the default lags and the 13 evaluation regions' column classes:

  ens50_o05, ens50_o2  50 members x 13 levels of 121 x 240 float32, orders 0.5
                       and 2
  det_o05, det_o2      a deterministic forecast (M = 1), 13 levels of 721 x
                       1440 float32

  python tools/variogram_bench.py [--reps R] [--only NAME] [--out PATH]
  python tools/variogram_bench.py --report-only        # on the CPU
  rocprofv3 --kernel-trace --stats -- python tools/variogram_bench.py --only det_o2

One JSON line per run, printed and appended to --out (default
profiles/variogram_bench.jsonl): ms per launch of wb2_variogram_sums (a HIP
event pair around every launch, median and min of --reps >= 10 launches over
alternating inputs, enough of them to exceed the 256 MiB Infinity Cache), GB/s
against the (M + 1) * sizeof B/point roofline -- every element counted ONCE,
although the kernel requests each one per distinct row offset and expects the
repeats from the caches -- and that as a share of 8 TB/s.  In the same
process, on the same operands:

  * wb2_conditional_sums (K24, by='forecast', 9 edges): the parent in the
    class-sums layer, which reads every element once;
  * the fold of the variogram sums (wb2_crps_bin_fold, n_slot = 3 n_lag, and
    wb2_event_fold, n_code = 2 n_lag; the simple path: no speed claim);
  * a torch expression: per lag `roll`, subtract, g (`abs().sqrt()` for order
    0.5), the member mean, the squared difference and three weighted sums of
    ONE region;
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
from weatherbench2_amd import _lib, engine, events, structure

SHAPES = {'ens50_o05': (50, 13, 121, 240, 0.5), 'ens50_o2': (50, 13, 121, 240, 2),
          'det_o05': (1, 13, 721, 1440, 0.5), 'det_o2': (1, 13, 721, 1440, 2)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'variogram_bench.jsonl')


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col, order = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class = mult.shape[1]
  lags = engine.variogram_lags(structure.DEFAULT_LAGS)
  n_lag = lags.shape[0]
  code = engine.variogram_order(order)
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
    pool.append((ens, truth))
  geo = engine.variogram_geometry(torch.float32, n_member, n_class, order, lags)
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'order': order, 'classes': n_class,
        'lags': lags.tolist(), 'pool': n, 'read_MB': round(read / 1e6, 1),
        'bytes_per_point': (n_member + 1) * 4, 'geometry': geo})
  yardstick(name)

  # (checks the tables once and gives the sums the other paths are held to)
  member_stride = n_outer * slab
  sums, cnt = engine.variogram_sums(pool[0][0], member_stride, n_member, None,
                                    pool[0][1], None, n_outer, n_row, n_col,
                                    col_class, n_class, order, lags)
  cls_dev = torch.from_numpy(col_class).to(dev)
  outs = [(torch.empty_like(sums), torch.empty_like(cnt)) for _ in range(2)]

  def launch(i):
    ens, truth = pool[i]
    s, c = outs[i % 2]
    _lib.check(lib.wb2_variogram_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
        member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
        code, lags.ctypes.data, n_lag, s.data_ptr(), c.data_ptr(), stream),
               'wb2_variogram_sums')
  ours = report('variogram_sums', timed(launch, n, args.reps))

  # K24 on the same operands: the parent in the class-sums layer
  edges = np.linspace(-1.6, 1.6, 11)[1:-1].astype(np.float64)
  edges_dev = torch.from_numpy(edges).to(dev)
  n_bin = edges.size + 1
  k24_out = [(torch.empty((n_outer, n_row, n_class, n_bin, 4),
                          dtype=torch.float64, device=dev),
              torch.empty((n_outer, n_row, n_class, n_bin), dtype=torch.int32,
                          device=dev)) for _ in range(2)]
  k24_members = min(n_member, engine.conditional_geometry(torch.float32)[
      'max_member'])

  def launch_k24(i):
    ens, truth = pool[i]
    s, c = k24_out[i % 2]
    _lib.check(lib.wb2_conditional_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None,
        k24_members, member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(),
        n_class, 1, edges_dev.data_ptr(), edges.size, s.data_ptr(),
        c.data_ptr(), stream), 'wb2_conditional_sums')
  k24 = timed(launch_k24, n, args.reps)
  report('conditional_sums_b10', k24,
         extra={'variogram_over_k24': round(ours / k24[0], 2),
                'note': 'K24, by=forecast, 10 bins, the same members and '
                        'truth'})

  def launch_fold(i):
    engine.variogram_fold(sums, cnt, None, wrow, mult)
  report('variogram_fold', timed(launch_fold, 1, args.reps),
         nbytes=sums.numel() * 8 + cnt.numel() * 4,
         extra={'note': 'crps_bin_fold + event_fold with their uploads; the '
                        'simple path, untuned'})
  table, counts = engine.variogram_fold(sums, cnt, None, wrow, mult)
  want = structure.host_fold(sums.cpu().numpy(), cnt.cpu().numpy(), None, wrow,
                             mult)
  fold_same = bool(np.array_equal(table.cpu().numpy(), want[0]) and
                   np.array_equal(counts.cpu().numpy(), want[1]))

  if not args.no_torch:
    w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)
    holder = [None]

    def g(d):
      if order == 2:
        return d * d
      return d.abs().sqrt() if order == 0.5 else d.abs()

    def torch_form(ens, truth):
      out = []
      for a, b in lags.tolist():
        rows = n_row - a
        wa = w[:rows]
        shift = lambda x: torch.roll(x[..., a:, :], -b, -1)
        gy = g(truth[..., :rows, :].double() - shift(truth).double())
        gf = g(ens[..., :rows, :].double() - shift(ens).double()).mean(0)
        sc = (gy - gf) ** 2
        out.append(torch.stack([(wa * gy).sum((-1, -2)),
                                (wa * gf).sum((-1, -2)),
                                (wa * sc).sum((-1, -2))], -1))
      return torch.stack(out, -2)  # [outer, lag, 3]
    got = torch_form(*pool[0])
    agree = bool(torch.allclose(got, table[:, 0], rtol=1e-9, atol=0))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, extra={
        'expression': 'per lag: roll, subtract, g, member mean, squared '
                      'difference, three weighted sums (one region, no NaN '
                      'handling)',
        'torch_over_hip': round(tt[0] / ours, 2), 'agree': agree,
        'fold_bit_equal_to_host': fold_same})
    holder[0] = None
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def variogram_resources() -> dict:
  """`resource_report` of csrc/variogram.hip with the SGPRs and AGPRs of the
  same remarks and the dynamic LDS (the geometry's `lds_bytes`) spelt out."""
  import re
  from weatherbench2_amd import build
  rep = resource_report('variogram.hip')
  cmd = [build._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17',
         '-ffp-contract=off', '-fPIC', '-I' + os.path.join(build.ROOT, 'include'),
         '-I' + build.CSRC, '-Rpass-analysis=kernel-resource-usage',
         '--cuda-device-only', '-c', os.path.join(build.CSRC, 'variogram.hip'),
         '-o', os.devnull]
  text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
  extra = []
  for line in text.splitlines():
    if 'Function Name:' in line:
      extra.append({})
    for key, pat in (('sgprs', r'TotalSGPRs: (\d+)'), ('agprs', r' AGPRs: (\d+)'),
                     ('sgprs_in_vgpr_lanes', r'SGPRs Spill: (\d+)')):
      m = re.search(pat, line)
      if m and extra:
        extra[-1][key] = int(m.group(1))
  # (both passes list the instantiations in the compiler's one order)
  if len(extra) == len(rep):
    for v, more in zip(rep.values(), extra):
      v.update(more)
  for v in rep.values():
    v['lds_dynamic'] = ('max(4 * n_off * 128 * sizeof(T), 64 * (3 n_lag | 1) '
                        '* 8) + 256, at most 65536')
  return rep


def report_resources(out):
  try:
    rep = variogram_resources()
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
