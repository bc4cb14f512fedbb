"""The quantile-score sums kernel alone (csrc/quantile_score.hip, K28), one
process per shape, float32, with the 13 evaluation regions' column classes:

  ens50_l5, ens50_l16  50 members x 13 levels of 121 x 240, 5 and 16 quantile
                       levels ('linear')
  direct5              a deterministic-sized field, 13 levels of 721 x 1440, in
                       direct mode: 5 quantile slabs, their 5 levels
  det_l16              a deterministic forecast (M = 1) of that size, 16 levels

  python tools/quantile_score_bench.py [--reps R] [--only NAME] [--out PATH]
  python tools/quantile_score_bench.py --report-only        # on the CPU
  rocprofv3 --kernel-trace --stats -- python tools/quantile_score_bench.py --only direct5

One JSON line per run, printed and appended to --out (default
profiles/quantile_score_bench.jsonl): ms per launch of wb2_quantile_score_sums
(a HIP event pair around every launch, median and min of --reps >= 10 launches
over alternating inputs, enough of them to exceed the 256 MiB Infinity Cache),
GB/s against the (M + 1) * sizeof B/point roofline and that as a share of 8
TB/s.  In the same process, on the same operands:

  * wb2_crps_bin_sums (K20): the same read and the same sort, M + 1 bins;
  * wb2_conditional_sums (K24, by='forecast', 9 edges): the same walk;
  * the fold of the sums (wb2_crps_bin_fold, n_slot = 2 n_level, and
    wb2_event_fold, n_code = 2 n_level + 2; the simple path: no speed claim);
  * a torch expression: `torch.quantile` over the member dim (direct mode: the
    slabs as they are), the pinball loss and its weighted sum over ONE region;
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
from weatherbench2_amd import _lib, engine, events, quantile_scores

# members, outer, rows, columns, levels, direct
SHAPES = {'ens50_l5': (50, 13, 121, 240, 5, False),
          'ens50_l16': (50, 13, 121, 240, 16, False),
          'direct5': (5, 13, 721, 1440, 5, True),
          'det_l16': (1, 13, 721, 1440, 16, False)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'quantile_score_bench.jsonl')


def levels_of(n_level):
  if n_level == 5:
    return np.array(quantile_scores.DEFAULT_LEVELS)
  return (np.arange(n_level) + 0.5) / n_level


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col, n_level, direct = SHAPES[name]
  lat = np.linspace(-90, 90, n_row)
  lon = np.linspace(0, 360, n_col, endpoint=False)
  regions = evaluation_regions()
  col_class, mult, wrow = events.column_classes(regions, lat, lon)
  n_class = mult.shape[1]
  tau = levels_of(n_level)
  tables = engine.quantile_score_levels(tau, n_member, 'linear', direct)
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
    if direct:  # monotone quantile forecasts
      ens = ens.sort(dim=0).values.contiguous()
    pool.append((ens, truth))
  geo = engine.quantile_score_geometry(torch.float32, n_member, n_class,
                                       n_level, direct)
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'levels': tau.tolist(), 'direct': direct,
        'classes': n_class, 'pool': n, 'read_MB': round(read / 1e6, 1),
        'bytes_per_point': (n_member + 1) * 4, 'geometry': geo})
  yardstick(name)

  # (checks the tables once and gives the sums the other paths are held to)
  member_stride = n_outer * slab
  sums, cnt, valid = engine.quantile_score_sums(
      pool[0][0], member_stride, n_member, None, pool[0][1], None, n_outer,
      n_row, n_col, col_class, n_class, tables, direct)
  cls_dev = torch.from_numpy(col_class).to(dev)
  outs = [(torch.empty_like(sums), torch.empty_like(cnt),
           torch.empty_like(valid)) for _ in range(2)]
  lo, hi, t, tau_t, omt = engine._quantile_score_tables(tables, n_member,
                                                        direct)

  def launch(i):
    ens, truth = pool[i]
    s, c, v = outs[i % 2]
    _lib.check(lib.wb2_quantile_score_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
        member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
        int(direct), n_level, lo.ctypes.data, hi.ctypes.data, t.ctypes.data,
        tau_t.ctypes.data, omt.ctypes.data, s.data_ptr(), c.data_ptr(),
        v.data_ptr(), stream), 'wb2_quantile_score_sums')
  ours = report('quantile_score_sums', timed(launch, n, args.reps))

  # K20 on the same operands: the same read and sort
  k20_out = [(torch.empty((n_outer, n_row, n_class, 2, n_member + 1),
                          dtype=torch.float64, device=dev),
              torch.empty((n_outer, n_row, n_class, 3), dtype=torch.int32,
                          device=dev)) for _ in range(2)]

  def launch_k20(i):
    ens, truth = pool[i]
    s, c = k20_out[i % 2]
    _lib.check(lib.wb2_crps_bin_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None, n_member,
        member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(), n_class,
        s.data_ptr(), c.data_ptr(), stream), 'wb2_crps_bin_sums')
  k20 = timed(launch_k20, n, args.reps)
  report('crps_bin_sums', k20,
         extra={'quantile_score_over_k20': round(ours / k20[0], 2),
                'note': 'K20, the same members and truth'})

  # K24 on the same operands: the same walk
  edges = np.linspace(-1.6, 1.6, 11)[1:-1].astype(np.float64)
  edges_dev = torch.from_numpy(edges).to(dev)
  n_bin = edges.size + 1
  k24_out = [(torch.empty((n_outer, n_row, n_class, n_bin, 4),
                          dtype=torch.float64, device=dev),
              torch.empty((n_outer, n_row, n_class, n_bin), dtype=torch.int32,
                          device=dev)) for _ in range(2)]

  def launch_k24(i):
    ens, truth = pool[i]
    s, c = k24_out[i % 2]
    _lib.check(lib.wb2_conditional_sums(
        _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None,
        n_member, member_stride, n_outer, n_row, n_col, cls_dev.data_ptr(),
        n_class, 1, edges_dev.data_ptr(), edges.size, s.data_ptr(),
        c.data_ptr(), stream), 'wb2_conditional_sums')
  k24 = timed(launch_k24, n, args.reps)
  report('conditional_sums_b10', k24,
         extra={'quantile_score_over_k24': round(ours / k24[0], 2),
                'note': 'K24, by=forecast, 10 bins, the same members and '
                        'truth'})

  def launch_fold(i):
    engine.quantile_score_fold(sums, cnt, valid, None, wrow, mult)
  report('quantile_score_fold', timed(launch_fold, 1, args.reps),
         nbytes=sums.numel() * 8 + cnt.numel() * 4 + valid.numel() * 4,
         extra={'note': 'crps_bin_fold + event_fold with their uploads; the '
                        'simple path, untuned'})
  table, counts = engine.quantile_score_fold(sums, cnt, valid, None, wrow,
                                             mult)
  want = quantile_scores.host_fold(sums.cpu().numpy(), cnt.cpu().numpy(),
                                   valid.cpu().numpy(), None, wrow, mult)
  fold_same = bool(np.array_equal(table.cpu().numpy(), want[0]) and
                   np.array_equal(counts.cpu().numpy(), want[1]))

  if not args.no_torch:
    w = torch.from_numpy(wrow[0][:, None] * mult[0][col_class][None, :]).to(dev)
    tau_dev = torch.from_numpy(tau).to(dev)
    holder = [None]

    def torch_form(ens, truth):
      if direct:
        q = ens.double()
      else:
        # (torch.quantile refuses inputs over 16 M elements: one outer index
        # at a time)
        q = torch.stack([torch.quantile(ens[:, o], tau_dev.float(), dim=0)
                         for o in range(n_outer)], 1).double()
      u = truth.double()[None] - q
      lv = tau_dev.reshape(-1, 1, 1, 1)
      pin = torch.where(u >= 0, lv * u, (lv - 1.0) * u)
      return (w * pin).sum((-1, -2)).T  # [outer, level]
    got = torch_form(*pool[0])
    agree = bool(torch.allclose(got, table[:, 0, :, 0], rtol=1e-5, atol=0))
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch', tt, extra={
        'expression': 'torch.quantile over the members per outer index '
                      '(direct: none), pinball, one weighted sum per level '
                      '(one region, no NaN handling, no counts)',
        'torch_over_hip': round(tt[0] / ours, 2), 'agree': agree,
        'fold_bit_equal_to_host': fold_same})
    holder[0] = None
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def quantile_score_resources() -> dict:
  """`resource_report` of csrc/quantile_score.hip with the SGPRs and AGPRs of
  the same remarks and the dynamic LDS (the geometry's `lds_bytes`) spelt
  out."""
  import re
  from weatherbench2_amd import build
  rep = resource_report('quantile_score.hip')
  cmd = [build._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17',
         '-ffp-contract=off', '-fPIC', '-I' + os.path.join(build.ROOT, 'include'),
         '-I' + build.CSRC, '-Rpass-analysis=kernel-resource-usage',
         '--cuda-device-only', '-c',
         os.path.join(build.CSRC, 'quantile_score.hip'), '-o', os.devnull]
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
    v['lds_dynamic'] = ('max(n_member * 64 * sizeof(T), 64 * (2 n_level | 1) '
                        '* 8) + 256, at most 65536')
  return rep


def report_resources(out):
  try:
    rep = quantile_score_resources()
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
