"""The cross-spectrum rows kernel alone (csrc/cross_spectrum.hip, K25), one
process per shape:

  det_1440    deterministic, 13 levels of 721 x 1440 float32
  ens50_240   50 members x 13 levels of 121 x 240 float32

  python tools/cross_spectrum_bench.py [--reps R] [--only NAME] [--out PATH]

Not a gate.  One JSON line per run, printed and appended to --out (default
profiles/cross_spectrum_bench.jsonl): ms per launch of wb2_cross_spectrum_rows
(a HIP event pair around every launch, median and min of --reps >= 10 launches
over alternating inputs, enough of them to exceed the 256 MiB Infinity Cache),
GB/s against the ((M + 1) * N * sizeof + 4 * NB * 8 + 8) bytes per row it has
to move, and that as a share of 8 TB/s.  In the same process, on the same rows:

  * the M + 1 existing wb2_zonal_spectrum launches (the two powers of every
    member and the truth; they give less: no phase): `rows_over_zonal`;
  * wb2_crps_bin_fold (n_slot = 4 NB) + wb2_event_fold on the rows (the simple
    path: no speed claim);
  * the torch expression: torch.fft.rfft of both, the four products, the
    member sum;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, LDS and
scratch (which must be 0) per instantiation (CPU side; needs hipcc)."""
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
from weatherbench2_amd import _lib, engine, spectral
from weatherbench2_amd import derived_variables as dv
from weatherbench2_amd import plan as plan_lib

SHAPES = {'det_1440': (1, 13, 721, 1440), 'ens50_240': (50, 13, 121, 240)}
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'cross_spectrum_bench.jsonl')


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_outer, n_row, n_col = SHAPES[name]
  n_bin = n_col // 2 + 1
  lat = np.linspace(-90, 90, n_row)
  circ = np.ascontiguousarray(dv.ZonalEnergySpectrum._circumference(lat),
                              dtype=np.float64)
  wrow = np.asarray(plan_lib.get_lat_weights(lat), np.float64)[None]
  slab = n_row * n_col
  n_rows = n_outer * n_row
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
  per_row = (n_member + 1) * n_col * 4 + 4 * n_bin * 8 + 8
  moved = per_row * n_rows
  n = max(args.pool, -(-600_000_000 // moved))
  pool = []
  for _ in range(n):
    truth = torch.randn((n_outer, n_row, n_col), device=dev, generator=gen) + 3
    ens = 0.8 * truth[None] + 0.6 * torch.randn(
        (n_member, n_outer, n_row, n_col), device=dev, generator=gen)
    pool.append((ens.contiguous(), truth))
  emit({'shape': name, 'members': n_member, 'outer': n_outer,
        'grid': [n_row, n_col], 'rows': n_rows, 'pool': n,
        'bytes_per_row': per_row,
        'geometry': engine.cross_spectrum_geometry(torch.float32, n_col,
                                                   n_member)})
  yardstick(name)
  member_stride = n_outer * slab
  # (checks the operands once, makes the plan and gives the reference rows)
  sums, cnt = engine.cross_spectrum_rows(pool[0][0], member_stride, n_member,
                                         None, pool[0][1], None, n_outer,
                                         n_row, n_col, circ)
  handle, _ = engine._SPECTRUM_PLANS.get(_lib.WB2_F32, n_col, 1)
  circ_dev = engine.upload_f64_table(circ, dev)
  outs = [(torch.empty_like(sums), torch.empty_like(cnt)) for _ in range(2)]

  def launch(i):
    ens, truth = pool[i]
    _lib.check(lib.wb2_cross_spectrum_rows(
        handle, _lib.WB2_F32, ens.data_ptr(), None, truth.data_ptr(), None,
        n_member, member_stride, n_outer, n_row, n_col, circ_dev.data_ptr(),
        outs[i % 2][0].data_ptr(), outs[i % 2][1].data_ptr(), stream),
               'wb2_cross_spectrum_rows')
  ours = report('cross_spectrum_rows', timed(launch, n, args.reps), moved,
                extra={'read_MB': round((n_member + 1) * n_col * 4 * n_rows /
                                        1e6, 1),
                       'written_MB': round((4 * n_bin * 8 + 8) * n_rows / 1e6,
                                           1),
                       'rows_over_zonal': None})

  # the M + 1 wb2_zonal_spectrum launches on the same rows (powers only)
  zplan, zbytes = engine._SPECTRUM_PLANS.get(_lib.WB2_F32, n_col, n_rows)
  work = torch.empty(max(zbytes, 256), dtype=torch.uint8, device=dev)
  zout = torch.empty((n_rows, n_bin), dtype=torch.float64, device=dev)

  def launch_zonal(i):
    ens, truth = pool[i]
    for x in [truth] + [ens[m] for m in range(n_member)]:
      _lib.check(lib.wb2_zonal_spectrum(
          zplan, x.data_ptr(), circ_dev.data_ptr(), n_row, 0, 1,
          zout.data_ptr(), work.data_ptr(), stream), 'wb2_zonal_spectrum')
  zonal = timed(launch_zonal, n, args.reps)
  report('zonal_spectrum_x_members_plus_1', zonal,
         (n_member + 1) * (n_col * 4 + n_bin * 8) * n_rows,
         extra={'launches': n_member + 1,
                'note': 'every launch overwrites one spectrum buffer; gives '
                        'the powers only'})
  lines[-2]['rows_over_zonal'] = round(ours / zonal[0], 2)
  print(json.dumps({'shape': name,
                    'rows_over_zonal': lines[-2]['rows_over_zonal']}),
        flush=True)

  holder = [None]

  def launch_fold(i):
    holder[0] = engine.cross_spectrum_fold(sums, cnt, wrow)
  report('cross_spectrum_fold', timed(launch_fold, 1, args.reps, warmup=2),
         sums.numel() * 8 + cnt.numel() * 4,
         extra={'note': 'rows fold + flag fold, the simple path, untuned, '
                        'Python launch layer included'})
  table, counts = (x.cpu().numpy() for x in holder[0])
  want = spectral.host_fold(sums.cpu().numpy(), cnt.cpu().numpy(), wrow)
  fold_same = bool(np.array_equal(table, want[0]) and
                   np.array_equal(counts, want[1]))

  if not args.no_torch:
    scale = torch.full((n_bin,), 2.0, dtype=torch.float64, device=dev)
    scale[0] = 1.0
    scale = scale[None] * circ_dev[:n_row, None]

    def torch_form(ens, truth):
      tt = torch.fft.rfft(truth, dim=-1, norm='forward')
      ff = torch.fft.rfft(ens, dim=-1, norm='forward')
      cross = ff * tt.conj()[None]
      return torch.stack([
          (ff.real ** 2 + ff.imag ** 2).double().sum(0) * scale,
          (tt.real ** 2 + tt.imag ** 2).double() * scale,
          cross.real.double().sum(0) * scale,
          cross.imag.double().sum(0) * scale], dim=2)
    got = torch_form(*pool[0])
    top = float(sums.abs().max())
    agree = bool(((got - sums).abs().max() / top) < 1e-5)
    del got

    def launch_torch(i):
      holder[0] = torch_form(*pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report('torch_rfft', tt, moved, extra={
        'expression': 'torch.fft.rfft of both, the four products, the member '
                      'sum',
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
    rep = resource_report('cross_spectrum.hip')
  except (OSError, subprocess.CalledProcessError) as e:
    print(json.dumps({'resource_report': f'not available: {e}'}))
    return
  spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
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
