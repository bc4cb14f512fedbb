"""The bootstrap-mean kernel (csrc/resample_means.hip, K23), one process per
shape:

  scalar_f32         T = 730, B = 1000, C = 8320 float32 (40 leads x 16 regions
                     x 13 levels of one scalar score)
  crps_level_f64     T = 730, B = 1000, C = 51 * 3 * 40 * 16 = 97920 float64
                     (one level of a CRPSTable, 50 members)
  scalar_f32_skipna  the first shape with skipna (and one NaN in 1000 values)

  python tools/bootstrap_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/bootstrap_bench.py \
      --only scalar_f32

One JSON line per run, printed and appended to --out (default
profiles/bootstrap_bench.jsonl): ms per call of wb2_resampled_means (a HIP
event pair around every call, median and min of --reps >= 10 calls over
distinct inputs and outputs), its used (b, t, c) terms per second -- a term is
one (count, value) pair with a nonzero count --, and, in the same process:

  * the float64 vector rate of the device from tools/f64_rate.hip (a loop of
    independent v_fma_f64, and of v_mul_f64 + v_add_f64 pairs, no memory), and
    the kernel's terms per second as a share of it: of the pair rate for
    float64 input, of the fma rate for float32 input (`share_of_f64_rate`);
  * the bytes the kernel requests, T * C * sizeof once per replicate group,
    against T * C * sizeof (`read_amplification`; requested, not HBM traffic:
    the groups of a tile run together and share its cache lines);
  * the torch expression `counts.double() @ x` / T (rocBLAS; a float32 x is
    widened first, inside the timing; with NaNs: nan_to_num and a second
    product with the validity mask), and whether it agrees with the kernel
    within (T + 2) u sum n |x| / W;
  * for the first shape, `bootstrap()` end to end with score_fn = sqrt (wall
    clock, synchronised, device-backed input);
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch
(expected 0) and occupancy per instantiation (CPU side; needs hipcc)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.derived_bench import timed
from tools.quantile_bench import resource_report
from weatherbench2_amd import _lib, bootstrap, build, engine
from weatherbench2_amd import xarray_lite as xl

ROOT = build.ROOT
# name: (n_time, n_replicate, n_cell, dtype, skipna)
SHAPES = {'scalar_f32': (730, 1000, 8320, torch.float32, False),
          'crps_level_f64': (730, 1000, 51 * 3 * 40 * 16, torch.float64, False),
          'scalar_f32_skipna': (730, 1000, 8320, torch.float32, True)}
U = 2.0 ** -53
DEFAULT_OUT = os.path.join(ROOT, 'profiles', 'bootstrap_bench.jsonl')
RATE_LIB = os.path.join(ROOT, 'build', 'libf64_rate.so')


def build_rate_lib():
  """build/libf64_rate.so from tools/f64_rate.hip (kept when up to date)."""
  src = os.path.join(ROOT, 'tools', 'f64_rate.hip')
  if os.path.exists(RATE_LIB) and (os.path.getmtime(RATE_LIB)
                                   >= os.path.getmtime(src)):
    return RATE_LIB
  os.makedirs(os.path.dirname(RATE_LIB), exist_ok=True)
  subprocess.run([build._hipcc(), '--offload-arch=gfx950', '-O3', '-shared',
                  '-fPIC', '-Wno-unused-result', '-Wno-unused-value', '-o',
                  RATE_LIB, src], check=True)
  return RATE_LIB


def f64_rates() -> dict:
  """{'fma': ops/s, 'mul_add': pairs/s}: the best over 1-4 waves per SIMD."""
  lib = ctypes.CDLL(build_rate_lib())
  lib.f64_rate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_double)]
  out = {}
  for name, form in (('fma', 0), ('mul_add', 1)):
    best = 0.0
    for threads in (256, 512, 1024):
      value = ctypes.c_double()
      status = lib.f64_rate(form, threads, 4096, ctypes.byref(value))
      if status != 0:
        raise RuntimeError(f'f64_rate failed ({status})')
      best = max(best, value.value)
    out[name] = best
  return out


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_time, n_rep, n_cell, dtype, skipna = SHAPES[name]
  esz = 4 if dtype == torch.float32 else 8
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

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

  geo = engine.resampled_means_geometry(dtype, True)
  n_group = -(-n_rep // geo['replicates_per_group'])
  counts = bootstrap.block_plan(n_time, n_rep, args.block_length, seed=0)
  wgt, tot = (a.to(dev) for a in engine.resampled_means_tables(
      engine.checked_counts(counts, n_time), dtype))
  used = int((counts != 0).sum()) * n_cell
  data_bytes = n_time * n_cell * esz
  # distinct inputs and outputs per launch, together larger than the cache
  n = min(20, max(2, -(-600_000_000 // data_bytes)))
  pool = [torch.rand((n_time, n_cell), device=dev, dtype=dtype, generator=gen)
          + 0.5 for _ in range(n)]
  if skipna:
    for x in pool:
      x[torch.rand(x.shape, device=dev, generator=gen) < 1e-3] = float('nan')
  outs = [torch.empty((n_rep, n_cell), dtype=torch.float64, device=dev)
          for _ in range(n)]
  rates = f64_rates()
  emit({'shape': name, 'n_time': n_time, 'n_replicate': n_rep,
        'n_cell': n_cell, 'dtype': str(dtype), 'skipna': skipna,
        'block_length': args.block_length, 'pool': n, 'geometry': geo,
        'used_terms': used, 'used_share': round(used / (
            n_rep * n_time * n_cell), 4),
        'f64_fma_per_s': rates['fma'], 'f64_mul_add_pairs_per_s':
            rates['mul_add']})
  yardstick(name)
  code = engine.dtype_code(dtype)

  def launch(i):
    _lib.check(lib.wb2_resampled_means(
        code, int(skipna), pool[i].data_ptr(), None, 1, n_time, n_cell,
        wgt.data_ptr(), tot.data_ptr(), n_rep, outs[i].data_ptr(), stream),
               'wb2_resampled_means')
  med, best = timed(launch, n, args.reps)
  rate = rates['fma'] if dtype == torch.float32 else rates['mul_add']
  emit({'shape': name, 'kernel': 'resampled_means', 'ms_median': round(med, 4),
        'ms_min': round(best, 4),
        'used_terms_per_s': round(used / med * 1e3, 1),
        'share_of_f64_rate': round(used / med * 1e3 / rate, 4),
        'rate_used': 'fma' if dtype == torch.float32 else 'mul_add',
        'requested_MB': round(n_group * data_bytes / 1e6, 1),
        'data_MB': round(data_bytes / 1e6, 1), 'read_amplification': n_group,
        'requested_GBps': round(n_group * data_bytes / med / 1e6, 1)})
  ours = med

  if not args.no_torch:
    cd = torch.from_numpy(counts.astype(np.float64)).to(dev)
    total = cd.sum(dim=1, keepdim=True)
    holder = [None]

    def expression(x):
      x64 = x.double()
      if not skipna:
        return (cd @ x64) / total
      ok = ~torch.isnan(x64)
      return (cd @ torch.nan_to_num(x64)) / (cd @ ok.double())

    def launch_torch(i):
      holder[0] = expression(pool[i])
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    launch(0)
    want = expression(pool[0])
    x64 = torch.nan_to_num(pool[0].double()).abs()
    bound = (n_time + 2) * U * (cd @ x64) / total * (2.0 if skipna else 1.0)
    agree = bool(((outs[0] - want).abs() <= bound).all())
    holder[0] = None
    emit({'shape': name, 'kernel': 'torch_matmul', 'ms_median':
          round(tt[0], 4), 'ms_min': round(tt[1], 4), 'expression':
          '(counts.double() @ x.double()) / W' if not skipna else
          '(c @ nan_to_num(x)) / (c @ ~isnan(x)), c = counts.double()',
          'torch_over_hip': round(tt[0] / ours, 3), 'agree': agree})
    del want, x64, bound

  if name == 'scalar_f32':
    da = xl.DataArray(pool[0], ('time', 'cell'), {}, 'score')
    walls = []
    for _ in range(3):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      bootstrap.bootstrap(da, lambda t: t.sqrt(), n_replicate=n_rep,
                          block_length=args.block_length, seed=0)
      torch.cuda.synchronize()
      walls.append(time.perf_counter() - t0)
    emit({'shape': name, 'kernel': 'bootstrap_end_to_end_sqrt',
          's_wall_median': round(float(np.median(walls)), 3),
          's_wall_first': round(walls[0], 3),
          'note': 'plan, upload of the counts, K23, download of B x C '
                  'float64, sqrt and the quantiles on the host; the NumPy '
                  'rank-1 form of the means alone takes 26 s on the CPU'})
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def report_resources(out):
  try:
    rep = resource_report('resample_means.hip')
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
  ap.add_argument('--block-length', type=int, default=1)
  ap.add_argument('--only', default=None)
  ap.add_argument('--out', default=DEFAULT_OUT)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--report-only', action='store_true')
  ap.add_argument('--build-only', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  if args.reps < 10:
    raise SystemExit('--reps must be at least 10')
  if args.build_only:
    print(build_rate_lib())
    return
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
           '--reps', str(args.reps), '--block-length', str(args.block_length),
           '--out', args.out]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    report_resources(args.out)


if __name__ == '__main__':
  main()
