"""The pooling kernel (csrc/pool.hip, K22), one process per shape, 'mean' and
'max':

  ens50_240   50 members x 13 levels of 121 x 240 float32, windows 3, 5, 9, 17
  det_1440    13 levels of 721 x 1440 float32, windows 5, 17, 65

  python tools/pool_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/pool_bench.py \
      --only ens50_240

One JSON line per run, printed and appended to --out (default
profiles/pool_bench.jsonl): ms per call of wb2_pool_fields (a HIP event pair
around every call -- W windows are one launch up to four, two beyond --, median
and min of --reps >= 10 calls over alternating inputs and outputs, enough of
them to exceed the 256 MiB Infinity Cache), GB/s against the (1 + W) * sizeof
B/element it has to move (one read, W writes), and that as a share of 8 TB/s.
In the same process, on the same operands:

  * the torch expression a user had before: circular pad of the longitudes,
    avg_pool2d (zero rows beyond the poles, divisor 1) over the pole divisor
    N_i, or max_pool2d -- timed in float32 as a user would run it
    (`torch_over_hip`); and, once, in float64 against the kernel's output
    within the bound of tests/pooling_np.py, (n + rows_i + 2) u * mean|x| +
    half an ulp of the output (`agree`; 'max': equal);
  * `PooledCRPS(windows).compute_chunk` end to end (wall clock, synchronised)
    beside W calls of the plain `ThresholdWeightedCRPS` at -inf on torch-pooled
    input (`pooled_crps_end_to_end`);
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch
(expected 0) and occupancy per instantiation (CPU side; needs hipcc); the LDS
is dynamic: lds_bytes of the geometry line."""
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
import torch.nn.functional as F

from tools.derived_bench import timed
from tools.quantile_bench import resource_report
from weatherbench2_amd import _lib, engine, pooling, threshold_weighted
from weatherbench2_amd import xarray_lite as xl
from weatherbench2_amd.neighborhood import ConstantThreshold

# name: (members or None, levels, n_row, n_col, windows)
SHAPES = {'ens50_240': (50, 13, 121, 240, (3, 5, 9, 17)),
          'det_1440': (None, 13, 721, 1440, (5, 17, 65))}
U = 2.0 ** -53
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'pool_bench.jsonl')


def torch_pool(x, n, kind):
  """The torch expression: [fields, n_row, n_col] -> the same shape."""
  h = n // 2
  n_row = x.shape[-2]
  xp = F.pad(x[None], (h, h, 0, 0), mode='circular')
  if kind == 'max':
    return F.max_pool2d(xp, (n, n), stride=1, padding=(h, 0))[0]
  total = F.avg_pool2d(xp, (n, n), stride=1, padding=(h, 0),
                       divisor_override=1)[0]
  rows = torch.arange(n_row, device=x.device)
  count = n * (torch.clamp(rows + h, max=n_row - 1) -
               torch.clamp(rows - h, min=0) + 1)
  return total / count.to(x.dtype)[:, None]


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_member, n_level, n_row, n_col, windows = SHAPES[name]
  n_field = (n_member or 1) * n_level
  n_elem = n_field * n_row * n_col
  n_win = len(windows)
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

  # alternating inputs and outputs, together larger than the Infinity Cache
  moved = (1 + n_win) * 4 * n_elem
  n = max(args.pool, -(-600_000_000 // moved))
  pool = [torch.randn((n_field, n_row, n_col), device=dev, generator=gen)
          for _ in range(n)]
  outs = [torch.empty((n_win, n_field, n_row, n_col), device=dev)
          for _ in range(n)]
  emit({'shape': name, 'fields': n_field, 'grid': [n_row, n_col],
        'windows': list(windows), 'pool': n,
        'geometry': engine.pool_geometry(torch.float32, n_col, windows)})
  yardstick(name)
  win = (ctypes.c_int32 * n_win)(*windows)

  for kind in ('mean', 'max'):
    code = engine.POOL_KINDS[kind]

    def launch(i):
      _lib.check(lib.wb2_pool_fields(
          _lib.WB2_F32, pool[i].data_ptr(), None, 1, 0, n_field, n_row, n_col,
          win, n_win, code, outs[i].data_ptr(), stream), 'wb2_pool_fields')
    ours = report(f'pool_fields_{kind}', timed(launch, n, args.reps), moved,
                  extra={'bytes_per_element': (1 + n_win) * 4,
                         'moved_MB': round(moved / 1e6, 1)})
    if args.no_torch:
      continue
    # agreement, once, on the first levels' worth of fields (float64 costs
    # twice the memory)
    some = min(n_field, 13)
    launch(0)
    agree = True
    x64 = pool[0][:some].double()
    for w, nw in enumerate(windows):
      got = outs[0][w, :some]
      want = torch_pool(x64, nw, kind)
      if kind == 'max':
        agree = agree and bool(torch.equal(got.double(), want))
        continue
      h = nw // 2
      rows = torch.arange(n_row, device=dev)
      n_rows = (torch.clamp(rows + h, max=n_row - 1) -
                torch.clamp(rows - h, min=0) + 1).double()[:, None]
      bound = ((nw + n_rows + 2) * U * torch_pool(x64.abs(), nw, kind) +
               0.5 * torch.from_numpy(np.spacing(np.abs(
                   got.cpu().numpy())).astype(np.float64)).to(dev))
      # (the torch sum is not exactly rounded: its own n^2 u is far below the
      # half ulp of a float32 output)
      agree = agree and bool(((got.double() - want).abs() <= bound).all())
    del x64
    holder = [None]

    def launch_torch(i):
      holder[0] = [torch_pool(pool[i], nw, kind) for nw in windows]
    tt = timed(launch_torch, n, max(10, args.reps // 2), warmup=2)
    report(f'torch_{kind}', tt, moved, extra={
        'expression': 'per window: circular pad, ' + (
            'avg_pool2d (divisor 1) / the pole divisor' if kind == 'mean'
            else 'max_pool2d'),
        'torch_over_hip': round(tt[0] / ours, 2), 'agree': agree})
    holder[0] = None

  # end to end: the wrapper metric beside what a user had before
  if not args.no_torch:
    lat = np.linspace(-90, 90, n_row)
    lon = np.linspace(0, 360, n_col, endpoint=False)
    coords = {'level': np.arange(n_level), 'latitude': lat, 'longitude': lon}
    dims = ('level', 'latitude', 'longitude')
    fdims = dims
    fdata = pool[0]
    if n_member:
      coords['realization'] = np.arange(n_member)
      fdims = ('realization',) + dims
      fdata = fdata.view(n_member, n_level, n_row, n_col)
    truth = torch.randn((n_level, n_row, n_col), device=dev, generator=gen)
    forecast = xl.Dataset({'x': xl.DataArray(fdata, fdims)}, coords)
    tru = xl.Dataset({'x': xl.DataArray(truth, dims)},
                     {k: v for k, v in coords.items() if k != 'realization'})
    plain = threshold_weighted.ThresholdWeightedCRPS(
        thresholds=[ConstantThreshold(-float('inf'))])
    for kind in ('mean', 'max'):
      metric = pooling.PooledCRPS(windows, kind)

      def ours_fn():
        return metric.compute_chunk(forecast, tru)

      def before_fn():
        out = []
        for nw in windows:
          pf = torch_pool(pool[0], nw, kind).view(fdata.shape)
          pt = torch_pool(truth, nw, kind)
          out.append(plain.compute_chunk(
              xl.Dataset({'x': xl.DataArray(pf, fdims)}, coords),
              xl.Dataset({'x': xl.DataArray(pt, dims)}, tru.coords)))
        return out

      def wall(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(reps):
          t0 = time.perf_counter()
          fn()
          torch.cuda.synchronize()
          best.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(best))
      a, b = wall(ours_fn), wall(before_fn)
      emit({'shape': name, 'kernel': f'pooled_crps_end_to_end_{kind}',
            'ms_pooled_crps': round(a, 3),
            'ms_torch_pool_and_W_plain_calls': round(b, 3),
            'before_over_pooled': round(b / a, 2),
            'note': 'wall clock with the Python layers, synchronised'})
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def report_resources(out):
  try:
    rep = resource_report('pool.hip')
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
