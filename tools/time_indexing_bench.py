"""The slab scatter alone (csrc/slab_scatter.hip, K16) on the three shapes of
weatherbench2_amd/time_indexing.py, one process per shape, distinct inputs and
outputs per launch (no re-use between launches):

  expand    expand_climatology of 4 hours x 366 days x (13 x 240 x 121)
            float32 onto one six-hourly year (2017): one destination per source
  valid     index_on_valid_time of 730 inits (12 h) x 41 leads (6 h) x 64 x 32
            float64 -> float32, with holes
  ensemble  the sampled ensemble of 50 members x 61 leads x 32 inits of
            13 x 64 x 32 float32 from 31 years (1990-2020) of six-hourly truth

  python tools/time_indexing_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/time_indexing_bench.py --only valid

One JSON line per run, printed and appended to --out (default
profiles/time_indexing_bench.jsonl): ms per launch (a HIP event pair around
every launch, median and min), GB/s against the roofline of U * sizeof(Tin) +
N * sizeof(Tout) bytes per point for U distinct sources and N destinations,
and that as a share of 8 TB/s.  The tables come from the module itself (its
`materialize=False` results over a one-point grid).  In the same process:

  * `scatter`: the kernel fed the planner's CSR (every source read once);
  * `gather`: the same kernel fed one destination per source entry, so every
    destination reads its source again: N * (sizeof(Tin) + sizeof(Tout));
  * the torch expression a user would write today: `index_select`, plus
    `masked_fill_` where there are holes and `.to(float32)` where the dtype
    changes, with `torch_over_hip` and whether the bits agree;
  * the project's wind_speed kernel, a plain stream: what this box gives at
    that moment (one line before and after every shape).

The last lines are the resource report of the build: registers, scratch and
occupancy per instantiation; none may use scratch (CPU side; needs hipcc)."""
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
from weatherbench2_amd import _lib, engine
from weatherbench2_amd import time_indexing as ti
from weatherbench2_amd import xarray_lite as xl

SHAPES = ('expand', 'valid', 'ensemble')
HOUR = np.timedelta64(3600 * 10**9, 'ns')
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'time_indexing_bench.jsonl')


def _axis(start, step_hours, n):
  return np.datetime64(start, 'ns') + np.arange(n) * (step_hours * HOUR)


def _table(dataset_fn, name):
  """The module's destination-to-source table over a one-point grid."""
  return dataset_fn()[name].data.index.ravel()


def problem(name):
  """(n_in_slab, n_point, in dtype, out dtype, destination-to-source table)."""
  if name == 'expand':
    clim = xl.Dataset(
        {'x': xl.DataArray(np.zeros((4, 366, 1, 1), np.float32),
                           ('hour', 'dayofyear', 'latitude', 'longitude'))},
        {'hour': np.arange(0, 24, 6), 'dayofyear': 1 + np.arange(366)})
    table = _table(lambda: ti.expand_climatology(
        clim, time_start='2017-01-01', time_stop='2017-12-31T18',
        materialize=False), 'x')
    return 4 * 366, 13 * 240 * 121, torch.float32, torch.float32, table
  if name == 'valid':
    forecast = xl.Dataset(
        {'x': xl.DataArray(np.zeros((730, 41, 1, 1), np.float32),
                           ('time', ti.DELTA, 'latitude', 'longitude'))},
        {'time': _axis('2020-01-01', 12, 730),
         ti.DELTA: np.arange(41) * (6 * HOUR)})
    table = _table(lambda: ti.index_on_valid_time(forecast, materialize=False),
                   'x')
    return 730 * 41, 64 * 32, torch.float64, torch.float32, table
  times = np.arange(np.datetime64('1990-01-01', 'h'),
                    np.datetime64('2022-01-01', 'h'),
                    np.timedelta64(6, 'h')).astype('datetime64[ns]')
  truth = xl.Dataset(
      {'x': xl.DataArray(np.zeros((len(times), 1, 1), np.float32),
                         ('time', 'latitude', 'longitude'))}, {'time': times})
  table = _table(lambda: ti.probabilistic_climatological_forecasts(
      truth, initial_time_start='2021-06-01', initial_time_end='2021-06-16T12',
      initial_time_spacing='12h', forecast_duration='15 days',
      timedelta_spacing='6h', climatology_start_year=1990,
      climatology_end_year=2020, day_window_size=15, ensemble_size=50,
      materialize=False), 'x')
  assert table.size == 50 * 61 * 32
  return len(times), 13 * 64 * 32, torch.float32, torch.float32, table


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  n_in, n_point, in_dtype, out_dtype, table = problem(name)
  n_out = table.size
  distinct = np.unique(table[table >= 0]).size
  n_hole = int((table < 0).sum())
  in_size = torch.empty(0, dtype=in_dtype).element_size()
  out_size = torch.empty(0, dtype=out_dtype).element_size()
  roofline = n_point * (distinct * in_size + n_out * out_size)
  gather_bytes = n_point * ((n_out - n_hole) * in_size + n_out * out_size)
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  emit({'shape': name, 'n_in_slab': n_in, 'n_out_slab': n_out,
        'n_point': n_point, 'distinct_sources': distinct, 'holes': n_hole,
        'in': str(in_dtype), 'out': str(out_dtype),
        'geometry': engine.slab_scatter_geometry(in_dtype, out_dtype, True)})

  def report(kernel, n_bytes, ms, extra=None):
    med, best = ms
    gbps = n_bytes / med / 1e6
    line = {'shape': name, 'kernel': kernel, 'ms_median': round(med, 4),
            'ms_min': round(best, 4), 'MB': round(n_bytes / 1e6, 1),
            'GBps': round(gbps, 1), 'frac_of_8TBps': round(gbps / 8000.0, 4)}
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
    report('wind_speed_f32', 12 * n_ws, timed(launch, len(ws), args.reps),
           {'before': before})

  n = args.pool
  pool = [torch.randn((n_in, n_point), device=dev, generator=gen,
                      dtype=in_dtype) for _ in range(n)]
  outs = [torch.empty((n_out, n_point), device=dev, dtype=out_dtype)
          for _ in range(n)]
  yardstick(name)

  def tables(src, begin, dst):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
            for a in (src, begin, dst)]

  forms = {
      'scatter': ti.plan_scatter(table, n_in),
      'gather': engine.scatter_csr(table, (np.arange(n_out + 1),
                                           np.arange(n_out)), n_in, n_out)}
  ms = {}
  for form, (src, begin, dst) in forms.items():
    dev_tables = tables(src, begin, dst)

    def launch(i):
      _lib.check(lib.wb2_slab_scatter(
          engine.dtype_code(in_dtype), engine.dtype_code(out_dtype),
          pool[i].data_ptr(), dev_tables[0].data_ptr(),
          dev_tables[1].data_ptr(), dev_tables[2].data_ptr(), int(src.size),
          n_point, args.dests_per_group, outs[i].data_ptr(), stream),
                 'wb2_slab_scatter')
    ms[form] = report(
        f'slab_scatter_{form}', roofline, timed(launch, n, args.reps),
        {'entries': int(src.size), 'moved_MB': round(
            (roofline if form == 'scatter' else gather_bytes) / 1e6, 1),
         'dests_per_group': args.dests_per_group})
  kept = outs[0].clone()

  if not args.no_torch:
    index = torch.from_numpy(np.maximum(table, 0)).to(dev)
    hole = torch.from_numpy(table < 0).to(dev) if n_hole else None
    holder = [None]

    def torch_form(x):
      out = torch.index_select(x, 0, index)
      if hole is not None:
        out.masked_fill_(hole[:, None], float('nan'))
      return out if out_dtype == in_dtype else out.to(out_dtype)
    want = torch_form(pool[0])
    same = bool((want.view(torch.int32 if out_size == 4 else torch.int64)
                 == kept.view(torch.int32 if out_size == 4 else torch.int64)
                 ).all())
    del want

    def launch_torch(i):
      holder[0] = torch_form(pool[i])
    theirs = timed(launch_torch, n, max(5, args.reps // 2), warmup=2)
    report('torch_index_select', roofline, theirs,
           {'torch_over_scatter': round(theirs[0] / ms['scatter'], 2),
            'torch_over_gather': round(theirs[0] / ms['gather'], 2),
            'agree': same})
    holder[0] = None
  emit({'shape': name, 'gather_over_scatter':
        round(ms['gather'] / ms['scatter'], 3)})
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool', type=int, default=2)
  ap.add_argument('--dests-per-group', type=int, default=4)
  ap.add_argument('--only', default=None)
  ap.add_argument('--out', default=DEFAULT_OUT)
  ap.add_argument('--no-report', action='store_true')
  ap.add_argument('--no-torch', action='store_true')
  args = ap.parse_args()
  if args.only is not None:
    if args.only not in SHAPES:
      raise SystemExit(f'--only must be one of {list(SHAPES)}')
    run_shape(args.only, args)
    return
  # one fresh process per shape: nothing of one shape's pool, allocator state
  # or clocks carries into the next
  for name in SHAPES:
    cmd = [sys.executable, os.path.abspath(__file__), '--only', name,
           '--reps', str(args.reps), '--pool', str(args.pool),
           '--dests-per-group', str(args.dests_per_group), '--out', args.out]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    try:
      rep = resource_report('slab_scatter.hip')
      spills = {k: v for k, v in rep.items() if v.get('scratch', 0) != 0}
      with open(args.out, 'a') as f:
        for k, v in rep.items():
          line = json.dumps({'instantiation': k, **v})
          print(line)
          f.write(line + '\n')
      print(json.dumps({'instantiations': len(rep), 'with_scratch': spills,
                        'max_vgprs': max(v['vgprs'] for v in rep.values())}))
      assert not spills, spills
    except (OSError, subprocess.CalledProcessError) as e:
      print(json.dumps({'resource_report': f'not available: {e}'}))


if __name__ == '__main__':
  main()
