"""The box gather alone (csrc/box_gather.hip, K17) on the shapes of
weatherbench2_amd/slicing.py, one process per shape, distinct inputs and
outputs per launch (no re-use between launches):

  flip        16 chunks x 13 levels of 721 x 1440 float32, the latitude rows
              reversed (make_dims_increasing on an ERA5-style axis)
  box         the same input, latitude -33.33..33.33, longitude 0..180
  lon_step4   the same input, longitude_step=4
  example     the same input, the script's own example: the `sel` box on
              latitude and `isel` longitude_start=0,longitude_stop=180,
              longitude_step=40
  lonlat_flip 16 x 13 of 1440 x 721 (the Zarr stores' layout), the latitude
              reversed: the innermost dim, rows of 721 elements
  time_range  1 464 times x 13 levels of 32 x 64 float32, a time range: whole
              slabs, the K16 path of `slice_dataset`, for comparison

  python tools/slice_bench.py [--reps R] [--only NAME] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/slice_bench.py --only flip

One JSON line per run, printed and appended to --out (default
profiles/slice_bench.jsonl): ms per launch (a HIP event pair around every
launch, median and min of --reps), GB/s against (the 128-byte requests the
kept elements touch + the bytes written) and that as a share of 8 TB/s.  The
position vectors come from the module itself (`slicing.compose_positions` on
the real coordinates).  In the same process:

  * the torch expression a user would write today (`torch.flip`, chained
    `index_select`), with `torch_over_hip` and whether the bits agree;
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
from weatherbench2_amd import _lib, engine, slicing
from weatherbench2_amd import xarray_lite as xl

SHAPES = ('flip', 'box', 'lon_step4', 'example', 'lonlat_flip', 'time_range')
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'profiles', 'slice_bench.jsonl')
N_SLAB = 16 * 13
LAT_UP = np.linspace(-90, 90, 721)
LON = np.linspace(0, 360, 1440, endpoint=False)

OPTIONS = {
    'flip': dict(make_dims_increasing='latitude'),
    'box': dict(sel='latitude_start=-33.33,latitude_stop=33.33,'
                    'longitude_start=0,longitude_stop=180'),
    'lon_step4': dict(isel='longitude_step=4'),
    'example': dict(sel='latitude_start=-33.33,latitude_stop=33.33',
                    isel='longitude_start=0,longitude_stop=180,'
                         'longitude_step=40'),
    'lonlat_flip': dict(make_dims_increasing='latitude'),
    'time_range': dict(isel='time_start=124,time_stop=1340'),
}


def problem(name):
  """(input shape [n_slab, n_row, n_col], positions per axis or None)."""
  if name == 'time_range':
    ds = xl.Dataset({'x': xl.DataArray(np.zeros((1464, 1, 1, 1), np.float32), (
        'time', 'level', 'latitude', 'longitude'))}, {})
    pos = slicing.compose_positions(ds, **OPTIONS[name])
    slabs = (pos['time'][:, None] * 13 + np.arange(13)[None, :]).ravel()
    return (1464 * 13, 32, 64), (slabs, None, None)
  lonlat = name == 'lonlat_flip'
  flipped = name in ('flip', 'lonlat_flip')
  dims = ('longitude', 'latitude') if lonlat else ('latitude', 'longitude')
  coords = {'latitude': LAT_UP[::-1].copy() if flipped else LAT_UP,
            'longitude': LON}
  ds = xl.Dataset({'x': xl.DataArray(
      np.zeros((coords[dims[0]].size, coords[dims[1]].size), np.int8), dims)},
                  coords)
  pos = slicing.compose_positions(ds, **OPTIONS[name])
  return ((N_SLAB, coords[dims[0]].size, coords[dims[1]].size),
          (None, pos.get(dims[0]), pos.get(dims[1])))


def touched_bytes(shape, rows, cols, item) -> int:
  """The bytes of the 128-byte requests that hold a kept element (a slab is a
  whole number of requests for every shape here)."""
  n_slab, n_row, n_col = shape
  assert n_row * n_col * item % 128 == 0
  rows = np.arange(n_row) if rows is None else rows
  cols = np.arange(n_col) if cols is None else cols
  at = (rows[:, None] * n_col + cols[None, :]) * item // 128
  return int(np.unique(at).size) * 128 * n_slab


def run_shape(name, args):
  dev = engine.require_gpu()
  lib = _lib.load()
  stream = engine.current_stream_ptr(dev)
  gen = torch.Generator(device=dev).manual_seed(0)
  shape, (slabs, rows, cols) = problem(name)
  n_slab, n_row, n_col = shape
  n_out_slab = n_slab if slabs is None else slabs.size
  n_row_out = n_row if rows is None else rows.size
  n_col_out = n_col if cols is None else cols.size
  out_shape = (n_out_slab, n_row_out, n_col_out)
  written = int(np.prod(out_shape)) * 4
  read = touched_bytes((n_out_slab, n_row, n_col), rows, cols, 4)
  kept = written
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  def report(kernel, ms, extra=None):
    med, best = ms
    gbps = (read + written) / med / 1e6
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

  n = args.pool
  pool = [torch.randn(shape, device=dev, generator=gen) for _ in range(n)]
  outs = [torch.empty(out_shape, device=dev) for _ in range(n)]
  affine = None if cols is None else slicing._affine(cols)  # pylint: disable=protected-access
  col_arg = (0, 1, n_col) if cols is None else (affine or cols)
  whole_slabs = rows is None and cols is None
  emit({'shape': name, 'options': OPTIONS[name], 'in': list(shape),
        'out': list(out_shape), 'kept_MB': round(kept / 1e6, 1),
        'requests_touched_MB': round(read / 1e6, 1),
        'written_MB': round(written / 1e6, 1),
        'path': 'slab_scatter' if whole_slabs else 'box_gather',
        'form': None if whole_slabs else engine.box_gather_form(
            pool[0], outs[0], n_col, col_arg),
        'geometry': None if whole_slabs else engine.box_gather_geometry(
            torch.float32, engine.box_gather_form(pool[0], outs[0], n_col,
                                                  col_arg), n_col_out)})
  yardstick(name)

  # the tables go up once: a launch is the library call alone, so that an event
  # pair holds no host work
  def table(a, dtype):
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a, dtype=dtype)).to(dev)
  if whole_slabs:
    src = table(slabs, np.int64)
    begin = table(np.arange(n_out_slab + 1), np.int64)
    dst = table(np.arange(n_out_slab), np.int64)

    def launch(i):
      _lib.check(lib.wb2_slab_scatter(
          _lib.WB2_F32, _lib.WB2_F32, pool[i].data_ptr(), src.data_ptr(),
          begin.data_ptr(), dst.data_ptr(), n_out_slab, n_row * n_col, 4,
          outs[i].data_ptr(), stream), 'wb2_slab_scatter')
  else:
    engine.box_gather(pool[0], n_row, n_col, src_slab=slabs, rows=rows,
                      cols=col_arg, out=outs[0])  # (checks the tables once)
    slab_dev, row_dev = table(slabs, np.int64), table(rows, np.int32)
    col_dev = None if isinstance(col_arg, tuple) else table(cols, np.int32)
    col0, step, _ = col_arg if isinstance(col_arg, tuple) else (0, 1, 0)

    def launch(i):
      _lib.check(lib.wb2_box_gather(
          4, pool[i].data_ptr(), _lib.ptr(slab_dev), n_out_slab, n_row, n_col,
          _lib.ptr(row_dev), n_row_out, col0, step, _lib.ptr(col_dev),
          n_col_out, outs[i].data_ptr(), stream), 'wb2_box_gather')
  ours = report('slab_scatter' if whole_slabs else 'box_gather',
                timed(launch, n, args.reps))
  result = outs[0].clone()

  if not args.no_torch:
    index = [None if p is None else torch.from_numpy(p).to(dev)
             for p in (slabs, rows, cols)]
    holder = [None]

    def torch_form(x):
      if name == 'flip':
        return torch.flip(x, [1])
      if name == 'lonlat_flip':
        return torch.flip(x, [2])
      for axis, idx in enumerate(index):
        if idx is not None:
          x = torch.index_select(x, axis, idx)
      return x
    want = torch_form(pool[0])
    same = bool((want.view(torch.int32) == result.view(torch.int32)).all())
    del want

    def launch_torch(i):
      holder[0] = torch_form(pool[i])
    theirs = timed(launch_torch, n, args.reps, warmup=2)
    report('torch', theirs, {
        'expression': 'torch.flip' if 'flip' in name else 'index_select chain',
        'torch_over_hip': round(theirs[0] / ours, 2), 'agree': same})
    holder[0] = None
  yardstick('end')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    for line in lines:
      f.write(json.dumps(line) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--pool', type=int, default=2)
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
           '--reps', str(args.reps), '--pool', str(args.pool), '--out',
           args.out]
    if args.no_torch:
      cmd.append('--no-torch')
    done = subprocess.run(cmd)
    if done.returncode != 0:
      raise SystemExit(f'{name}: exit status {done.returncode}')
  if not args.no_report:
    try:
      rep = resource_report('box_gather.hip')
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
