"""The official-chunk leg of tools/official_chunk.py with the documented
`--derived_variables=wind_speed,10m_wind_speed`: the chunks carry u and v only
and the two wind speeds are derived on the fly.

  python tools/derived_chunk.py [--chunks 64] [--pool 8] [--reps 5]

(a) `derived_variables.WindSpeed`: computed once per chunk up front by
    `evaluate_chunks`, chunk programs and windows stay on;
(b) an equivalent duck-typed torch WindSpeed: a foreign object, so the config
    takes the generic path chunk by chunk (what every config with derived
    variables took before the materialising classes existed).
Both run in the same call, alternating, chunk by chunk (`batch_chunks=1`) and
in the default window.  One JSON line: ms per chunk (median, min, max over the
repetitions) of each, and the ratios b / a."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
  if p not in sys.path:
    sys.path.insert(0, p)

PAIRS = {'wind_speed': ('u_component_of_wind', 'v_component_of_wind'),
         '10m_wind_speed': ('10m_u_component_of_wind',
                            '10m_v_component_of_wind')}


class TorchWindSpeed:
  """The duck-typed protocol, in torch: what a user could write before."""

  def __init__(self, u_name, v_name):
    self.u_name, self.v_name = u_name, v_name

  @property
  def base_variables(self):
    return [self.u_name, self.v_name]

  def compute(self, dataset):
    import torch
    from weatherbench2_amd import xarray_lite as xl
    u, v = dataset[self.u_name], dataset[self.v_name]
    return xl.DataArray(torch.sqrt(u.data * u.data + v.data * v.data), u.dims,
                        u.coords)


def without_speeds(chunks):
  from weatherbench2_amd import xarray_lite as xl
  out = []
  for f, t in chunks:
    out.append(tuple(xl.Dataset({k: v for k, v in ds.data_vars.items()
                                 if k not in PAIRS}, ds.coords)
                     for ds in (f, t)))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chunks', type=int, default=64)
  ap.add_argument('--pool', type=int, default=8)
  ap.add_argument('--reps', type=int, default=5)
  args = ap.parse_args()
  import torch
  import official_chunk as leg
  from weatherbench2_amd import derived_variables as dv
  from weatherbench2_amd import engine, evaluation
  dev = engine.require_gpu()
  chunks, cfg = leg.build(dev, args.chunks, args.pool, seeps=False)
  ours = dataclasses.replace(cfg, derived_variables={
      k: dv.WindSpeed(u_name=u, v_name=v) for k, (u, v) in PAIRS.items()})
  foreign = dataclasses.replace(cfg, derived_variables={
      k: TorchWindSpeed(u, v) for k, (u, v) in PAIRS.items()})

  def once(config, batch):
    fresh = without_speeds(chunks)  # (the generic path assigns in place)
    kwargs = {} if batch is None else {'batch_chunks': batch}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluation.evaluate_chunks(fresh, config, False, prefetch=0,
                                     **kwargs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(fresh), res

  out = {'chunks': args.chunks, 'pool': args.pool, 'reps': args.reps}
  for label, batch in (('chunk_by_chunk', 1), ('default_window', None)):
    times = {'hip_classes': [], 'torch_duck_typed': []}
    results = {}
    for rep in range(args.reps + 1):  # (the first round warms both up)
      for name, config in (('hip_classes', ours),
                           ('torch_duck_typed', foreign)):
        ms, res = once(config, batch)
        results[name] = res
        if rep:
          times[name].append(ms)
    a, b = results['hip_classes'], results['torch_duck_typed']
    same = all(np.array_equal(a[k].values, b[k].values, equal_nan=True)
               for k in a.data_vars)
    row = {k: {'ms_per_chunk_median': round(float(np.median(v)), 4),
               'min': round(min(v), 4), 'max': round(max(v), 4)}
           for k, v in times.items()}
    row['torch_over_hip'] = round(
        float(np.median(times['torch_duck_typed'])
              / np.median(times['hip_classes'])), 3)
    row['same_values'] = bool(same)
    out[label] = row
  print(json.dumps(out))


if __name__ == '__main__':
  main()
