"""Interleaved A/B runs of plain `bench.py`: one JSON line per run.

  python tools/k1_ring_ab.py --runs 5 \\
      parent=PATH/libwb2hip.so  pr=  ring3=,WB2HIP_K1_RING=3  w2=build/variants/libwb2hip_w2.so

Every build is NAME=LIB[,ENV=VALUE...]: LIB is a libwb2hip.so (empty: the
tree's own library), selected through WB2HIP_LIB, the ENV pairs are set for
that build's runs only.  The builds run round-robin -- run 0 of every build,
then run 1 of every build, ... -- so a drift of the box over the session hits
all of them alike.  Each run is a child process of its own under a time limit;
the first run that fails, faults or runs out of time ends the session with its
exit status (nothing more is started on the device).

Line: {"build", "run", "value", "ms_per_step", "lib", "env"}; a summary line
per build (min, median, max of `value`) follows the runs.  Extra arguments
after `--` go to bench.py (e.g. `-- --steps 200 --warmup 20`, its defaults).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_build(spec):
  name, _, rest = spec.partition('=')
  parts = rest.split(',') if rest else ['']
  env = dict(p.split('=', 1) for p in parts[1:] if p)
  lib = os.path.abspath(parts[0]) if parts[0] else ''
  if lib and not os.path.exists(lib):
    raise SystemExit(f'{name}: no library at {lib}')
  return name, lib, env


def last_json_line(text):
  for line in reversed(text.splitlines()):
    line = line.strip()
    if line.startswith('{'):
      return json.loads(line)
  raise ValueError('no JSON line in the output of bench.py')


def main():
  argv = sys.argv[1:]
  bench_args = []
  if '--' in argv:
    i = argv.index('--')
    argv, bench_args = argv[:i], argv[i + 1:]
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--timeout', type=float, default=240.0,
                  help='seconds per bench.py run')
  ap.add_argument('builds', nargs='+', help='NAME=LIB[,ENV=VALUE...]')
  args = ap.parse_args(argv)
  builds = [parse_build(b) for b in args.builds]
  values = {name: [] for name, _, _ in builds}
  for run in range(args.runs):
    for name, lib, env in builds:
      child_env = dict(os.environ, **env)
      child_env.pop('WB2HIP_LIB', None)
      if lib:
        child_env['WB2HIP_LIB'] = lib
      try:
        done = subprocess.run(
            [sys.executable, os.path.join(ROOT, 'bench.py')] + bench_args,
            cwd=ROOT, env=child_env, stdout=subprocess.PIPE,
            stderr=subprocess.PIPE, text=True, timeout=args.timeout)
      except subprocess.TimeoutExpired:
        print(json.dumps({'build': name, 'run': run, 'error': 'timeout'}),
              flush=True)
        return 124
      if done.returncode != 0:
        print(json.dumps({'build': name, 'run': run,
                          'error': f'exit status {done.returncode}',
                          'stderr': done.stderr[-2000:]}), flush=True)
        return done.returncode if done.returncode > 0 else 1
      out = last_json_line(done.stdout)
      values[name].append(out['value'])
      print(json.dumps({'build': name, 'run': run, 'value': out['value'],
                        'ms_per_step': out.get('ms_per_step'),
                        'lib': lib or 'tree', 'env': env}), flush=True)
  for name, vals in values.items():
    print(json.dumps({'build': name, 'runs': len(vals), 'min': min(vals),
                      'median': statistics.median(vals), 'max': max(vals)}),
          flush=True)
  return 0


if __name__ == '__main__':
  sys.exit(main())
