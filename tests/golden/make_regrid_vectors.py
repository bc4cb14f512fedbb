"""Writes tests/golden/reference_regrid_v1.<case>.npz: outputs of the
REFERENCE's own, unmodified weatherbench2/regridding.py for its three
regridders on the seeded cases of tests/regrid_cases.py, one shard per case (a
committed file stays below 1 MiB; tests/regrid_cases.load_golden reads them
back as one dict).

As for the other reference_*_v1 fixtures, "the reference" means the
reference's code on the mini-xarray of oracle/refshim/ (see
make_derived_vectors.py, whose set-up this generator imports).  jax is absent
here as well; this generator installs a NumPy stand-in for it into sys.modules
at run time, in its own process: `jit` returns the function, `vmap` loops and
stacks, `jax.numpy` is numpy with an `einsum` that drops `precision=`, and
`jax.Array` is np.ndarray.  So the reference runs in float64 (jax's default
would demote everything to float32: that demotion is not what the fixtures
pin).  `BallTree` is scikit-learn's own.  Nothing under oracle/ changes.

Per case the file holds
  <case>/source/*, <case>/target/*   the grids (the keyword arguments of Grid)
  <case>/field                       the float64 input, (..., lon, lat)
  <case>/<label>/ref                 regrid_array of the reference, label in
                                     nearest, bilinear, conservative
  <case>/lon_weights, lat_weights    the reference's dense conservative weights
  <case>/nearest/indices, /ties      its index table; where the nearest and the
                                     second-nearest source node are closer
                                     than 1e-9 rad (a tie: BallTree's pick is
                                     arbitrary there)
and <case>/seed; known/<name>/{ref, expected}: the inputs of the reference's
known-answer tests (regridding_test.py:313-330, 495-591, 593-618) through the
reference, next to the values written there; structure/structure: class names,
Grid's fields, enum members.

What the generator asserts: ties of a nearest case lie on the pole rows of the
target and on the target rows / columns that are exactly midway between two
source nodes (tests/regrid_cases.tie_rows_and_columns), and at most a third
of the nodes tie; off ties BallTree equals the full brute-force table; in the
bilinear NaN case no finite source node that a target node coincides with has
a NaN neighbour along that axis (np.interp takes the node's value there: what
jax's interp does is not pinned).

Only runs where the reference is at hand:
    python tests/golden/make_regrid_vectors.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_derived_vectors as base  # noqa: E402  (paths, stand-in xarray)


def _install_jax_stand_in():
  jax = types.ModuleType('jax')
  jnp = types.ModuleType('jax.numpy')
  jnp.__dict__.update({k: v for k, v in np.__dict__.items()
                       if not k.startswith('__')})
  jnp.einsum = lambda *a, precision=None, **k: np.einsum(*a, **k)

  def vmap(fn, in_axes=0, out_axes=0):
    def mapped(*args):
      axes = in_axes if isinstance(in_axes, tuple) else (in_axes,) * len(args)
      n = next(np.shape(a)[ax] for a, ax in zip(args, axes) if ax is not None)
      return np.stack([fn(*[a if ax is None else np.take(a, i, axis=ax)
                            for a, ax in zip(args, axes)])
                       for i in range(n)], axis=out_axes)
    return mapped

  jax.jit = lambda fn, **kwargs: fn
  jax.vmap = vmap
  jax.Array = np.ndarray
  jax.numpy = jnp
  sys.modules['jax'] = jax
  sys.modules['jax.numpy'] = jnp


_install_jax_stand_in()

from weatherbench2 import regridding as ref_rg  # noqa: E402

from tests import regrid_cases as rc  # noqa: E402
from tests import regrid_np  # noqa: E402

assert ref_rg.__file__.startswith(base.REFERENCE)


def _grids(case):
  return (rc.make_grid(ref_rg, case['source']),
          rc.make_grid(ref_rg, case['target']))


def _put_grid(out, key, grid_spec):
  out[f'{key}/longitudes'] = np.asarray(grid_spec['longitudes'], np.float64)
  out[f'{key}/latitudes'] = np.asarray(grid_spec['latitudes'], np.float64)
  out[f'{key}/flags'] = np.array([grid_spec['periodic'],
                                  grid_spec['includes_poles']])


def _check_ties(cname, case, indices, out):
  dist = regrid_np.haversine_matrix(case['source'], case['target'])
  two = np.partition(dist, 1, axis=1)[:, :2]
  ties = (two[:, 1] - two[:, 0]) < rc.TIE_GAP
  t_shape = (len(case['target']['longitudes']),
             len(case['target']['latitudes']))
  cols, rows = rc.tie_rows_and_columns(case['source'], case['target'])
  allowed = np.zeros(t_shape, dtype=bool)
  allowed[sorted(cols), :] = True
  allowed[:, sorted(rows)] = True
  assert not (ties.reshape(t_shape) & ~allowed).any(), cname
  assert ties.mean() <= 1 / 3, (cname, ties.mean())
  brute = np.argmin(dist, axis=1)
  np.testing.assert_array_equal(indices[~ties], brute[~ties], err_msg=cname)
  out[f'{cname}/nearest/indices'] = np.asarray(indices, dtype=np.int64)
  out[f'{cname}/nearest/ties'] = ties


def _check_bilinear_nan(cname, case):
  """No finite coincident node with a NaN neighbour, on either axis."""
  src, tgt, field = case['source'], case['target'], case['field']
  def coincident(a, b):
    return [i for i, v in enumerate(np.asarray(a, float))
            if (np.asarray(b, float) == v).any()]
  nan = np.isnan(field)
  for j in coincident(src['latitudes'], tgt['latitudes']):
    for k in (j - 1, j + 1):
      if 0 <= k < field.shape[-1]:
        assert not (~nan[..., j] & nan[..., k]).any(), (cname, 'lat', j)
  lat_interp = np.interp if src['includes_poles'] else (
      lambda x, xp, fp: np.interp(x, xp, fp, left=np.nan, right=np.nan))
  flat = field.reshape(-1, field.shape[-1])
  g = np.stack([lat_interp(tgt['latitudes'], src['latitudes'], row)
                for row in flat]).reshape(field.shape[:-1] + (-1,))
  gnan = np.isnan(g)
  n = g.shape[-2]
  for b in coincident(np.asarray(src['longitudes']) % 360,
                      np.asarray(tgt['longitudes']) % 360):
    for k in ((b - 1) % n, (b + 1) % n):
      assert not (~gnan[..., b, :] & gnan[..., k, :]).any(), (cname, 'lon', b)


def generate() -> dict:
  out = {}
  for cname, build in rc.cases().items():
    case = build()
    source, target = _grids(case)
    _put_grid(out, f'{cname}/source', case['source'])
    _put_grid(out, f'{cname}/target', case['target'])
    out[f'{cname}/field'] = case['field']
    out[f'{cname}/seed'] = np.array(case['seed'])
    for name in rc.CLASSES:
      label = rc.LABELS[name]
      regridder = getattr(ref_rg, name)(source, target)
      with np.errstate(all='ignore'):
        ref = np.asarray(regridder.regrid_array(case['field']))
      assert ref.dtype == np.float64, (cname, label, ref.dtype)
      out[f'{cname}/{label}/ref'] = ref
      if name == 'NearestRegridder':
        _check_ties(cname, case, regridder.indices, out)
    if case['nan']:
      _check_bilinear_nan(cname, case)
    with np.errstate(all='ignore'):
      out[f'{cname}/lon_weights'] = np.asarray(
          ref_rg._conservative_longitude_weights(
              source.longitudes, target.longitudes, source.periodic,
              target.periodic))
      out[f'{cname}/lat_weights'] = np.asarray(
          ref_rg._conservative_latitude_weights(
              source.latitudes, target.latitudes, source.includes_poles,
              target.includes_poles))
  for kname, (cls, src, tgt, field, expected) in rc.known_answers().items():
    regridder = getattr(ref_rg, cls)(rc.make_grid(ref_rg, src),
                                     rc.make_grid(ref_rg, tgt))
    with np.errstate(all='ignore'):
      ref = np.asarray(regridder.regrid_array(field))
    if expected is None:
      assert np.isfinite(ref).all(), kname
      expected = np.isfinite(ref)
    else:
      np.testing.assert_allclose(ref, expected, atol=rc.KNOWN_ATOL)
    out[f'known/{kname}/ref'] = ref
    out[f'known/{kname}/expected'] = np.asarray(expected)
  out['structure/structure'] = np.array(
      json.dumps(rc.structure(ref_rg), sort_keys=True))
  return out


def shards(out: dict) -> dict:
  """{shard name: its arrays}: one per case, `known` and `structure` apart."""
  by_shard: dict = {}
  for key, value in out.items():
    by_shard.setdefault(key.split('/')[0], {})[key] = value
  return by_shard


def main():
  out = generate()
  directory = os.environ.get('WB2_REGRID_OUT') or HERE
  for shard, arrays in shards(out).items():
    path = os.path.join(directory, f'{rc.GOLDEN_STEM}.{shard}.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f'wrote {path}: {len(arrays)} arrays, {size / 1e3:.0f} kB')
  for cname in rc.cases():
    for label in rc.LABELS.values():
      a = out[f'{cname}/{label}/ref']
      print(f'{cname:12s} {label:13s} -> {a.shape}  NaN '
            f'{np.isnan(a).sum():4d}/{a.size}')
    print(f'{cname:12s} nearest ties  {out[f"{cname}/nearest/ties"].sum()}')


if __name__ == '__main__':
  main()
