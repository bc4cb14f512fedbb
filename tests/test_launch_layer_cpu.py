"""The reduction launch layer (engine.PreparedLaunch, engine.hooked_call and
the entry points built on them) on CPU plans, with a recording stand-in in the
place of libwb2hip.so: the host-only geometry functions pass through to the real
library (it loads without a GPU), every launch is recorded and returns the
stand-in's status.

For every entry form: the plan's arguments that reach C -- spelled here in the
order of include/wb2hip.h -- are the fields of the `wb2_plan_tables` struct
`plan_tables` builds for the same plan and tile, and those of
`plan.seg_entries` at the tile the library reports; `partials` is
[n_outer, n_chunk, nwf, n_ts, k]; the profiling hook sees the bracket the entry
always had; a failed call raises and sends no 'end'."""
import ctypes
import types

import numpy as np
import pytest
import torch

from weatherbench2_amd import _lib, engine, plan as plan_lib, program
from weatherbench2_amd import regions as R, xarray_lite as xl

HOST_ONLY = {'wb2_num_slots', 'wb2_ens_num_slots', 'wb2_tile_cols_ex',
             'wb2_ens_tile_cols', 'wb2_energy_layout', 'wb2_pairs_supported',
             'wb2_last_error'}
_REST = ['chunk_row0', 'chunk_nrow', 'n_chunk', 'n_ctile', 'seg_col0',
         'seg_eoff', 'n_seg', 'n_ts']
STREAM = ['n_row', 'n_col', 'w_row', 'w_col', 'wfield', 'wfield_dtype', 'aux',
          'scalar'] + _REST
ENS = ['n_row', 'n_col', 'w_row', 'w_col', 'wfield'] + _REST
FOLD = ['n_chunk', 'nwf', 'n_seg', 'seg_eoff', 'n_ts', 'band_chunk0', 'n_band',
        'coef_band', 'coef_seg', 'region_wf', 'region_wsum', 'n_region']
# entry point -> (position of n_outer, the plan's arguments behind it)
LONG = {'wb2_stream_partials_ex': (5, STREAM),
        'wb2_stream_partials_addr': (5, STREAM),
        'wb2_ens_partials_maps': (8, ENS), 'wb2_ens_partials_gather': (6, ENS),
        'wb2_ens_partials_addr': (6, ENS),
        'wb2_ens_threshold_partials': (10, ENS)}
FOLDS = {'wb2_det_combine': 3, 'wb2_ens_combine': 2}   # position of n_outer
# entry point -> (position of the struct, of n_outer, of partials)
STRUCT = {'wb2_det_suite_step': (0, 7, 8), 'wb2_det_wind_suite_step': (0, 7, 9),
          'wb2_energy_score': (9, 8, 10)}
N_OUTER = N_MEMBER = 3
MODE = _lib.MODE_DET_ACC


class StandIn:
  """libwb2hip.so with every launch recorded instead of run."""

  def __init__(self):
    self.real, self.calls, self.status = _lib.load(), [], 0

  def __getattr__(self, name):
    if name in HOST_ONLY:
      return getattr(self.real, name)

    def record(*args):
      self.calls.append((name, args))
      return self.status
    return record


@pytest.fixture
def lib(monkeypatch):
  stand_in = StandIn()
  monkeypatch.setattr(_lib, '_lib', stand_in)
  monkeypatch.setattr(engine, 'current_stream_ptr', lambda device: 0)
  made, empty = [], torch.empty

  def recording_empty(*args, **kw):
    made.append(empty(*args, **kw))   # (kept: no address comes twice)
    return made[-1]
  monkeypatch.setattr(torch, 'empty', recording_empty)
  stand_in.shape_at = lambda address: next(
      tuple(x.shape) for x in reversed(made) if x.data_ptr() == address)
  return stand_in


def _case(n_lat, n_lon, dtype, land):
  lat = np.linspace(-75, 75, n_lat)
  lon = np.arange(n_lon) * (360.0 / n_lon)
  regions = {'global': None, 'tropics': R.SliceRegion(lat_slice=slice(-20, 20)),
             'east': R.SliceRegion(lon_slice=slice(100, 300))}
  if land:
    lsm = (np.random.RandomState(3).uniform(size=(n_lat, n_lon)) > 0.4)
    regions['land'] = R.LandRegion(land_sea_mask=xl.DataArray(
        lsm.astype(np.float32), ('latitude', 'longitude'),
        {'latitude': lat, 'longitude': lon}))
  pl = plan_lib.build_plan(lat, lon, plan_lib.LATLON, regions, 'cpu',
                           rows_per_chunk=5)
  assert (pl.wfield is not None) == land == (pl.wfield32 is not None)
  zeros = lambda *shape: torch.zeros(shape + (n_lat, n_lon), dtype=dtype)
  ins = [zeros(N_OUTER) for _ in range(3)]
  size = n_lat * n_lon * ins[0].element_size()
  return types.SimpleNamespace(
      pl=pl, dtype=dtype, ins=ins, ens=zeros(N_MEMBER, N_OUTER),
      truth=zeros(N_OUTER), thr=zeros(N_OUTER),
      stride=N_OUTER * n_lat * n_lon,
      ident=[torch.arange(N_OUTER) for _ in range(3)],
      addr=[x.data_ptr() + torch.arange(N_OUTER) * size for x in ins],
      member_ptrs=torch.zeros((N_OUTER, N_MEMBER), dtype=torch.int64),
      addresses=torch.zeros((2, N_OUTER), dtype=torch.int64),
      out=torch.zeros((_lib.NMETRIC_ENS * pl.n_region * N_OUTER,),
                      dtype=torch.float64))


def _suite_step(c, by_address, bind):
  step = engine.SuiteStep(c.pl, MODE, c.dtype, False, N_OUTER,
                          by_address=by_address)
  args = (None, c.addr) if by_address else (c.ins, c.ident)
  return step.bind(*args)() if bind else step.run(*args)


def _ens_pass(c):
  p = program._EnsPass()
  p._setup(c.pl, False, c.dtype, N_MEMBER, c.stride, N_OUTER)
  p.launch(c.addresses.data_ptr(), c.out, 0)


def _ens(c, **kw):
  return engine.ensemble_reduce(c.pl, c.ens, c.stride, N_MEMBER, None, c.truth,
                                None, N_OUTER, False, **kw)


# name -> (the call, the hook's kernel -- None: the entry has no bracket --,
#          'det' or 'ens': whose tile and slot count)
ENTRIES = {
    'stream_reduce': (lambda c: engine.stream_reduce(
        c.pl, MODE, c.ins, [None] * 3, N_OUTER, False), 'stream_partials',
                      'det'),
    'stream_reduce-slabs': (lambda c: engine.stream_reduce(
        c.pl, MODE, c.ins, c.ident, N_OUTER, False, want_sums=True),
                            'stream_partials', 'det'),
    'stream_reduce_addr': (lambda c: engine.stream_reduce_addr(
        c.pl, MODE, c.dtype, c.addr, True, N_OUTER, False), 'stream_partials',
                           'det'),
    'SuiteStep.run': (lambda c: _suite_step(c, False, False),
                      'stream_partials', 'det'),
    'SuiteStep.run-addr': (lambda c: _suite_step(c, True, False),
                           'stream_partials', 'det'),
    'SuiteStep.bind': (lambda c: _suite_step(c, False, True), None, 'det'),
    'SuiteStep.bind-addr': (lambda c: _suite_step(c, True, True), None, 'det'),
    'PairSuiteStep.run': (lambda c: engine.PairSuiteStep(
        c.pl, MODE, c.dtype, False, N_OUTER, 0).run(c.ins, c.ident),
                          'stream_partials', 'det'),
    'ensemble_reduce': (_ens, 'ens_partials', 'ens'),
    'ensemble_reduce-member_ptrs': (
        lambda c: _ens(c, member_ptrs=c.member_ptrs), 'ens_partials', 'ens'),
    'ensemble_reduce-addresses': (
        lambda c: _ens(c, addresses=c.addresses), 'ens_partials', 'ens'),
    'ensemble_threshold_reduce': (lambda c: engine.ensemble_threshold_reduce(
        c.pl, c.ens, c.stride, N_MEMBER, None, c.truth, None, c.thr, None,
        N_OUTER, False), None, 'thr'),
    'energy_score': (lambda c: engine.energy_score(
        c.pl, c.ens, c.stride, N_MEMBER, None, c.truth, None, N_OUTER, False),
                     'energy_score', 'energy'),
    '_EnsPass': (_ens_pass, 'ens_partials', 'ens'),
}
GRIDS = [(6, 7, torch.float32),   # one full 4-wide vector + a shifted last lane
         (6, 3, torch.float32),   # one column per lane
         (5, 3, torch.float64)]


def _expected(lib, c, kind):
  """(the struct of plan_tables, the shape of partials) of a launch."""
  pl, real = c.pl, lib.real
  has_field = int(pl.wfield is not None)
  rows = N_OUTER
  if kind == 'det':
    tile = real.wb2_tile_cols_ex(MODE, engine.dtype_code(c.dtype), 0, has_field,
                                 pl.n_col, 1)
    field, code = pl.wfield, _lib.WB2_F64
    if c.dtype == torch.float32 and has_field:
      field, code = pl.wfield32, _lib.WB2_F32
    k = real.wb2_num_slots(MODE, 0)
  else:
    tile = real.wb2_ens_tile_cols(pl.n_col)
    field, code = pl.wfield, _lib.WB2_F64
    k = {'ens': real.wb2_ens_num_slots(0),
         'thr': real.wb2_num_slots(_lib.MODE_ENS_THR, 0)}.get(kind)
    if kind == 'energy':
      out = [ctypes.c_int32() for _ in range(3)]
      assert real.wb2_energy_layout(N_MEMBER, 0, has_field,
                                    *map(ctypes.byref, out)) == 0
      rows, k = N_OUTER * out[1].value, out[2].value
  tables, _ = engine.plan_tables(pl, tile, field, code)
  seg_eoff, n_ts = pl.seg_entries(tile)
  assert (tables.seg_eoff, tables.n_ts, tables.n_ctile) == (
      seg_eoff.data_ptr(), n_ts, -(-pl.n_col // tile))
  return tables, (rows, pl.n_chunk, pl.nwf, n_ts, k)


@pytest.mark.parametrize('land', [False, True], ids=['global', 'land'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}-{g[2]}')
@pytest.mark.parametrize('entry', ENTRIES)
def test_entry_reaches_c_with_the_plan_of_plan_tables(lib, entry, grid, land):
  call, kernel, kind = ENTRIES[entry]
  c = _case(*grid, land)
  want, shape = _expected(lib, c, kind)
  field_of = lambda f: c.pl.nwf if f == 'nwf' else getattr(want, f) or 0
  events = []
  old = engine.set_launch_hook(lambda when, what: events.append((when, what)))
  try:
    call(c)
  finally:
    engine.set_launch_hook(old)
  assert events == ([('begin', kernel), ('end', kernel)] if kernel else [])
  seen = set()
  for name, args in lib.calls:
    partials = None
    if name in LONG:
      at, names = LONG[name]
      got = args[at + 1:at + 1 + len(names)]
      partials = args[at + 1 + len(names)]
    elif name in FOLDS:
      at, names = FOLDS[name], FOLD
      got = args[at + 1:at + 1 + len(names)]
      assert lib.shape_at(args[at - 1]) == shape
    else:
      at_struct, at, at_partials = STRUCT[name]
      names = [f for f, _ in _lib.PlanTables._fields_]
      got = [getattr(args[at_struct]._obj, f) for f in names]
      partials = args[at_partials]
    assert [v or 0 for v in got] == [field_of(f) for f in names], name
    assert args[at] == N_OUTER
    if partials is not None:
      assert lib.shape_at(partials) == shape, name
    seen.add(name)
  assert seen & (set(LONG) | set(STRUCT)), 'no launch was recorded'


@pytest.mark.parametrize('entry', ENTRIES)
def test_failed_call_raises_and_sends_no_end(lib, entry):
  call, kernel, _ = ENTRIES[entry]
  c = _case(6, 7, torch.float32, True)
  lib.status = -1
  events = []
  old = engine.set_launch_hook(lambda when, what: events.append((when, what)))
  try:
    with pytest.raises(_lib.Wb2HipError):
      call(c)
  finally:
    engine.set_launch_hook(old)
  assert events == ([('begin', kernel)] if kernel else [])
  assert len(lib.calls) == 1   # nothing is launched behind a failed call
