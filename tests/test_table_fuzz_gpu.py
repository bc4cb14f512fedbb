"""The verification-table fuzz on the device (-m gpu): K18 (csrc/event_table
.hip), K19 (csrc/neighborhood.hip), K20 (csrc/crps_bins.hip), K21 (csrc/twcrps
.hip), K22 (csrc/pool.hip) and K24 (csrc/conditional_sums.hip) on the seeded
cases of tests/table_fuzz_cases.py.

Every case runs on the device -- at the engine level the `engine.*` calls and
their folds, at the metric level `compute_chunk` (K22: `pooling.pool`) on
device-backed variables with the forecast in the case's operand form -- and is
held to three things: the package's host path, bit for bit (the K22 pooling
pins no NaN payload: there every NaN is one pattern); a second run of the same
call, bit for bit; and the independent definition of tests/*_np.py -- equal
for the integer tables of K18 and K19, within the bound that module derives
for the float tables (events_np's 2 n u, neighborhood_np.bound, crps_
decomposition_np.table_rtol, twcrps_np.table_rtol, conditional_np.table_atol,
pooling_np.mean_bound + half_ulp, dense_max).  tests/test_table_fuzz_cpu.py
holds the host path to the same definitions without a GPU.

Each case prints the largest deviation from the definition it saw, as a
fraction of the bound; it is a figure to read, the bound is the assertion."""
import pytest

from tests import table_fuzz_cases as fc
from tests import table_fuzz_checks as checks

pytestmark = pytest.mark.gpu

_ID = lambda case: case.id


def _held_to_host_itself_and_the_definition(case):
  host = checks.run(case, device=False)
  dev = checks.run(case, device=True)
  checks.assert_same(case, dev, host, 'device against host')
  again = checks.run(case, device=True)
  checks.assert_same(case, again, dev, 'second run')
  worst = checks.against_definition(case, dev)
  print(f'{case.id}: deviation {worst:.4f} of the bound')
  assert worst <= 1.0


@pytest.mark.parametrize('case', fc.BY_FAMILY['k18'], ids=_ID)
def test_event_tables(case):
  _held_to_host_itself_and_the_definition(case)


@pytest.mark.parametrize('case', fc.BY_FAMILY['k19'], ids=_ID)
def test_fractions(case):
  _held_to_host_itself_and_the_definition(case)


@pytest.mark.parametrize('case', fc.BY_FAMILY['k20'], ids=_ID)
def test_crps_bins(case):
  _held_to_host_itself_and_the_definition(case)


@pytest.mark.parametrize('case', fc.BY_FAMILY['k21'], ids=_ID)
def test_twcrps(case):
  _held_to_host_itself_and_the_definition(case)


@pytest.mark.parametrize('case', fc.BY_FAMILY['k22'], ids=_ID)
def test_pooling(case):
  _held_to_host_itself_and_the_definition(case)


@pytest.mark.parametrize('case', fc.BY_FAMILY['k24'], ids=_ID)
def test_conditional_tables(case):
  _held_to_host_itself_and_the_definition(case)
