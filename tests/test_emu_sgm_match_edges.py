"""SemiGlobalMatcher::Match on the hand-built problems of tests/sgm_match_edge_cases.py, on the CPU: libsgmhip compiled against the wave64 emulator (tests/emu.py), through
the C ABI, in every mapping of work to lanes and on both aggregation routes, against oracle.pyoracle.sgm_match bit for bit -- cost volume, 8-path sums, disparity and cost.
Every problem first proves, on its inputs or on the oracle's result, that it reaches the edge it is named after.  Forwards here, and with every workgroup and lane in
reverse in a child run: the atomic sums and the byte volumes' "each byte written once" must not depend on who comes first.

The conversion of a grey difference that is not finite cannot fail here -- the emulator converts as x86 does; the device file tests/test_zz_gpu_sgm_match_edges.py is
its judge."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import sgm
from tests import emu
from tests import sgm_match_edge_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def matcher():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        m = sgm.SemiGlobalMatcherHIP(0)
        yield m
        m.close()


@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_emulated_match(matcher, family):
    assert ec.check_family(matcher, family) >= 4 * len(ec.problems(family))


def test_emulated_refusals(matcher):
    """P1 above an entry of the table and an entry with 8 (255 + P2) > 65535 raise SGMError from Match and from the resident loop; the engine stays usable."""
    ec.check_refusals(matcher)


def test_emulated_zz_no_lane_ever_read_a_lane_that_was_not_there(matcher):
    """Runs last of the emulated tests: over every problem above, no DPP shift, shuffle or readlane took its value from a lane that was not executing the same operation."""
    launches, fibers, exchanges, inactive = emu.counters(sgm)
    assert launches > 1000 and exchanges > 100000
    assert inactive == 0, "%d cross-lane reads of non-participating lanes" % inactive


@pytest.mark.parametrize("order", ["reverse"])
def test_results_do_not_depend_on_the_execution_order(order):
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    env = dict(os.environ, HIPEMU_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "emulated"],
                       cwd=os.path.dirname(HERE), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
