"""Plain SGM on the CPU: libsgmhip compiled against the wave64 emulator (tests/emu.py), through the C ABI -- the wide uniform Match of csrc/sgm_kernels_wide.hip
(sgmhip_set_problem_uniform, D up to 1024) and the resident plain loop (sgmhip_tsgm_match with minResolution 0) on the cases of tests/sgm_plain_cases.py, bit for bit
against oracle.pyoracle.  Forwards here, and with every workgroup and lane in reverse in a child run: the atomic sums and the byte volumes' "each byte written once"
must not depend on who comes first.

The conversion of a grey difference that is not finite cannot fail here -- the emulator converts as x86 does; the device file tests/test_zz_gpu_sgm_plain.py is its
judge."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import sgm
from tests import emu
from tests import sgm_plain_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def matcher():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        m = sgm.SemiGlobalMatcherHIP(0)
        yield m
        m.close()


@pytest.mark.parametrize("D", pc.SWEEP_D)
def test_emulated_sweep(matcher, D):
    """the planted disparity at entry 1, 256 and D - 2 of a range of D entries, byte deltas and u16 sums"""
    for c in pc.sweep_cases(D):
        pc.check_case(matcher, c)


@pytest.mark.parametrize("side", ["right", "left"])
def test_emulated_range_outside_the_image(matcher, side):
    pc.check_case(matcher, pc.outside_case(side))


@pytest.mark.parametrize("k", range(3))
def test_emulated_degenerate_grids(matcher, k):
    pc.check_case(matcher, pc.degenerate_cases()[k])


@pytest.mark.parametrize("k", range(5))
def test_emulated_chunk_boundaries(matcher, k):
    pc.check_case(matcher, pc.chunk_cases()[k])


def test_emulated_non_finite_grey(matcher):
    pc.check_case(matcher, pc.nonfinite_case())


@pytest.mark.parametrize("k", range(3))
def test_emulated_refine_after_a_wide_match(matcher, k):
    pc.check_refine(matcher, pc.refine_cases()[k])


@pytest.mark.parametrize("D", pc.NARROW_D)
def test_emulated_narrow_ranges_through_the_uniform_entry(matcher, D):
    pc.check_narrow(matcher, D)


def test_emulated_refusals(matcher):
    pc.check_refusals(matcher)


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_emulated_resident_loop_against_the_stepwise_loop(matcher, name):
    pc.check_loop(matcher, None, name)


def test_emulated_loop_errors(matcher):
    pc.check_loop_errors(matcher)


def test_emulated_zz_no_lane_ever_read_a_lane_that_was_not_there(matcher):
    """Runs last of the emulated tests: over every case above, no DPP shift or readlane took its value from a lane that was not executing the same operation."""
    launches, fibers, exchanges, inactive = emu.counters(sgm)
    assert launches > 500 and exchanges > 100000
    assert inactive == 0, "%d cross-lane reads of non-participating lanes" % inactive


@pytest.mark.parametrize("order", ["reverse"])
def test_results_do_not_depend_on_the_execution_order(order):
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    env = dict(os.environ, HIPEMU_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "emulated"],
                       cwd=os.path.dirname(HERE), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=2400)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
