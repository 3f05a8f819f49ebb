"""-m gpu: plain SGM on the device -- the wide uniform Match of csrc/sgm_kernels_wide.hip through sgmhip_set_problem_uniform (D up to 1024) and the resident plain loop
(sgmhip_tsgm_match with minResolution 0) on the cases of tests/sgm_plain_cases.py, bit for bit against oracle.pyoracle: cost volume, 8-path sums, disparity, cost.
Every case first asserts that it reaches the edge it is named after.

This file is the judge of what the emulator cannot see: the conversion of a grey difference that is not finite, the real DPP wave shifts across 16-lane rows, and the
packed 16-bit atomics of the device."""
import pytest

from openmvs_amd import sgm
from tests import sgm_plain_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


@pytest.mark.parametrize("entry", [1, 256, "last"])
@pytest.mark.parametrize("D", pc.SWEEP_D)
def test_device_sweep(matcher, D, entry):
    """the planted disparity at entry 1, 256 and D - 2 of a range of D entries, byte deltas and u16 sums"""
    pc.check_case(matcher, pc.sweep_case(D, entry))


@pytest.mark.parametrize("side", ["right", "left"])
def test_device_range_outside_the_image(matcher, side):
    pc.check_case(matcher, pc.outside_case(side))


@pytest.mark.parametrize("k", range(3))
def test_device_degenerate_grids(matcher, k):
    pc.check_case(matcher, pc.degenerate_cases()[k])


@pytest.mark.parametrize("k", range(5))
def test_device_chunk_boundaries(matcher, k):
    pc.check_case(matcher, pc.chunk_cases()[k])


def test_device_non_finite_grey(matcher):
    pc.check_case(matcher, pc.nonfinite_case())


@pytest.mark.parametrize("k", range(3))
def test_device_refine_after_a_wide_match(matcher, k):
    pc.check_refine(matcher, pc.refine_cases()[k])


@pytest.mark.parametrize("D", pc.NARROW_D)
def test_device_narrow_ranges_through_the_uniform_entry(matcher, D):
    pc.check_narrow(matcher, D)


def test_device_refusals(matcher):
    for _ in range(2):
        pc.check_refusals(matcher)


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_device_resident_loop_against_the_stepwise_loop(matcher, name):
    pc.check_loop(matcher, None, name)


def test_device_loop_errors(matcher):
    pc.check_loop_errors(matcher)


def test_device_sizes_interleaved(matcher):
    """a wide problem, a narrow one and a wide one again on one engine: what the larger problem left in the volumes must not show"""
    for c in (pc.sweep_case(1024, 1), pc.narrow_case(2), pc.sweep_case(513, "last"), pc.degenerate_cases()[0], pc.sweep_case(1024, 256)):
        pc.check_case(matcher, c)


def test_device_pipeline_routes_agree(matcher):
    """match_pair(min_resolution=0) on the test scene at level 2 (seeded D = 66; see check_pipeline for why that level): host-rectified == device-rectified == oracle"""
    pc.check_pipeline(matcher)
