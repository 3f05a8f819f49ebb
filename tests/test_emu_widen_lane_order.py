"""pm_sweep_widen_kernel at the edges of its lane and workgroup maps on the wave64 emulator (tests/cpp/hipemu): the cases of
tests/widen_lane_order_cases.py against the sequential oracle, bit for bit, and no cross-lane read of a lane that was not taking part."""
import pytest

from openmvs_amd import patchmatch
from tests import emu, widen_lane_order_cases as cases


@pytest.fixture(scope="module")
def pm_emulated():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield


@pytest.mark.parametrize("case,hyps", cases.CASES, ids=["%s-hyps%d" % c for c in cases.CASES])
def test_widen_lane_order_case(pm_emulated, case, hyps):
    before = emu.counters(patchmatch)
    cases.run(case, hyps)
    after = emu.counters(patchmatch)
    assert after[0] > before[0] and after[2] > before[2]
    assert after[3] == before[3], "%d cross-lane reads of lanes that did not take part" % (after[3] - before[3])
