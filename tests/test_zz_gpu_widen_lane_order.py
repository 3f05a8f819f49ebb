"""-m gpu: pm_sweep_widen_kernel at the edges of its lane and workgroup maps on the device -- the cases of tests/widen_lane_order_cases.py against the sequential oracle, bit for bit."""
import pytest

from tests import widen_lane_order_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,hyps", cases.CASES, ids=["%s-hyps%d" % c for c in cases.CASES])
def test_widen_lane_order_case(case, hyps):
    cases.run(case, hyps)
