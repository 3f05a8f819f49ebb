"""-m gpu: the view-major lane order of pm_sweep2_kernel on the device -- the cases of tests/lane_order_cases.py against the sequential oracle, bit for bit."""
import pytest

from tests import lane_order_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,lanes", cases.CASES, ids=["%s-lanes%d" % c for c in cases.CASES])
def test_lane_order_case(case, lanes):
    cases.run(case, lanes)
