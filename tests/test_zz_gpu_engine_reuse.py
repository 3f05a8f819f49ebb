"""One PatchMatch engine reused across scenes of different sizes gives what fresh engines give (tests/engine_chain_cases.py), on the MI355X."""
import pytest

from tests import engine_chain_cases as ec

pytestmark = pytest.mark.gpu


def test_device_reused_engine_equals_fresh_engines():
    ec.check_reuse()
