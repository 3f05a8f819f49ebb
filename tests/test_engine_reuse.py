"""One PatchMatch engine reused across scenes of different sizes gives what fresh engines give (tests/engine_chain_cases.py), under the wave64 emulator."""
import pytest

from openmvs_amd import patchmatch
from tests import emu
from tests import engine_chain_cases as ec


@pytest.fixture(scope="module")
def lib():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as path:
        yield path


def test_reused_engine_equals_fresh_engines(lib):
    ec.check_reuse()
