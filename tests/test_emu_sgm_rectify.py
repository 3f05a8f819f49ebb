"""The device rectification of the SGM path (csrc/sgm_rectify.hip, the sgmhip_scene_* / sgmhip_rectify_pair / sgmhip_tsgm_match_rectified calls and the
device route of sgm_pipeline) on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py, the pattern of
tests/test_emu_kernels.py), run through the same C ABI and Python mirror as on the device, against the host code they replace -- bit for bit.
The cases are those of tests/test_zz_gpu_sgm_rectify.py (tests/sgm_rectify_cases.py)."""
import pytest

from openmvs_amd import sgm
from tests import emu
from tests import sgm_rectify_cases as cases


@pytest.fixture(scope="module")
def matcher():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        m = sgm.SemiGlobalMatcherHIP(0)
        yield m
        m.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_rectified_pair_equals_the_host_code(matcher, name):
    cases.same_bits(matcher, cases.CASES[cases.NAMES.index(name)])


def test_errors_leave_the_engine_usable(matcher):
    fresh = sgm.SemiGlobalMatcherHIP(0)                                         # (an engine that never rectified a pair; `matcher` keeps the emulated library loaded)
    try:
        cases.errors_leave_the_engine_usable(fresh, sgm.SGMError)
    finally:
        fresh.close()


def test_match_pair_device_route_equals_host_route(matcher):
    cases.match_pair_routes_agree(matcher, level=2, min_resolution=40)          # quarter-size images


def test_dense_reconstruction_device_route_writes_the_same_files(matcher, tmp_path):
    cases.dense_reconstruction_routes_agree(matcher, tmp_path)
