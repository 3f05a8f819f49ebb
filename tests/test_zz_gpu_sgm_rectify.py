"""The device rectification of the SGM path on the device: csrc/sgm_rectify.hip through sgmhip_scene_* / sgmhip_rectify_pair / sgmhip_rectified_get /
sgmhip_tsgm_match_rectified and the device route of sgm_pipeline, against the host code they replace (rectify.warp_perspective_u8 +
sgm_pipeline.to_gray_linear, then the uploaded-images loop) -- bit for bit.  The cases are shared with the emulator suite (tests/sgm_rectify_cases.py,
tests/test_emu_sgm_rectify.py); the full-size ones run only here."""
import pytest

from openmvs_amd import sgm
from tests import sgm_rectify_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_rectified_pair_equals_the_host_code(matcher, name):
    cases.same_bits(matcher, cases.CASES[cases.NAMES.index(name)])


def test_real_pair_at_the_scene_size(matcher):
    cases.same_bits(matcher, cases.real_pair_case())                             # 640 x 479 sources, H1 / H2 of pair (0, 2)


def test_errors_leave_the_engine_usable():
    fresh = sgm.SemiGlobalMatcherHIP(0)                                          # an engine that never rectified a pair
    try:
        cases.errors_leave_the_engine_usable(fresh, sgm.SGMError)
    finally:
        fresh.close()


def test_match_pair_device_route_equals_host_route(matcher):
    cases.match_pair_routes_agree(matcher, level=0, min_resolution=160)         # full-size images


def test_dense_reconstruction_device_route_writes_the_same_files(matcher, tmp_path):
    cases.dense_reconstruction_routes_agree(matcher, tmp_path)
