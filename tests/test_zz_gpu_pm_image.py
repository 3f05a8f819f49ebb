"""-m gpu, collected last: the engine's image store on the device -- csrc/pm_image.hip through pmhip_image_prepare / _scale / _get, pmhip_scene_set_view_stored and the
device route of densify.load_scene / dense_reconstruction -- against the host code it replaces (densify._resize_area_u8, views.to_gray, densify.scale_image), bit for
bit.  The cases are shared with the emulator suite (tests/pm_image_cases.py, tests/test_emu_pm_image.py); the scene-level ones run at 320 x 240 here, and the two
full-size resizes run only here."""
import pytest

from openmvs_amd import patchmatch
from tests import pm_image_cases as cases

pytestmark = pytest.mark.gpu


def new_engine():
    return patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine():
    e = new_engine()
    yield e
    e.close()


def test_working_size_equals_the_host_rule():
    cases.working_sizes_equal_the_host_rule()
    cases.scaled_sizes_equal_need_scale_image()


@pytest.mark.parametrize("name", cases.RESIZE_NAMES)
def test_resize_and_gray_equal_the_host_code(engine, name):
    cases.resize_equals_the_host_code(engine, cases.RESIZE[cases.RESIZE_NAMES.index(name)])


@pytest.mark.parametrize("case", cases.FULL_SIZE, ids=lambda c: c[0])
def test_full_size_resize_equals_the_host_code(engine, case):
    cases.resize_equals_the_host_code(engine, case)


@pytest.mark.parametrize("size", cases.SCALE_SOURCES, ids=lambda s: "%dx%d" % s)
def test_scale_image_equals_the_host_code(engine, size):
    cases.scale_image_equals_the_host_code(engine, size, patchmatch.PatchMatchError)


def test_errors_leave_the_engine_usable():
    e = new_engine()
    try:
        cases.errors_leave_the_engine_usable(e, patchmatch.PatchMatchError)
    finally:
        e.close()


def test_scene_routes_hold_the_same_images():
    cases.scene_routes_hold_the_same_images(new_engine, "cuda", level=1, min_resolution=160, size=(320, 240))


def test_mixed_sizes_by_both_routes():
    cases.scene_routes_hold_the_same_images(new_engine, "cuda", level=1, min_resolution=160, size=(320, 240), mixed=True, estimate=True)


def test_dense_reconstruction_routes_write_the_same_archive(tmp_path):
    cases.dense_reconstruction_routes_agree(new_engine, tmp_path, level=1, min_resolution=160)
