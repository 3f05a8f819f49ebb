"""The engine's image store (csrc/pm_image.hip, the pmhip_image_* calls, pmhip_scene_set_view_stored and the device route of densify.load_scene) on the CPU: the
product's sources compiled against the wave64 emulator (tests/emu.py), run through the same C ABI and Python mirror as on the device, against the host code they
replace -- bit for bit.  The cases are those of tests/test_zz_gpu_pm_image.py (tests/pm_image_cases.py); the scene-level ones run at 80 x 60 here."""
import pytest

from openmvs_amd import patchmatch
from tests import emu
from tests import pm_image_cases as cases


@pytest.fixture(scope="module")
def emulated():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield lambda: patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine(emulated):
    e = emulated()
    yield e
    e.close()


def test_working_size_equals_the_host_rule(emulated):
    cases.working_sizes_equal_the_host_rule()
    cases.scaled_sizes_equal_need_scale_image()


@pytest.mark.parametrize("name", cases.RESIZE_NAMES)
def test_resize_and_gray_equal_the_host_code(engine, name):
    cases.resize_equals_the_host_code(engine, cases.RESIZE[cases.RESIZE_NAMES.index(name)])


@pytest.mark.parametrize("size", cases.SCALE_SOURCES, ids=lambda s: "%dx%d" % s)
def test_scale_image_equals_the_host_code(engine, size):
    cases.scale_image_equals_the_host_code(engine, size, patchmatch.PatchMatchError)


def test_errors_leave_the_engine_usable(emulated):
    e = emulated()
    try:
        cases.errors_leave_the_engine_usable(e, patchmatch.PatchMatchError)
    finally:
        e.close()


def test_scene_routes_hold_the_same_images(emulated):
    cases.scene_routes_hold_the_same_images(emulated, "cpu", level=3, min_resolution=40, size=(80, 60))


def test_mixed_sizes_by_both_routes(emulated):
    cases.scene_routes_hold_the_same_images(emulated, "cpu", level=3, min_resolution=40, size=(80, 60), mixed=True, estimate=True)


def test_dense_reconstruction_routes_write_the_same_archive(emulated, tmp_path):
    cases.dense_reconstruction_routes_agree(emulated, tmp_path, level=3, min_resolution=40)
