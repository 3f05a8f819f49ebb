"""-m gpu, collected last: the image and PLY outputs of csrc/pm_export.hip on the device -- every entry point of include/pmhip_export.h on the cases of
tests/map_export_cases.py against the numpy statements of openmvs_amd/mapexport.py, bit for bit, one engine for the module; then the routes that use them.  The cases
are shared with the emulator suite (tests/test_emu_map_export.py), which also holds the checks of the writers and of the twins alone."""
import os

import pytest

from openmvs_amd import patchmatch
from tests import map_export_cases as cases

pytestmark = pytest.mark.gpu

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.fixture(scope="module")
def engine():
    e = patchmatch.PatchMatchHIP(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65])
def test_kernel_selection_small_counts(engine, n):
    cases.count_case(engine, n)


def test_kernel_selection_counts_around_the_quantum(engine):
    for n in cases.quantum_counts(engine):
        cases.count_case(engine, n)


def test_kernel_selection_past_the_grid_cap(engine):
    cases.past_the_grid_cap(engine)


def test_kernel_selection_value_patterns(engine):
    cases.pattern_cases(engine)


def test_kernel_selection_infinite_median_is_pinned(engine):
    cases.infinite_median_is_pinned(engine)


def test_kernel_selection_without_a_valid_value(engine):
    cases.no_valid_value(engine, patchmatch.PatchMatchError)


@pytest.mark.parametrize("h,w", cases.COLOUR_SIZES)
def test_kernel_colour_map(engine, h, w):
    cases.colour_map_case(engine, h, w)


def test_kernel_colour_map_without_a_valid_pixel(engine):
    cases.no_valid_pixel(engine)


def test_kernel_colour_map_equal_range_is_pinned(engine):
    cases.equal_range_is_pinned(engine)


def test_kernel_normal_image(engine):
    cases.normal_image_cases(engine)


def test_kernel_confidence_image(engine):
    cases.conf_image_cases(engine)


def test_kernel_confidence_image_equal_range_is_pinned(engine):
    cases.equal_confidence_is_pinned(engine)


@pytest.mark.parametrize("w", cases.CLOUD_WIDTHS)
def test_kernel_view_cloud(engine, w):
    cases.view_cloud_case(engine, w, patchmatch.PatchMatchError)


def test_kernel_view_cloud_without_a_valid_pixel(engine, tmp_path):
    cases.empty_view_cloud(engine, tmp_path)


def test_kernel_point_scales(engine):
    cases.scale_cases(engine)
    cases.scale_tie_case(engine)


def test_refusals_leave_the_engine_usable(engine):
    cases.error_cases(engine, patchmatch.PatchMatchError)
    cases.scale_needs_a_cloud_and_cameras(engine, patchmatch.PatchMatchError)


def test_dense_reconstruction_writes_the_verbose_files_and_the_ply(tmp_path):
    e = patchmatch.PatchMatchHIP(0)
    try:
        cases.dense_reconstruction_case(e, SCENE, tmp_path, light=False)
    finally:
        e.close()


def test_export_mesh_depth_maps_writes_colour_mapped_pngs(tmp_path):
    e = patchmatch.PatchMatchHIP(0)
    try:
        cases.mesh_png_case(e, SCENE, tmp_path)
    finally:
        e.close()
