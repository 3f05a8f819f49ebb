"""-m gpu, collected last: MVS::EstimateNormalMap of csrc/pm_normal.hip on the device -- both entry points (pmhip_estimate_normal_map, pmhip_scene_estimate_normals) on
the cases of tests/normal_map_cases.py against `views.estimate_normal_map`, bit for bit, one engine reused across the sizes; the map larger than one pass of the launch's
capped grid (only here); then the two routes that use it: the resume of a .dmap stored without normals, and `--fusion-mode -2` through to the cloud on
`DeviceBackend(SemiGlobalMatcherHIP(0), PatchMatchHIP(0))`.  The cases are shared with the emulator suite (tests/test_emu_normal_map.py), which also holds the checks
on the host statement alone."""
import os

import pytest

from openmvs_amd import patchmatch
from tests import normal_map_cases as cases

pytestmark = pytest.mark.gpu

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.fixture(scope="module")
def engine():
    e = patchmatch.PatchMatchHIP(0)
    yield e
    e.close()


def test_kernel_tilted_plane(engine):
    cases.tilted_plane_case(engine)


def test_kernel_never_three_neighbours(engine):
    cases.never_three_neighbours(engine)


def test_kernel_two_by_two_and_three_by_three(engine):
    cases.two_by_two(engine)
    cases.three_by_three(engine)


@pytest.mark.parametrize("transpose", (0, 1), ids=("widths", "heights"))
@pytest.mark.parametrize("n", cases.WIDTHS)
def test_kernel_sizes_around_the_wave_and_the_block(engine, n, transpose):
    cases.width_case(engine, n, transpose)


def test_kernel_rows_that_end_inside_a_group_of_pixels(engine):
    cases.row_end_case(engine)


def test_kernel_stride_loop_takes_a_second_trip(engine):
    cases.stride_case(engine)


def test_kernel_zero_and_negative_depths(engine):
    cases.zeros_and_negatives(engine)


def test_kernel_every_count_of_similar_neighbours(engine):
    cases.checkerboard_counts(engine)
    cases.two_and_three_neighbours(engine)


def test_kernel_non_finite_depths(engine):
    cases.non_finite(engine)


@pytest.mark.parametrize("magnitude", cases.MAGNITUDES)
def test_kernel_three_per_cent_test_is_strict(engine, magnitude):
    cases.threshold_case(engine, magnitude)


@pytest.mark.parametrize("scale", cases.SCALES)
def test_kernel_arithmetic_at_depth_magnitudes(engine, scale):
    cases.arithmetic_case(engine, scale)


def test_kernel_scene_views_at_their_own_size(engine):
    cases.scene_case(engine)


def test_kernel_sizes_in_turn_on_one_engine(engine):
    cases.interleaved_sizes(engine)


def test_refusals_leave_the_engine_usable(engine):
    cases.error_cases(engine, patchmatch.PatchMatchError)


def test_resume_of_a_dmap_without_normals_estimates_them_on_the_engine(tmp_path, monkeypatch):
    e = patchmatch.PatchMatchHIP(0)
    try:
        cases.resume_case(e, tmp_path, monkeypatch)
    finally:
        e.close()


def test_mode_minus_2_through_to_the_cloud(tmp_path):
    from openmvs_amd import sgm, sgm_pipeline
    be = sgm_pipeline.DeviceBackend(sgm.SemiGlobalMatcherHIP(0), patchmatch.PatchMatchHIP(0))
    try:
        cases.mode2_case(be, SCENE, tmp_path)
    finally:
        be.e.close()
        be.m.close()
