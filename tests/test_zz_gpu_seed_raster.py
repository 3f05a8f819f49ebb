"""-m gpu, collected last: the seed rasteriser of csrc/seed_raster.hip on the device -- pmhip_seed_raster and pmhip_scene_seed_view on the cases of
tests/seed_raster_cases.py against the literal sequential walk (`views._raster_face` face after face, the 2x2 loop) and, where oracle/_ref is built, the reference's
compiled rasteriser, bit for bit, one engine reused across meshes, sizes, modes and box thresholds; every refusal; `seed_on_device` through `densify.load_scene`,
`compute_depth_maps` and `dense_reconstruction` at 320 x 240; one 1920 x 1080 mesh of the test scene's points against the reference's rasteriser.  The cases are
shared with the emulator suite (tests/test_emu_seed_raster.py).  Nothing outside the repository is read."""
import pytest

from openmvs_amd import patchmatch, sgm
from oracle import pyref
from tests import seed_raster_cases as cases
from tests import sgm_seed_cases as sgm_cases

pytestmark = pytest.mark.gpu


def new_engine():
    return patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine():
    e = new_engine()
    yield e
    e.close()


@pytest.mark.parametrize("case", cases.DELAUNAY_CASES, ids=cases.DELAUNAY_IDS)
def test_faces_of_random_delaunay_meshes(engine, case):
    cases.run_case(engine, case)


def test_faces_of_an_integer_grid_follow_the_order_of_the_list(engine):
    cases.grid_case(engine)


@pytest.mark.parametrize("case", cases.BOX_CASES, ids=cases.BOX_IDS)
def test_box_rules_on_their_boundaries(engine, case):
    cases.box_case(engine, case)


def test_back_facing_and_collinear_faces_are_skipped(engine):
    cases.culled_case(engine)


def test_maps_do_not_depend_on_the_box_threshold(engine):
    cases.routes_case(engine)


def test_normals_that_cancel_give_zeros(engine):
    cases.zero_normal_case(engine)


@pytest.mark.parametrize("case", cases.POINTS_CASES, ids=cases.POINTS_IDS)
def test_points(engine, case):
    cases.points_case(engine, case)


def test_empty_meshes_give_zero_maps(engine):
    cases.empty_case(engine)


def test_refusals_leave_the_engine_usable(engine):
    cases.refusal_cases(engine, patchmatch.PatchMatchError)


def test_scene_seed_view_is_scene_set_maps_of_the_host_maps():
    e = new_engine()
    try:
        cases.scene_view_case(e)
    finally:
        e.close()


@pytest.mark.parametrize("sparse", [True, False], ids=["bInitSparse_1", "bInitSparse_0"])
def test_scene_routes_give_the_same_maps(sparse):
    cases.scene_routes_agree(new_engine, level=1, min_resolution=160, size=(320, 240), sparse=sparse)


def test_dense_reconstruction_routes_write_the_same_archive(tmp_path):
    cases.dense_reconstruction_routes_agree(new_engine, tmp_path, level=1, min_resolution=160)


def test_full_hd_faces_against_the_reference_rasteriser(engine):
    assert pyref.fuse_available(), "oracle/_ref/libref_fuse.so travels with the tree"
    cases.full_hd_case(engine)


# ---- the SGM route: include/sgmhip_seed.h ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


def test_sgm_seed_steps_equal_the_host_seed(matcher):
    sgm_cases.seed_steps_case(matcher, sgm.SGMError, level=0, min_resolution=160)


@pytest.mark.parametrize("level,min_resolution", [(0, 160), (2, 0)], ids=["tsgm", "plain"])
def test_match_pair_seed_routes_agree(matcher, level, min_resolution):
    sgm_cases.match_pair_seed_routes_agree(matcher, sgm.SGMError, level=level, min_resolution=min_resolution)
