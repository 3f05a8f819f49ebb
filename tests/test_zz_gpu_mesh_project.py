"""-m gpu, collected last: the mesh renderer of csrc/pm_mesh.hip on the device -- pmhip_mesh_project and pmhip_mesh_visibility on the cases of
tests/mesh_project_cases.py against the host twin (`views.project_mesh`, `views.mesh_visibility`), bit for bit, one engine reused across meshes, sizes and box
thresholds (every face on the lane route, on the workgroup route, and at the default); two engines in one process; a 320-pixel visibility run over 5 views of a
~2 000-face displaced grid; every refusal; `--mesh-file` through `densify.load_scene` and `densify.dense_reconstruction`.  The cases are shared with the emulator suite
(tests/test_emu_mesh_project.py); the C++ driver on the device is tests/test_cpp_mesh_project_driver.py.  Nothing outside the repository is read."""
import os

import numpy as np
import pytest

from openmvs_amd import patchmatch
from tests import mesh_project_cases as cases

pytestmark = pytest.mark.gpu

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.fixture(scope="module")
def engine():
    e = patchmatch.PatchMatchHIP(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", cases.RENDER_CASES, ids=cases.RENDER_IDS)
def test_kernel_render(engine, case):
    cases.run_case(engine, case)


def test_kernel_visibility_edges(engine):
    cases.visibility_edges_case(engine)


def test_kernel_visibility_counts_across_the_word_boundary(engine):
    cases.visibility_counts_case(engine)


def test_kernel_two_engines_in_turn():
    cases.interleaved_engines(lambda: patchmatch.PatchMatchHIP(0))


def test_visibility_of_a_displaced_grid_at_320_pixels(engine):
    cases.grid_visibility_case(engine)


def test_refusals_leave_the_engine_usable(engine):
    cases.error_cases(engine, patchmatch.PatchMatchError)


def test_mesh_file_replaces_the_sparse_cloud_before_view_selection(tmp_path):
    e = patchmatch.PatchMatchHIP(0)
    try:
        cases.mesh_file_case(e, SCENE, tmp_path)
        cases.dense_reconstruction_case(e, SCENE, tmp_path)
    finally:
        e.close()
