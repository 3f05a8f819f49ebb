"""The mesh renderer of csrc/pm_mesh.hip on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py), pmhip_mesh_project and
pmhip_mesh_visibility on the cases of tests/mesh_project_cases.py against the host twin (`views.project_mesh`, `views.mesh_visibility`), bit for bit, at the default
box threshold and with every face forced onto the lane route and onto the workgroup route; the kernel cases again with lanes and workgroups executed in reverse (the
64-bit atomicMin makes the result independent of the order); every refusal of include/pmhip_mesh.h; and `--mesh-file` through `densify.load_scene`.  The cases are
those of tests/test_zz_gpu_mesh_project.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openmvs_amd import patchmatch
from tests import emu
from tests import mesh_project_cases as cases

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.fixture(scope="module")
def emulated():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield lambda: patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine(emulated):
    e = emulated()
    yield e
    e.close()


def test_the_emulated_library_exports_the_mesh_entry_points(emulated):
    import re
    lib = patchmatch.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pmhip_mesh.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(pmhip_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted(patchmatch.MESH_EXPORTS) and {"pmhip_mesh_set", "pmhip_mesh_get_vertex_normals", "pmhip_mesh_project", "pmhip_mesh_visibility", "pmhip_mesh_release"} <= set(names)
    assert all(hasattr(lib, n) and getattr(lib, n).argtypes is not None for n in names) and hasattr(lib, "hipemu_counters")
    assert '#include "pmhip_mesh.h"' in open(os.path.join(root, "include", "pmhip.h")).read()
    assert len(lib.pmhip_mesh_project.argtypes) == 8 and len(lib.pmhip_mesh_visibility.argtypes) == 8 and len(lib.pmhip_mesh_set.argtypes) == 6


@pytest.mark.parametrize("case", cases.RENDER_CASES, ids=cases.RENDER_IDS)
def test_kernel_render(engine, case):
    cases.run_case(engine, case)


def test_kernel_visibility_edges(engine):
    cases.visibility_edges_case(engine)


def test_kernel_visibility_counts_across_the_word_boundary(engine):
    cases.visibility_counts_case(engine)


def test_kernel_visibility_of_a_displaced_grid_at_320_pixels(engine):
    cases.grid_visibility_case(engine)


def test_kernel_two_engines_in_turn(emulated):
    cases.interleaved_engines(emulated)


def test_refusals_leave_the_engine_usable(engine):
    cases.error_cases(engine, patchmatch.PatchMatchError)


def test_destroy_releases_the_mesh(emulated):
    e = emulated()
    c = cases.RENDER_CASES[0]
    e.mesh_set(c.V, c.F)
    e.close()
    e = emulated()
    try:
        e.mesh_set(c.V, c.F); e.Release()                                  # pmhip_release frees it too
        with pytest.raises(patchmatch.PatchMatchError, match="no mesh"):
            e.mesh_project([c.cams[0][0]], [c.cams[0][1]], [c.cams[0][2]], [c.cams[0][3:]])
    finally:
        e.close()


def test_mesh_memory_is_owned_and_a_failing_allocation_leaks_nothing(emulated):
    """The emulator counts live device allocations and can fail the k-th one (tests/test_engine_memory.py): release, destroy and a replaced mesh leave nothing behind,
    and a render whose k-th allocation fails is PMHIP_E_HIP, after which the same call succeeds."""
    import ctypes as C
    lib = patchmatch.load_library()

    def live():
        out = (C.c_uint64 * 2)()
        lib.hipemu_live_allocs(out)
        return int(out[0]), int(out[1])
    start = live()
    c, big = cases.RENDER_CASES[0], cases.RENDER_CASES[-4]
    K, R, Cc = (np.array([v[k] for v in c.cams]) for k in range(3))
    e = emulated()
    e.mesh_set(big.V, big.F); e.mesh_project(*(np.array([v[k] for v in big.cams]) for k in range(3)), [v[3:] for v in big.cams])
    held = live()
    assert held[0] > start[0]
    e.mesh_set(c.V, c.F)                                                   # a mesh replaces the one before, working buffers included
    assert live()[0] == start[0] + 3 and live()[1] < held[1]
    for k in range(1, 9):
        lib.hipemu_fail_malloc_at(C.c_int64(k))
        try:
            e.mesh_project(K, R, Cc, [c.cams[0][3:]])
        except patchmatch.PatchMatchError as ex:
            assert "pmhip error -3" in str(ex)
        else:
            break
        finally:
            lib.hipemu_fail_malloc_at(C.c_int64(0))
    assert k > 4, "the render allocates its working buffers on its first call"
    cases.same_bits(e.mesh_project(K, R, Cc, [c.cams[0][3:]])[0][0], cases.twin(c)[0][0], "after failed allocations")
    e.mesh_release()
    assert live() == start
    e.mesh_set(c.V, c.F); e.mesh_visibility(K, R, Cc, [c.cams[0][3:]], len(c.V))
    e.close()
    assert live() == start


@pytest.mark.parametrize("order", ["reverse"])
def test_kernel_results_do_not_depend_on_the_execution_order(order):
    """Every kernel case again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER, as tests/test_emu_kernels.py does)."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_kernel_ and not execution_order"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPEMU_ORDER=order), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


# ---- the route: --mesh-file ----------------------------------------------------------------------------------------------------------------------------------
def test_mesh_file_replaces_the_sparse_cloud_before_view_selection(emulated, tmp_path):
    e = emulated()
    try:
        cases.mesh_file_case(e, SCENE, tmp_path)
        cases.dense_reconstruction_case(e, SCENE, tmp_path, light=True)
    finally:
        e.close()
