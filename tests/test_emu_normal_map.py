"""MVS::EstimateNormalMap of csrc/pm_normal.hip on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py), both entry points
(pmhip_estimate_normal_map, pmhip_scene_estimate_normals) on the cases of tests/normal_map_cases.py against `views.estimate_normal_map`, bit for bit; the kernel cases again
with lanes and workgroups executed in reverse; then the two routes that use it: the resume of a .dmap stored without normals and `--fusion-mode -2` through to the cloud
(SGM steps from the oracle backend, the PatchMatch engine emulated).  The cases are those of tests/test_zz_gpu_normal_map.py; the grid-stride case runs on the device only."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import patchmatch
from tests import emu
from tests import normal_map_cases as cases

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


def test_the_emulated_library_exports_both_entry_points(emulated):
    import ctypes as C
    import re
    lib = patchmatch.load_library()
    assert hasattr(lib, "pmhip_estimate_normal_map") and hasattr(lib, "pmhip_scene_estimate_normals") and hasattr(lib, "hipemu_counters")
    # include/pmhip_normals.h, the companion header pmhip.h includes: every name it declares has a parsed signature, set on the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pmhip_normals.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(pmhip_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted(patchmatch.NORMALS_EXPORTS) == ["pmhip_estimate_normal_map", "pmhip_scene_estimate_normals"]
    assert '#include "pmhip_normals.h"' in open(os.path.join(root, "include", "pmhip.h")).read()
    assert len(lib.pmhip_estimate_normal_map.argtypes) == 6 and lib.pmhip_estimate_normal_map.argtypes[3] is C.c_int and lib.pmhip_estimate_normal_map.restype is C.c_int
    assert len(lib.pmhip_scene_estimate_normals.argtypes) == 3 and lib.pmhip_scene_estimate_normals.argtypes[0] is C.c_void_p


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("order", ["reverse"])
def test_kernel_results_do_not_depend_on_the_execution_order(order):
    """Every kernel case again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER, as tests/test_emu_kernels.py does): each
    output has one writer, so the bits must not move."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_kernel_ and not execution_order"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPEMU_ORDER=order), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


# ---- the routes ----------------------------------------------------------------------------------------------------------------------------------------------
def test_resume_of_a_dmap_without_normals_estimates_them_on_the_engine(emulated, tmp_path, monkeypatch):
    e = emulated()
    try:
        cases.resume_case(e, tmp_path / "device", monkeypatch)
    finally:
        e.close()
    _stand_in_engine_gets_host_normals(tmp_path / "host")


def _stand_in_engine_gets_host_normals(tmp_path):
    """The sharded driver's stand-in engines answer every name: the resume then computes the normals on the host and installs them with the depth."""
    import numpy as np
    from openmvs_amd import densify, dmap, synth, views
    from openmvs_amd.patchmatch import PMHipParams

    class StandIn:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append((name,) + a)

    sc = synth.make_scene(2, 32, 24, n_src=1)
    sc.sizes = [(32, 24)] * 2
    depth = cases.surface(np.random.default_rng(22), 24, 32)
    os.makedirs(str(tmp_path))
    for v in range(2):
        dmap.save(os.path.join(str(tmp_path), dmap.depth_file_name(v)), "x.jpg", [v, 1 - v], (32, 24), sc.K[v], sc.R[v], sc.C[v], 1.0, 9.0, depth, None, np.ones((24, 32), np.float32))
    s = StandIn()
    p = PMHipParams(); p.nEstimationGeometricIters = 0
    assert densify.compute_depth_maps(s, [0, 1], p, n_optimize=0, scene=sc, dmap_dir=str(tmp_path)) == [0, 1]
    assert "scene_estimate_normals" not in [c[0] for c in s.calls]
    got = [c for c in s.calls if c[0] == "scene_set_maps"]
    assert len(got) == 2 and all(np.array_equal(c[3], views.estimate_normal_map(sc.K[c[1]], depth)) for c in got)


def test_mode_minus_2_through_to_the_cloud(emulated, tmp_path):
    from tests.tsgm_backends import OracleBackend
    be = OracleBackend()
    be.e = emulated()
    try:
        cases.mode2_case(be, SCENE, tmp_path)
    finally:
        be.e.close()


def test_mvs_out_needs_mode_minus_2_and_an_engine(tmp_path):
    from openmvs_amd import sgm_pipeline
    from tests.tsgm_backends import OracleBackend
    with pytest.raises(ValueError, match="-2"):
        sgm_pipeline.dense_reconstruction(OracleBackend(), SCENE, str(tmp_path), -1, cases.mode2_options(), mvs_out=str(tmp_path / "x.mvs"))
    with pytest.raises(ValueError, match="PatchMatch engine"):
        sgm_pipeline.dense_reconstruction(OracleBackend(), SCENE, str(tmp_path), -2, cases.mode2_options(), mvs_out=str(tmp_path / "x.mvs"))
