"""A C++ host on the device seed route (tests/cpp/seed_view_driver.cpp): mvsf_point_mesh (libmvsfront.so) -> MVS::PatchMatchHIP::SeedView -> pmhip_scene_estimate on
tests/data/scene gives the seed maps, the depth range and the estimated maps of the Python device route (`densify.load_scene(seed_on_device=True)` +
`PatchMatchHIP.scene_seed_view` + `scene_estimate`), bit for bit, with the 2x2 splats and with the faces rasterised.  The program links the emulated library in the CPU
suite (at 80 x 60) and the device library in the GPU suite (at 320 x 240)."""
import os
import subprocess

import numpy as np
import pytest

from openmvs_amd import build, densify, patchmatch
from tests import seed_raster_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp, lib, hip):
    exe = os.path.join(tmp, "seed_view_driver")
    front = build.build_host_lib("libmvsfront.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "seed_view_driver.cpp"), "-o", exe, lib, front,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.dirname(front)] + (["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []))
    return exe


def _run(tmp_path, exe, new_engine, level, min_resolution, size, sparse):
    from openmvs_amd import mvsi, views
    opt = cases._opt(level, min_resolution, sparse)
    sv = densify.load_scene(cases.SCENE, opt=opt, seed_on_device=True)
    assert (sv.width, sv.height) == size and sv.ids[0] == 0 and not sv.alias_of
    w, h = size
    n, levels, iters, seed = len(sv.gray), 1, 2, 5
    mode, proj, vz, normals, faces = sv.seed_mesh[0]
    sc = mvsi.load(cases.SCENE)
    points = views.select_views(sc, views.Cameras(sc, sv.sizes), 0, opt.dense_options())[1].astype(np.uint32)
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"
    with open(job, "wb") as f:
        f.write(np.array([n, w, h, levels, iters, seed, mode, len(points)], np.int32).tobytes())
        for i in range(n):
            f.write(np.concatenate([np.ravel(sv.K[i]), np.ravel(sv.R[i]), np.ravel(sv.C[i])]).astype(np.float64).tobytes())
            f.write(np.array([sv.dmin[i], sv.dmax[i]], f32).tobytes())
            nb = np.ascontiguousarray(sv.neighbors[i], np.int32)
            f.write(np.array([len(nb)], np.int32).tobytes()); f.write(nb.tobytes()); f.write(np.ascontiguousarray(sv.gray[i], f32).tobytes())
        f.write(points.tobytes())
    subprocess.check_call([exe, cases.SCENE, str(job), str(out)])
    raw = np.frombuffer(open(out, "rb").read(), f32)
    P = w * h
    assert raw.size == 2 + 4 * P + 5 * P
    assert float(raw[0]) == float(f32(sv.dmin[0])) and float(raw[1]) == float(f32(sv.dmax[0]))
    e = new_engine()
    try:
        e.scene_load(sv, n_levels=levels)
        e.scene_seed_view(0, mode, proj, vz, normals, faces)
        d, nm, _ = e.scene_get_maps(0)
        assert (d > 0).mean() > (0.001 if sparse else 0.3)
        cases.same_bits(raw[2:2 + P].reshape(h, w), d, "seed depth"); cases.same_bits(raw[2 + P:2 + 4 * P].reshape(h, w, 3), nm, "seed normals")
        e.Init(False)
        e.scene_estimate([0], -1, patchmatch.default_params(nSubResolutionLevels=levels, nEstimationIters=iters, seed=seed))
        at = 2 + 4 * P
        for got, want, what in zip((raw[at:at + P].reshape(h, w), raw[at + P:at + 4 * P].reshape(h, w, 3), raw[at + 4 * P:].reshape(h, w)), e.scene_get_maps(0), ("depth", "normal", "confidence")):
            cases.same_bits(got, want, "estimated " + what)
        assert (e.scene_get_maps(0)[0] > 0).mean() > 0.3
    finally:
        e.close()


@pytest.mark.parametrize("sparse", [True, False], ids=["points", "faces"])
def test_seed_view_driver_under_the_emulator(tmp_path, sparse):
    from tests import emu
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as lib:
        _run(tmp_path, _build(str(tmp_path), lib, hip=False), lambda: patchmatch.PatchMatchHIP(0), 3, 40, (80, 60), sparse)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [True, False], ids=["points", "faces"])
def test_seed_view_driver_on_the_device(tmp_path, sparse):
    _run(tmp_path, _build(str(tmp_path), build.build_lib("libpmhip.so"), hip=True), lambda: patchmatch.PatchMatchHIP(0), 1, 160, (320, 240), sparse)
