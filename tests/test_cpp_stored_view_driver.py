"""include/DenseDepthMapsHIP.hpp fed with decoded 8-bit images (View::image8): a C++ host that has no working-resolution image of its own -- the engine's image store
resizes and converts -- computes the depth maps and the coloured cloud that the Python host route (numpy resize and gray, uploaded) computes.  The program links the
emulated library in the CPU suite and the device library in the GPU suite."""
import os
import subprocess

import numpy as np
import pytest

from openmvs_amd import densify, patchmatch, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL, MIN_RES, MAX_RES = 1, 40, 3200


def _build(tmp, lib, hip):
    exe = os.path.join(tmp, "stored_view_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stored_view_driver.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + os.path.dirname(lib)] + (["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []))
    return exe


def _both_routes(tmp_path, sc, exe, new_engine, seed=31):
    n, ns = sc.n_views, sc.neighbors.shape[1]
    rgb = [np.ascontiguousarray(np.repeat(np.repeat(sc.bgr[i][..., ::-1], 2, 0), 2, 1)) for i in range(n)]        # decoded images at twice the working size
    H0, W0 = rgb[0].shape[:2]
    res, _ = views.compute_max_resolution(W0, H0, LEVEL, MIN_RES, MAX_RES)
    w, h = views.resized_size(W0, H0, res)
    assert (w, h) == (sc.width, sc.height)
    inp, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n, W0, H0, ns, LEVEL, MIN_RES, MAX_RES], np.int32).tobytes())
        for i in range(n):
            f.write(rgb[i].tobytes())
            f.write(np.concatenate([sc.K[i].ravel(), sc.R[i].ravel(), sc.C[i].ravel()]).astype(np.float64).tobytes())
            f.write(np.array([sc.dmin[i], sc.dmax[i]], np.float32).tobytes()); f.write(np.ascontiguousarray(sc.neighbors[i], np.int32).tobytes())
    subprocess.check_call([exe, str(inp), str(out), str(seed)])
    raw = open(out, "rb").read()
    assert tuple(np.frombuffer(raw[:8], np.int32)) == (w, h)
    P = w * h
    maps = np.frombuffer(raw[8:8 + n * P * 5 * 4], np.float32).reshape(n, 5 * P)
    nP = int(np.frombuffer(raw[8 + n * P * 20:16 + n * P * 20], np.uint64)[0])
    pts = np.frombuffer(raw[16 + n * P * 20:16 + n * P * 20 + 12 * nP], np.float32).reshape(nP, 3)
    col = np.frombuffer(raw[16 + n * P * 20 + 12 * nP:], np.uint8).reshape(nP, 3)
    # the Python host route: numpy resize and gray, uploaded images, the same schedule
    small = [densify._resize_area_u8(r, w, h) for r in rgb]
    e = new_engine()
    try:
        e.scene_create(n, w, h, 1)
        for i in range(n):
            e.scene_set_view(i, views.to_gray(small[i]), sc.K[i], sc.R[i], sc.C[i], float(sc.dmin[i]), float(sc.dmax[i]), sc.neighbors[i])
        p = patchmatch.default_params(seed=seed, nSubResolutionLevels=1, nEstimationIters=2, nEstimationGeometricIters=1)
        ids = list(range(n))
        e.Init(False)
        for v in ids:
            e.scene_reset_view(v)
        e.scene_estimate(ids, -1, p); e.scene_commit_round(); e.Init(True); e.scene_estimate(ids, 0, p)
        for v in ids:
            d, nr, c = e.scene_get_maps(v)
            assert np.array_equal(maps[v][:P].reshape(h, w), d) and np.array_equal(maps[v][P:4 * P].reshape(h, w, 3), nr) and np.array_equal(maps[v][4 * P:].reshape(h, w), c), v
            assert (d > 0).mean() > 0.5
        for i in range(n):
            e.scene_set_color(i, np.ascontiguousarray(small[i][..., ::-1]))
        order = sorted(ids, key=lambda i: (-len(sc.neighbors[i]), i))
        cloud = e.scene_fuse(order, 2, 0.01, 25.0, True, True)
        assert nP == cloud["nPoints"] > 0 and np.array_equal(pts, cloud["points"]) and np.array_equal(col, cloud["colors"])
    finally:
        e.close()


def test_stored_view_driver_under_the_emulator(tmp_path):
    from openmvs_amd import synth
    from tests import emu
    sc = synth.make_scene(3, 64, 48, n_src=2)
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as lib:
        exe = _build(str(tmp_path), lib, hip=False)
        _both_routes(tmp_path, sc, exe, lambda: patchmatch.PatchMatchHIP(0))


@pytest.mark.gpu
def test_stored_view_driver_on_the_device(tmp_path, small_scene):
    from openmvs_amd import build
    exe = _build(str(tmp_path), build.build_lib("libpmhip.so"), hip=True)
    _both_routes(tmp_path, small_scene, exe, lambda: patchmatch.PatchMatchHIP(0))
