"""include/DenseDepthMapsHIP.hpp::FilterPointCloud: a C++ host estimates, fuses, finishes and filters a small scene without Python in the loop
(tests/cpp/cloud_filter_driver.cpp); the result equals the Python path on the same cloud, and the removal the literal swap-remove loop."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from openmvs_amd import build
    lib = build.build_lib("libpmhip.so")
    front = build.build_host_lib("libmvsfront.so")
    exe = os.path.join(tmp, "cloud_filter_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cloud_filter_driver.cpp"),
                           "-o", exe, lib, front, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_cloud_filter_driver_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    assert subprocess.run([exe]).returncode == 2          # usage error path, no GPU touched


def _read(raw, off):
    nP, nV = (int(x) for x in np.frombuffer(raw[off:off + 16].tobytes(), np.uint64)); off += 16
    c = {"nPoints": nP}
    for k, dt, n, shape in (("points", np.float32, 3 * nP, (nP, 3)), ("viewStart", np.uint32, nP + 1, (nP + 1,)), ("views", np.uint32, nV, (nV,)),
                            ("weights", np.float32, nV, (nV,)), ("colors", np.uint8, 3 * nP, (nP, 3)), ("normals", np.float32, 3 * nP, (nP, 3))):
        size = n * np.dtype(dt).itemsize
        c[k] = np.frombuffer(raw[off:off + size].tobytes(), dt).reshape(shape); off += size
    return c, off


@pytest.mark.gpu
def test_cloud_filter_driver_equals_the_python_path(tmp_path, small_scene):
    from openmvs_amd import patchmatch
    from tests import cloud_cases as cc
    from tests import cloud_filter_cases as fc
    sc = small_scene
    exe = _build(str(tmp_path))
    inp = tmp_path / "scene.bin"; out = tmp_path / "out.bin"
    n, w, h, ns = sc.n_views, sc.width, sc.height, sc.neighbors.shape[1]
    with open(inp, "wb") as f:
        f.write(np.array([n, w, h, ns], np.int32).tobytes())
        for i in range(n):
            f.write(np.ascontiguousarray(sc.gray[i], np.float32).tobytes()); f.write(np.ascontiguousarray(sc.bgr[i], np.uint8).tobytes())
            f.write(np.concatenate([sc.K[i].ravel(), sc.R[i].ravel(), sc.C[i].ravel()]).astype(np.float64).tobytes())
            f.write(np.array([sc.dmin[i], sc.dmax[i]], np.float32).tobytes()); f.write(np.ascontiguousarray(sc.neighbors[i], np.int32).tobytes())
    th, min_views = -1, 3
    subprocess.check_call([exe, str(inp), str(out), str(th), str(min_views), "31"])
    raw = np.fromfile(out, np.uint8)
    fin, off = _read(raw, 0)
    flt, off = _read(raw, off)
    nvis = int(np.frombuffer(raw[off:off + 8].tobytes(), np.uint64)[0]); off += 8
    vis = np.frombuffer(raw[off:off + 4 * nvis].tobytes(), np.int32); off += 4 * nvis
    assert off == len(raw) and fin["nPoints"] > 1000
    # the Python path on the same cloud, the scene's cameras
    e = patchmatch.PatchMatchHIP(0)
    e.scene_load(sc, n_levels=0)
    e.scene_cloud_load(fin["points"], fin["viewStart"], fin["views"], fin["weights"], fin["colors"], fin["normals"])
    py = e.scene_cloud_filter(th_remove=th, min_views=min_views)
    e.close()
    ang, c2 = fc.cone_constants(sc.K, [w] * n)
    assert np.array_equal(py["cones"][:, 0], ang)
    base = fc.remove_min_views(fin, min_views)
    print("\n%d finished, %d after min_views %d, %d votes non-zero, %d after the filter" % (fin["nPoints"], base["nPoints"], min_views, (vis != 0).sum(), flt["nPoints"]))
    assert 0 < base["nPoints"] < fin["nPoints"] and nvis == base["nPoints"]
    assert np.array_equal(vis, py["visibility"])
    want = cc.crop_reference(base, vis > th)
    for k in ("points", "viewStart", "views", "weights", "colors", "normals"):
        assert np.array_equal(flt[k], py[k]), k
        assert np.array_equal(flt[k], want[k]), k
    # a sample of the votes against the restatement over all cones
    rng = np.random.default_rng(5)
    nz = np.nonzero(vis)[0]
    tg = np.unique(np.concatenate([rng.choice(nz, min(100, len(nz)), replace=False), rng.choice(nvis, 100, replace=False)]).astype(np.int64))
    assert np.array_equal(fc.visibility_sampled(base, sc.C, py["cones"][:, 0], py["cones"][:, 1], tg), vis[tg])
