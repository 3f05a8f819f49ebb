"""include/DenseDepthMapsHIP.hpp::FinishPointCloud with OptDenseHIP.hpp's mapping of --estimate-colors 1 / --estimate-normals 1: a C++ host estimates, fuses and
finishes a small scene without Python in the loop (tests/cpp/cloud_driver.cpp); the crop order, the colours and the orientation of the normals are checked
against tests/cloud_cases.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from openmvs_amd import build
    lib = build.build_lib("libpmhip.so")
    front = build.build_host_lib("libmvsfront.so")
    exe = os.path.join(tmp, "cloud_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cloud_driver.cpp"),
                           "-o", exe, lib, front, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_cloud_driver_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    assert subprocess.run([exe]).returncode == 2          # usage error path, no GPU touched


def _read(raw, off, colors):
    nP, nV = (int(x) for x in np.frombuffer(raw[off:off + 16].tobytes(), np.uint64)); off += 16
    c = {"nPoints": nP}
    c["points"] = np.frombuffer(raw[off:off + 12 * nP].tobytes(), np.float32).reshape(nP, 3); off += 12 * nP
    c["viewStart"] = np.frombuffer(raw[off:off + 4 * (nP + 1)].tobytes(), np.uint32); off += 4 * (nP + 1)
    c["views"] = np.frombuffer(raw[off:off + 4 * nV].tobytes(), np.uint32); off += 4 * nV
    if colors:
        c["colors"] = raw[off:off + 3 * nP].reshape(nP, 3); off += 3 * nP
        c["normals"] = np.frombuffer(raw[off:off + 12 * nP].tobytes(), np.float32).reshape(nP, 3); off += 12 * nP
    return c, off


@pytest.mark.gpu
def test_cloud_driver_finishes_the_fused_cloud(tmp_path, small_scene):
    from tests import cloud_cases as cc
    sc = small_scene
    exe = _build(str(tmp_path))
    inp = tmp_path / "scene.bin"; out = tmp_path / "out.bin"; obb = tmp_path / "obb.bin"
    n, w, h, ns = sc.n_views, sc.width, sc.height, sc.neighbors.shape[1]
    with open(inp, "wb") as f:
        f.write(np.array([n, w, h, ns], np.int32).tobytes())
        for i in range(n):
            f.write(np.ascontiguousarray(sc.gray[i], np.float32).tobytes()); f.write(np.ascontiguousarray(sc.bgr[i], np.uint8).tobytes())
            f.write(np.concatenate([sc.K[i].ravel(), sc.R[i].ravel(), sc.C[i].ravel()]).astype(np.float64).tobytes())
            f.write(np.array([sc.dmin[i], sc.dmax[i]], np.float32).tobytes()); f.write(np.ascontiguousarray(sc.neighbors[i], np.int32).tobytes())
    # an OBB around the middle of the ground-truth surface of view 0, enlarged by 10 % (fBorderROI 1.1)
    gt = sc.gt_depth[0]
    ys, xs = np.mgrid[0:h, 0:w]
    ray = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3).astype(np.float64) @ np.linalg.inv(sc.K[0]).T
    X = (ray * gt.reshape(-1, 1)) @ sc.R[0] + sc.C[0]
    lo, hi = np.percentile(X, 25, axis=0), np.percentile(X, 75, axis=0)
    rot = np.eye(3, dtype=np.float32); pos = ((lo + hi) / 2).astype(np.float32); ext = ((hi - lo) / 2).astype(np.float32)
    np.concatenate([rot.ravel(), pos, ext, [1.1]]).astype(np.float32).tofile(obb)
    subprocess.check_call([exe, str(inp), str(out), str(obb), "31"])
    raw = np.fromfile(out, np.uint8)
    fused, off = _read(raw, 0, False)
    fin, off = _read(raw, off, True)
    assert off == len(raw) and fused["nPoints"] > 1000
    r2, p2, e2 = cc.obb_enlarged(rot, pos, ext, 1.1)
    want = cc.crop_reference(dict(fused, weights=None, projs=None), cc.obb_inside(fused["points"], r2, p2, e2))
    assert 0 < fin["nPoints"] == want["nPoints"] < fused["nPoints"]
    for k in ("points", "viewStart", "views"):
        assert np.array_equal(fin[k], want[k]), k
    Ps = [cc.compose_P(sc.K[i], sc.R[i], sc.C[i]) for i in range(n)]
    assert np.array_equal(fin["colors"], cc.colors_reference(fin, Ps, list(sc.bgr)))
    first = fin["views"][fin["viewStart"][:-1].astype(np.int64)]
    _, dot = cc.orient(fin["normals"], fin["points"], sc.C[first].astype(np.float32))
    assert (dot >= 0).all() and np.allclose(np.linalg.norm(fin["normals"], axis=1), 1, atol=1e-5)
