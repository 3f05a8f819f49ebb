"""pmhip_scene_cloud_finish on the MI355X: the fused cloud of 9 x 1920x1080 views (more than a million points) cropped, coloured and given PCA normals
where fusion left it, against the restatements of tests/cloud_cases.py; the device against the emulated engine on a small cloud."""
import time

import numpy as np
import pytest

from openmvs_amd import patchmatch, synth
from openmvs_amd.patchmatch import PatchMatchHIP
from oracle import pyoracle as po
from tests import cloud_cases as cc
from tests import emu
from tests import fuse_cases as fc

pytestmark = pytest.mark.gpu

F = np.float32


def _fused_1080p():
    sc = synth.make_scene(9, 1920, 1080, n_src=8, device="cuda")
    maps = fc.make_maps(sc, seed=7)
    e = PatchMatchHIP(0)
    e.scene_load(sc, n_levels=0)
    d, n, c = maps
    for v in range(sc.n_views):
        e.scene_set_maps(v, d[v], n[v]); e.scene_set_conf(v, c[v]); e.scene_set_color(v, sc.bgr[v])
    cloud = e.scene_fuse(po.fuse_order([len(x) for x in sc.neighbors]), bEstimateColor=False, bEstimateNormal=False)
    return sc, e, cloud


def test_device_cloud_finish_1080p():
    sc, e, fused = _fused_1080p()
    assert fused["nPoints"] > 1_000_000
    pts = fused["points"]
    lo, hi = np.percentile(pts, 3, axis=0), np.percentile(pts, 97, axis=0)
    ang = 0.2
    rot = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], F)
    pos = ((lo + hi) * 0.5).astype(F); ext = ((hi - lo) * 0.5).astype(F)
    e.scene_cloud_finish()                                              # (nothing to do: a no-op)
    t = time.time()
    got = e.scene_cloud_finish(crop_obb=(rot, pos, ext), border_roi=0.0, estimate_colors=True, estimate_normals=True)
    dt = time.time() - t
    # crop: the swap-remove order, exactly
    keep = cc.obb_inside(pts, rot, pos, ext)
    want = cc.crop_reference(fused, keep)
    assert 0 < got["nPoints"] < fused["nPoints"]
    for k in ("points", "viewStart", "views", "weights", "projs"):
        assert np.array_equal(got[k], want[k]), k
    # colours: bit-exact
    Ps = [cc.compose_P(sc.K[i], sc.R[i], sc.C[i]) for i in range(sc.n_views)]
    assert np.array_equal(got["colors"], cc.colors_reference(want, Ps, list(sc.bgr)))
    # neighbours of a 20 k sample against cKDTree, normals within tolerance and oriented
    n = got["nPoints"]
    q = np.sort(np.random.default_rng(1).choice(n, 20000, replace=False)).astype(np.uint32)
    nb = e.scene_cloud_knn(q, 16)
    ref, d = cc.knn_reference(got["points"], q, 16)
    ref = cc.knn_tie_order(got["points"], q, ref)
    distinct = d[:, 15] < d[:, 16]
    assert distinct.mean() > 0.9 and np.array_equal(nb[distinct], ref[distinct])
    first = got["views"][got["viewStart"][:-1].astype(np.int64)]
    cf = sc.C[first].astype(F)
    rn, lam = cc.pca_normals(got["points"], nb.astype(np.int64), cf[q])
    rn, _ = cc.orient(rn, got["points"][q], cf[q])
    _, dot = cc.orient(got["normals"][q], got["points"][q], cf[q])
    assert (dot >= 0).all()
    ok = (lam[:, 1] - lam[:, 0]) > 1e-3 * lam[:, 2]
    a = cc.angle(got["normals"][q], rn)
    assert ok.mean() > 0.9 and a[ok].max() < 1e-5
    print("\ncloud finish 9x1080p: %d -> %d points, %.0f ms incl. download; steps %s" %
          (fused["nPoints"], n, dt * 1e3, {k: round(v, 2) for k, v in got["times"].items()}))
    # against the synthetic surface: fuse noise-free maps (the perturbed ones carry depth noise far above the point spacing at k = 16) and compare
    # with the ground-truth normal at the pixel of each point's first view
    d, nrm, c = fc.make_maps(sc, seed=8, outlier=0.0, tilt=0.0, noise=0.0)
    for v in range(sc.n_views):
        e.scene_set_maps(v, d[v], nrm[v]); e.scene_set_conf(v, c[v])
    e.scene_fuse(po.fuse_order([len(x) for x in sc.neighbors]), bEstimateColor=False, bEstimateNormal=False)
    clean = e.scene_cloud_finish(estimate_normals=True)
    first = clean["views"][clean["viewStart"][:-1].astype(np.int64)]
    xy = clean["projs"][clean["viewStart"][:-1].astype(np.int64)]
    gt = np.zeros((clean["nPoints"], 3))
    for v in np.unique(first):
        m = first == v
        gt[m] = fc.normals_from_depth(sc.gt_depth[v], sc.K[v])[xy[m, 1], xy[m, 0]].astype(np.float64) @ sc.R[v]
    gang = np.degrees(cc.angle(clean["normals"], gt))
    print("noise-free maps: %d points, median angle of the PCA normal to the ground-truth normal %.3f deg (90th percentile %.3f)" %
          (clean["nPoints"], float(np.median(gang)), float(np.percentile(gang, 90))))
    assert np.median(gang) < 2.0
    e.close()


def test_device_equals_emulator_on_a_small_cloud():
    sc = synth.make_scene(5, 160, 120, n_src=4)
    cl = cc.random_cloud(sc, 8000, seed=21, jitter=1e-3)
    rot = np.eye(3, dtype=F); pos = np.median(cl["points"], axis=0).astype(F); ext = (np.ptp(cl["points"], axis=0) * 0.4).astype(F)

    def run():
        e = patchmatch.PatchMatchHIP(0)
        e.scene_load(sc, n_levels=0)
        for v in range(sc.n_views):
            e.scene_set_color(v, sc.bgr[v])
        e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"], cl["weights"])
        r = e.scene_cloud_finish(crop_obb=(rot, pos, ext), border_roi=-0.01, estimate_colors=True, estimate_normals=True)
        r["knn"] = e.scene_cloud_knn(np.arange(r["nPoints"], dtype=np.uint32), 16)
        e.close()
        return r

    dev = run()
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        host = run()
    assert dev["nPoints"] == host["nPoints"] > 1000
    for k in ("points", "viewStart", "views", "weights", "colors", "normals", "knn"):
        assert np.array_equal(dev[k], host[k]), k
