"""pmhip_scene_cloud_filter on the MI355X: the device against the emulated engine bit for bit on a 50 000-point cloud, and the fused cloud of 9 x 1920x1080
views (more than a million points) with 2 % of its points turned into floaters, filtered where it lies: a sample of the votes against the restatement
summed over all cones, the removal in full against the literal swap-remove loop."""
import time

import numpy as np
import pytest

from openmvs_amd import patchmatch, synth
from tests import cloud_cases as cc
from tests import cloud_filter_cases as fc
from tests import emu

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("points", "viewStart", "views", "weights", "colors", "normals")


def test_device_equals_emulator_on_50k_points():
    sc = synth.make_scene(7, 640, 480, n_src=6)
    cl = cc.random_cloud(sc, 50000, seed=31)
    cl, _ = fc.move_along_first_ray(cl, sc.C, 0.08, seed=8)
    cl = fc.with_attributes(cl, seed=9)

    def run():
        e = patchmatch.PatchMatchHIP(0)
        e.scene_load(sc, n_levels=0)
        e.scene_cloud_load(cl["points"], cl["viewStart"], cl["views"], cl["weights"], cl["colors"], cl["normals"])
        r = e.scene_cloud_filter(th_remove=-1, min_views=2)
        e.close()
        return r

    dev = run()
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        host = run()
    print("\n50k: %d -> %d points, %d votes non-zero; device steps %s" % (cl["nPoints"], dev["nPoints"], (dev["visibility"] != 0).sum(), {k: round(v, 2) for k, v in dev["times"].items()}))
    assert 1000 < dev["nPoints"] == host["nPoints"] < cl["nPoints"] and (host["visibility"] != 0).sum() > 1000
    assert np.array_equal(dev["visibility"], host["visibility"]) and np.array_equal(dev["cones"], host["cones"])
    for k in FIELDS:
        assert np.array_equal(dev[k], host[k]), k


def test_device_cloud_filter_1080p():
    from tests.test_zz_gpu_cloud_finish import _fused_1080p
    sc, e, fused = _fused_1080p()
    assert fused["nPoints"] > 1_000_000
    fin = e.scene_cloud_finish(estimate_colors=True, estimate_normals=True)
    assert fin["colors"] is not None and fin["normals"] is not None
    cl, moved = fc.move_along_first_ray(fin, sc.C, 0.02, seed=10)
    n = cl["nPoints"]
    nv = np.diff(cl["viewStart"].astype(np.int64))
    print("\n1080p: %d points, %d cones (%.2f views per point), %d moved" % (n, len(cl["views"]), nv.mean(), len(moved)))

    def run():
        e.scene_cloud_load(cl["points"], cl["viewStart"], cl["views"], cl["weights"], cl["colors"], cl["normals"])
        t = time.time()
        r = e.scene_cloud_filter(th_remove=-1)
        return r, time.time() - t

    got, dt = run()
    vis = got["visibility"]
    flagged = int((vis <= -1).sum())
    print("filter: %d -> %d points (%d flagged, %d votes non-zero: %d negative, %d positive), %.0f ms incl. download; steps %s" %
          (n, got["nPoints"], flagged, (vis != 0).sum(), (vis < 0).sum(), (vis > 0).sum(), dt * 1e3, {k: round(v, 2) for k, v in got["times"].items()}))
    assert 1000 < flagged < n // 2
    ang, c2 = fc.cone_constants(sc.K, [1920] * sc.n_views)
    assert np.array_equal(got["cones"][:, 0], ang)
    assert (np.abs(got["cones"][:, 1].astype(np.float64) - c2) <= np.spacing(c2.astype(F)).astype(np.float64)).all()
    # a seeded sample of targets, half from the device's non-zero votes, half uniform, against the sum over all cones; enlarged until 100 reference votes are non-zero
    rng = np.random.default_rng(11)
    nz = np.nonzero(vis)[0]
    tg = np.zeros(0, np.int64); ref = np.zeros(0, np.int32)
    for attempt in range(4):
        more = np.concatenate([rng.choice(nz, 100, replace=False), rng.choice(n, 100, replace=False)]).astype(np.int64)
        more = np.setdiff1d(more, tg)
        t = time.time()
        ref = np.concatenate([ref, fc.visibility_sampled(cl, sc.C, got["cones"][:, 0], got["cones"][:, 1], more)]); tg = np.concatenate([tg, more])
        print("sample of %d targets: %d reference votes non-zero (%.0f s)" % (len(tg), (ref != 0).sum(), time.time() - t))
        if len(tg) >= 200 and (ref != 0).sum() >= 100:
            break
    assert len(tg) >= 200 and (ref != 0).sum() >= 100
    assert np.array_equal(vis[tg], ref)
    # the removal, exactly and in full, from the device's own votes
    want = cc.crop_reference(cl, vis > -1)
    assert got["nPoints"] == want["nPoints"] == n - flagged
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), k
    again, _ = run()
    assert np.array_equal(again["visibility"], vis)
    for k in FIELDS:
        assert np.array_equal(again[k], got[k]), k
    e.close()
