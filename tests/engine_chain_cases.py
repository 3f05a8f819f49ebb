"""The whole chain of the PatchMatch engine on one small scene -- create, views, masks, colours, estimate (photometric + one geometric round), filter + commit,
gap interpolation, small segments, fusion with colours and normals, cloud finish with a crop, cloud filter -- and every output on the way.  Shared by the
tests of the engine's memory (tests/test_engine_memory.py) and of its reuse across scenes (tests/test_engine_reuse.py on the emulator,
tests/test_zz_gpu_engine_reuse.py on the device)."""
import numpy as np

from openmvs_amd import patchmatch, synth
from oracle import pyoracle as po

LEVELS = 2


def make_case(n_views, w, h, own=None):
    """A synthetic scene of n_views views of w x h; own = (view, w2, h2): that view carries its own image size (the same camera rendered at w2 x h2)."""
    sc = synth.make_scene(n_views, w, h, n_src=min(4, n_views - 1))
    case = dict(scene=sc, own={})
    if own is not None:
        v, w2, h2 = own
        small = synth.make_scene(n_views, w2, h2, n_src=min(4, n_views - 1))
        case["own"][v] = (small.gray[v], small.K[v], small.bgr[v])
    return case


def _mask(w, h):
    m = np.ones((h, w), np.uint8)
    m[: h // 4, : w // 3] = 0
    return m


def load(e, case):
    sc = case["scene"]
    e.Init(True)
    e.scene_create(sc.n_views, sc.width, sc.height, LEVELS)
    for i in range(sc.n_views):
        rest = (sc.R[i], sc.C[i], float(sc.dmin[i]), float(sc.dmax[i]), sc.neighbors[i])
        if i in case["own"]:
            e.scene_set_view_sized(i, case["own"][i][0], case["own"][i][1], *rest)
        else:
            e.scene_set_view(i, sc.gray[i], sc.K[i], *rest)
    for i in sorted({0} | set(case["own"])):                              # a mask in the scene's arrays and one in a view's own storage
        e.scene_set_mask(i, _mask(*e.view_size(i)))
    for i in range(sc.n_views):
        e.scene_set_color(i, case["own"][i][2] if i in case["own"] else sc.bgr[i])


def run_chain(e, case):
    """-> {name: array}: the depth, normal and confidence maps as estimated and as filtered, the fused cloud, the cropped one and the filtered one with its votes."""
    sc = case["scene"]
    ids = list(range(sc.n_views))
    load(e, case)
    p = patchmatch.default_params(nSubResolutionLevels=LEVELS, nEstimationIters=1, nRandomIters=2, nEstimationGeometricIters=1)
    e.scene_estimate(ids, -1, p)
    e.scene_commit_round()
    e.scene_estimate(ids, 0, p)
    out = {}

    def maps(tag):
        for i in ids:
            for name, a in zip(("depth", "normal", "conf"), e.scene_get_maps(i)):
                out["%s.%s.%d" % (tag, name, i)] = a

    def cloud(tag, c, extra=()):
        for k in ("points", "viewStart", "views", "weights", "projs", "colors", "normals") + tuple(extra):
            assert c[k] is not None, (tag, k)
            out["%s.%s" % (tag, k)] = c[k]

    maps("estimated")
    e.scene_filter(ids, commit=True)
    e.scene_gap_interpolation(ids)
    e.scene_remove_small_segments(ids, nSpeckleSize=20)
    maps("filtered")
    fused = e.scene_fuse(po.fuse_order([len(x) for x in sc.neighbors]), bEstimateColor=True, bEstimateNormal=True)
    assert fused["nPoints"] > 200, fused["nPoints"]
    cloud("fused", fused)
    lo, hi = np.percentile(fused["points"], 10, axis=0), np.percentile(fused["points"], 90, axis=0)
    box = (np.eye(3, dtype=np.float32), ((lo + hi) * 0.5).astype(np.float32), ((hi - lo) * 0.5).astype(np.float32))
    cropped = e.scene_cloud_finish(crop_obb=box, estimate_colors=True, estimate_normals=True)
    assert 0 < cropped["nPoints"] < fused["nPoints"]
    cloud("cropped", cropped)
    cloud("cloud_filtered", e.scene_cloud_filter(th_remove=-1, min_views=2), extra=("visibility",))
    return out


def same(got, want, what):
    """bit for bit: the same arrays, compared as bytes"""
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


def check_reuse():
    """One engine runs scene A, then the larger scene B with views of mixed sizes (a larger batch, fuse slab and cloud: every regrow path, the restart of the fusion's
    working buffers, the swap of the cloud's two buffer sets), then A again: every output equals, bit for bit, what a fresh engine gives for that scene alone."""
    cases = dict(A=make_case(4, 64, 48), B=make_case(5, 96, 80, own=(2, 80, 64)))
    fresh = {}
    for name, case in cases.items():
        e = patchmatch.PatchMatchHIP(0)
        fresh[name] = run_chain(e, case)
        e.close()
    e = patchmatch.PatchMatchHIP(0)
    for step, name in enumerate("ABA"):
        same(run_chain(e, cases[name]), fresh[name], "run %d (scene %s) on a reused engine" % (step, name))
    e.close()
