"""Cases for the speculative kernel pm_sweep_widen_kernel (csrc/pm_wide_n.hip: 16 or 32 lanes per pixel -- hypothesis slot x source view --, 4 or 2 pixels per wave) where
its lanes and workgroups meet edges: whatever a pixel's lanes exchange -- the smoothness factors inside a quad, the two-smallest reduction over the eight view lanes, the
group leaders' hypotheses and scores read by every lane -- and the XCD-aware workgroup -> (view, chunk) map must give the sequential sweep's maps whichever lanes, pixels
and workgroups are idle, so every case compares depth, normal and confidence bit for bit with the sequential oracle.  The cases were written for a candidate lane order
(a pixel's lanes PPW apart; measured and not taken: DESIGN.md 4.2) and hold for any order.  Run on the wave64 emulator by tests/test_emu_widen_lane_order.py and on the
device by tests/test_zz_gpu_widen_lane_order.py.

Shapes: nine views at 64x48 (ten for the nine-source case) with one sub-resolution level, i.e. levels of 64x48 and 32x24 whose inner anti-diagonals have every length
from 1 to 40 -- waves of four or two pixels and their quads occur partly filled at both ends.  The speculative kernel is forced with wideHyps = 2 or 4; each case runs
the photometric pass and one geometric round on top of it."""
import functools

import numpy as np

from openmvs_amd import synth
from openmvs_amd.patchmatch import default_params
from oracle import pyoracle as po
from tests.test_gpu_patchmatch import _same

W, H, REF, SEED = 64, 48, 4, 5

# (case, hypotheses per round)
CASES = [("src8", 2), ("src7", 2), ("src5", 2), ("src3", 2), ("src1", 2), ("src9", 2), ("mask", 2), ("own_size", 2), ("tiles8", 2),
         ("src8", 4), ("src3", 4), ("tiles8", 4), ("scene_groups", 2)]


@functools.lru_cache(maxsize=None)
def scene(n_views=9):
    return synth.make_scene(n_views, W, H, n_src=n_views - 1)


def _engine(hyps, **more):
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    want = dict(wideMaxViews=64, wideHyps=hyps, **more)
    got = e.tuning(**want)
    assert all(got[k] == v for k, v in want.items()), got
    return e


@functools.lru_cache(maxsize=None)
def _expected_rounds(n_views, nsrc, tile, masked=False, own=False):
    """Oracle maps of the photometric pass and of one geometric round on top of it (the sources' depth maps: the reference view's photometric map -- any maps do, both
    sides read the same, and plausible depths take the consistency branch)."""
    sc = scene(n_views)
    ref = REF if n_views == 9 else 5
    ids = [ref] + [int(i) for i in sc.neighbors[ref][:nsrc]]
    gray, K = _own_images(ids) if own else (sc.gray, sc.K)
    mask = _the_mask() if masked else None
    kw = dict(nSubResolutionLevels=1, nEstimationGeometricIters=1)
    if tile:
        kw.update(tileW=tile, tileH=tile)
    opt = po.default_opt(seed=SEED, viewID=ref, **kw)
    dmin, dmax = float(sc.dmin[ref]), float(sc.dmax[ref])
    views, keep = po.make_views(gray, K, sc.R, sc.C, ids)
    if masked:
        photo = po.estimate_depth_map_masked(views, len(ids), dmin, dmax, opt, mask, mask_mode=True)
        geo = None       # (the masked oracle entry runs the photometric pass)
    else:
        photo = po.estimate_depth_map(views, len(ids), dmin, dmax, opt)
        geo = None
        if not own:
            views, keep = po.make_views(gray, K, sc.R, sc.C, ids, depth_maps={i: photo[0] for i in ids[1:]})
            geo = po.estimate_depth_map(views, len(ids), dmin, dmax, opt, geo_iter=0, depth=photo[0], normal=photo[1])
    for a in tuple(photo) + tuple(geo or ()):
        a.setflags(write=False)
    return ref, ids, photo, geo


def _the_mask():
    """Ignored pixels inside quads and waves: single pixels scattered so that quads of neighbouring diagonal pixels lose one or two, and a whole anti-diagonal."""
    mask = np.full((H, W), 255, np.uint8)
    mask[::3, ::5] = 0
    mask[7::4, 9::7] = 0
    for y in range(6, 44):
        mask[y, 55 - y] = 0
    return mask


def _own_images(ids):
    """Two of the eight sources carry their own image size (0.75x and 1.25x): the batch reads its taps through each view's own pointer with clamped coordinates (BUF = false)."""
    base = scene()
    small = synth.make_scene(9, W * 3 // 4, H * 3 // 4, n_src=8)
    big = synth.make_scene(9, W * 5 // 4, H * 5 // 4, n_src=8)
    gray = {i: base.gray[i] for i in range(9)}; K = {i: base.K[i] for i in range(9)}
    gray[ids[2]] = small.gray[ids[2]]; K[ids[2]] = small.K[ids[2]]
    gray[ids[5]] = big.gray[ids[5]]; K[ids[5]] = big.K[ids[5]]
    return gray, K


def _both_rounds(hyps, n_views, nsrc, tile=0, masked=False, own=False):
    sc = scene(n_views)
    ref, ids, photo, geo = _expected_rounds(n_views, nsrc, tile, masked, own)
    what = "%d sources, %d hypotheses per round%s%s%s" % (nsrc, hyps, ", %dx%d tiles" % (tile, tile) if tile else "", ", ignore mask" if masked else "", ", own sizes" if own else "")
    gray, K = _own_images(ids) if own else (sc.gray, sc.K)
    mask = _the_mask() if masked else None
    e = _engine(hyps)
    try:
        if tile:
            e.set_sweep_tiles(tile, tile)
        p = default_params(seed=SEED, nSubResolutionLevels=1, nEstimationGeometricIters=1)
        e.Init(False)
        kw = dict(mask=mask) if masked else {}
        got = e.EstimateDepthMap(gray, K, sc.R, sc.C, ids, sc.dmin[ref], sc.dmax[ref], params=p, **kw)
        for a, b, name in zip(got, photo, ("depth", "normal", "conf")):
            _same(a, b, "%s: photometric %s" % (what, name))
        if masked:
            assert not got[0][mask == 0].any() and (got[0][mask != 0] > 0).mean() > 0.3
        else:
            assert (got[0] > 0).mean() > 0.3
        # one geometric round on top; where the oracle has no entry for the case's extra (mask, own sizes) the round runs on the plain scene with the same sources
        if geo is None:
            ref, ids, photo, geo = _expected_rounds(n_views, nsrc, tile)
        e.Init(True)
        got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[ref], sc.dmax[ref], depth=photo[0].copy(), normal=photo[1].copy(),
                                 src_depths={i: photo[0] for i in ids[1:]}, nGeometricIter=0, params=p)
        for a, b, name in zip(got, geo, ("depth", "normal", "conf")):
            _same(a, b, "%s: geometric %s" % (what, name))
        assert (got[0] != photo[0]).any()
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _scene_expected():
    """Five reference views of the nine-view scene, each against its eight neighbours: photometric pass, then one geometric round in which every view reads the
    photometric maps of its sources."""
    sc = scene()
    refs = [0, 2, 4, 6, 8]
    opt = lambda v: po.default_opt(seed=SEED, viewID=v, nSubResolutionLevels=1, nEstimationGeometricIters=1)
    photo = {}
    for v in range(sc.n_views):
        ids = [v] + [int(i) for i in sc.neighbors[v]]
        views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
        photo[v] = po.estimate_depth_map(views, len(ids), float(sc.dmin[v]), float(sc.dmax[v]), opt(v))
    geo = {}
    for v in refs:
        ids = [v] + [int(i) for i in sc.neighbors[v]]
        views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps={i: photo[i][0] for i in ids[1:]})
        geo[v] = po.estimate_depth_map(views, len(ids), float(sc.dmin[v]), float(sc.dmax[v]), opt(v), geo_iter=0, depth=photo[v][0], normal=photo[v][1])
    for m in list(photo.values()) + list(geo.values()):
        for a in m:
            a.setflags(write=False)
    return refs, photo, geo


def _scene_groups(hyps):
    """Through the scene interface: a batch of five reference views in two view groups (grid.y = 3 and 2), the other four views estimated in a batch of their own so that
    every source has a photometric map for the geometric round."""
    sc = scene()
    refs, photo, geo = _scene_expected()
    rest = [v for v in range(sc.n_views) if v not in refs]
    e = _engine(hyps, viewGroups=2)
    try:
        p = default_params(seed=SEED, nSubResolutionLevels=1, nEstimationGeometricIters=1)
        e.Init(False); e.scene_load(sc, n_levels=1)
        e.scene_estimate(refs, -1, p)
        e.scene_estimate(rest, -1, p)
        for v in range(sc.n_views):
            for a, b, name in zip(e.scene_get_maps(v), photo[v], ("depth", "normal", "conf")):
                _same(a, b, "scene batch, view %d: photometric %s" % (v, name))
        e.scene_commit_round(); e.Init(True)
        e.scene_estimate(refs, 0, p)
        for v in refs:
            got = e.scene_get_maps(v)
            for a, b, name in zip(got, geo[v], ("depth", "normal", "conf")):
                _same(a, b, "scene batch, view %d: geometric %s" % (v, name))
            assert (got[0] != photo[v][0]).any()
    finally:
        e.close()


def run(case, hyps):
    if case.startswith("src"):
        nsrc = int(case[3:])
        # 8: every view lane scores; 7, 5, 3, 1: view lanes idle in every quad row; 9: more sources than view lanes -- the engine's choice of kernel for such a batch
        _both_rounds(hyps, 10 if nsrc > 8 else 9, nsrc)
    elif case == "tiles8":
        _both_rounds(hyps, 9, 8, tile=8)           # tile diagonals of 1 .. 8 pixels: a wave holds pixels of several tiles, neighbours come from the snapshot
    elif case == "mask":
        _both_rounds(hyps, 9, 8, masked=True)
    elif case == "own_size":
        _both_rounds(hyps, 9, 8, own=True)
    elif case == "scene_groups":
        _scene_groups(hyps)
    else:
        raise KeyError(case)
