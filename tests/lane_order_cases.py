"""Cases for the sweep kernel's view-major lane order (pm_sweep2_kernel, csrc/pm_band.hip: lane = lane row v * PPW + pixel, PPW = 64 / G pixels per wave): whatever the
G lanes of a pixel exchange -- the close-neighbour ballot, the smoothness factors through the pixel's LDS state, the sine / cosine swap of Dir2Normal, the two-smallest
reduction over lanes PPW apart, the verdict of lane row 0 on prior and mask -- crosses quads and DPP rows, so every case compares depth, normal and confidence bit for
bit with the sequential oracle.  Run on the wave64 emulator by tests/test_emu_lane_order.py and on the device by tests/test_zz_gpu_lane_order.py.

Shapes: nine views at 64x48 with one sub-resolution level, i.e. levels of 64x48 and 32x24 whose inner anti-diagonals have every length from 1 to 40 -- quads and waves
occur partly filled at both ends.  pm_sweep2 is forced (no speculative kernels) with 4 or 8 lanes per pixel."""
import functools

import numpy as np

from openmvs_amd import synth
from openmvs_amd.patchmatch import default_params
from oracle import pyoracle as po
from tests.test_gpu_patchmatch import _oracle, _same

W, H, REF, SEED = 64, 48, 4, 5

# (case, lanes per pixel): every case with 4 lanes; 8 sources, 3 sources and the 8x8 tiles also with 8
CASES = [("src8", 4), ("src7", 4), ("src5", 4), ("src3", 4), ("src1", 4), ("src9", 4), ("mask", 4), ("own_size", 4), ("tiles8", 4),
         ("src8", 8), ("src3", 8), ("tiles8", 8)]


@functools.lru_cache(maxsize=None)
def scene(n_views=9):
    return synth.make_scene(n_views, W, H, n_src=n_views - 1)


def _engine(lanes):
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    got = e.tuning(wideMaxViews=-1, sweepLanes=lanes, wideHyps=-1)
    assert got["sweepLanes"] == lanes and got["wideMaxViews"] == -1
    return e


@functools.lru_cache(maxsize=None)
def _expected_rounds(n_views, nsrc, tile):
    """Oracle maps of the photometric pass and of one geometric round on top of it (the sources' depth maps: the reference view's photometric map -- any maps do, both
    sides read the same, and plausible depths take the consistency branch)."""
    sc = scene(n_views)
    ref = REF if n_views == 9 else 5
    ids = [ref] + [int(i) for i in sc.neighbors[ref][:nsrc]]
    kw = dict(nSubResolutionLevels=1, nEstimationGeometricIters=1)
    if tile:
        kw.update(tileW=tile, tileH=tile)
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
    opt = po.default_opt(seed=SEED, viewID=ref, **kw)
    photo = po.estimate_depth_map(views, len(ids), float(sc.dmin[ref]), float(sc.dmax[ref]), opt)
    src = {i: photo[0] for i in ids[1:]}
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps=src)
    geo = po.estimate_depth_map(views, len(ids), float(sc.dmin[ref]), float(sc.dmax[ref]), opt, geo_iter=0, depth=photo[0], normal=photo[1])
    for a in photo + geo:
        a.setflags(write=False)
    return ref, ids, photo, geo


def _both_rounds(lanes, n_views, nsrc, tile=0):
    sc = scene(n_views)
    ref, ids, photo, geo = _expected_rounds(n_views, nsrc, tile)
    what = "%d sources, %d lanes%s" % (nsrc, lanes, ", %dx%d tiles" % (tile, tile) if tile else "")
    e = _engine(lanes)
    try:
        if tile:
            e.set_sweep_tiles(tile, tile)
        p = default_params(seed=SEED, nSubResolutionLevels=1, nEstimationGeometricIters=1)
        e.Init(False)
        got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[ref], sc.dmax[ref], params=p)
        for a, b, name in zip(got, photo, ("depth", "normal", "conf")):
            _same(a, b, "%s: photometric %s" % (what, name))
        assert (got[0] > 0).mean() > 0.3
        e.Init(True)
        got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[ref], sc.dmax[ref], depth=photo[0].copy(), normal=photo[1].copy(),
                                 src_depths={i: photo[0] for i in ids[1:]}, nGeometricIter=0, params=p)
        for a, b, name in zip(got, geo, ("depth", "normal", "conf")):
            _same(a, b, "%s: geometric %s" % (what, name))
        assert (got[0] != photo[0]).any()
    finally:
        e.close()


def _mask(lanes):
    """Ignored pixels inside quads and waves: single pixels scattered so that quads of neighbouring diagonal pixels lose one or two, and a whole anti-diagonal (38 pixels in a
    row: at least one whole wave of 16 whatever the wave boundaries are).  8 sources, photometric pass over both levels."""
    sc = scene()
    ids = [REF] + [int(i) for i in sc.neighbors[REF]]
    mask = np.full((H, W), 255, np.uint8)
    mask[::3, ::5] = 0
    mask[7::4, 9::7] = 0
    for y in range(6, 44):
        mask[y, 55 - y] = 0
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
    want = po.estimate_depth_map_masked(views, len(ids), float(sc.dmin[REF]), float(sc.dmax[REF]), po.default_opt(seed=SEED, viewID=REF, nSubResolutionLevels=1), mask, mask_mode=True)
    e = _engine(lanes)
    try:
        e.Init(False)
        got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[REF], sc.dmax[REF], params=default_params(seed=SEED, nSubResolutionLevels=1), mask=mask)
        for a, b, name in zip(got, want, ("depth", "normal", "conf")):
            _same(a, b, "ignore mask, %d lanes: %s" % (lanes, name))
        assert not got[0][mask == 0].any() and (got[0][mask != 0] > 0).mean() > 0.3
    finally:
        e.close()


def _own_size(lanes):
    """Two of the eight sources carry their own image size (0.75x and 1.25x): the batch reads its taps through each view's own pointer with clamped coordinates, not
    through the level's quad buffer."""
    base = scene()
    small = synth.make_scene(9, W * 3 // 4, H * 3 // 4, n_src=8)
    big = synth.make_scene(9, W * 5 // 4, H * 5 // 4, n_src=8)
    ids = [REF] + [int(i) for i in base.neighbors[REF]]
    gray = {i: base.gray[i] for i in range(9)}; K = {i: base.K[i] for i in range(9)}
    gray[ids[2]] = small.gray[ids[2]]; K[ids[2]] = small.K[ids[2]]
    gray[ids[5]] = big.gray[ids[5]]; K[ids[5]] = big.K[ids[5]]
    views, keep = po.make_views(gray, K, base.R, base.C, ids)
    want = po.estimate_depth_map(views, len(ids), float(base.dmin[REF]), float(base.dmax[REF]), po.default_opt(seed=SEED, viewID=REF, nSubResolutionLevels=1))
    e = _engine(lanes)
    try:
        e.Init(False)
        got = e.EstimateDepthMap(gray, K, base.R, base.C, ids, base.dmin[REF], base.dmax[REF], params=default_params(seed=SEED, nSubResolutionLevels=1))
        for a, b, name in zip(got, want, ("depth", "normal", "conf")):
            _same(a, b, "sources of their own size, %d lanes: %s" % (lanes, name))
        assert (got[0] > 0).mean() > 0.3
    finally:
        e.close()


def run(case, lanes):
    if case.startswith("src"):
        nsrc = int(case[3:])
        # 8, 7, 5: (4,2) or (8,1), the second view round / the upper lane rows partly idle; 3: (4,1) with lane row 3 idle; 1: the minimum over a group with one score;
        # 9: (4,4) or (8,2) -- a ten-view scene
        _both_rounds(lanes, 10 if nsrc > 8 else 9, nsrc)
    elif case == "tiles8":
        _both_rounds(lanes, 9, 8, tile=8)          # tile diagonals of 1 .. 8 pixels: shorter than a quad, a wave holds pixels of several tiles
    elif case == "mask":
        _mask(lanes)
    elif case == "own_size":
        _own_size(lanes)
    else:
        raise KeyError(case)
