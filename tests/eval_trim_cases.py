"""Cases for what surrounds the taps of a patch evaluation (pm_score_view / pm_row_issue, csrc/pm_kernels.hip; pm_visit, csrc/pm_band.hip): the test of the first row's
two corner taps before any load, the image-size thresholds a quad-buffer launch keeps in scalar registers, and the prior blend's distance term formed once per trip.

1. The cases of tests/tap_fallback_cases.py and the `families` scene of tests/geo_gather_cases.py once more, through pm_sweep2_kernel with 4 and 8 lanes per pixel under
   buffer and pointer addressing, and the engine's default (TUNINGS).
2. half_seen: every source is a twin of the reference camera (same centre and rotation, so the homography does not depend on the plane) with 0.9 x the focal length --
   every tap of every patch lands inside -- and source 1's principal point is moved down by 8 px: y' = cy + 8 + 0.9 (y - cy).  A patch's first row (y - 4) is inside for
   every pixel; its last rows leave the image (y' > h - 2) for the pixels of rows 61 .. 67.  The test before the loads passes and the verdict after the gather decides.
3. row0_outside: the mirrored source, moved up by 8 px: the first row lies above y' = 1 for the pixels of rows 4 .. 9 while their last row is inside: the test before the
   loads decides, no other test would.
4. prior: two pyramid levels of 96x72 -- the prior is positive on level 0 -- with six sources (two per lane on four lanes per pixel), photometric pass and one geometric
   round, through the init kernel (part of every call), pm_sweep2_kernel and the two-wide kernel.

Every expected value is the sequential oracle's, computed once per case.  All cases are 96x72.  Run on the wave64 emulator by tests/test_emu_eval_trim.py (with the census
of the two new cases' branches) and on the device by tests/test_zz_gpu_eval_trim.py."""
import functools

import numpy as np

from openmvs_amd import synth
from openmvs_amd.patchmatch import default_params
from oracle import pyoracle as po
from tests import geo_gather_cases as geo, tap_fallback_cases as tap
from tests.test_gpu_patchmatch import _same

W, H, SEED = tap.W, tap.H, tap.SEED
NEW_CASES = ["half_seen", "row0_outside"]
SHIFT = {"half_seen": 8.0, "row0_outside": -8.0}
FOCAL = 0.9
# rows of reference pixels whose patches the shifted source sees half of (from the formulas above, with a row to spare at the band's fuzzy end), and the pixels per row
BAND_ROWS = {"half_seen": 6, "row0_outside": 5}
ROW_PIXELS = W - 2 * 4
TUNINGS = {"sweep2-lanes4-buffer": dict(wideMaxViews=-1, sweepLanes=4, quadBuffer=1), "sweep2-lanes4-pointer": dict(wideMaxViews=-1, sweepLanes=4, quadBuffer=2),
           "sweep2-lanes8-buffer": dict(wideMaxViews=-1, sweepLanes=8, quadBuffer=1), "sweep2-lanes8-pointer": dict(wideMaxViews=-1, sweepLanes=8, quadBuffer=2),
           "default": None}
PRIOR_TUNINGS = {"sweep2-lanes4": dict(wideMaxViews=-1, sweepLanes=4), "wide2": dict(wideMaxViews=64, wideHyps=2)}
PRIOR_VIEWS = 7


@functools.lru_cache(maxsize=None)
def inputs(case):
    if case not in NEW_CASES:
        return tap.inputs(case)
    sc = tap._scene(4)
    ref = 0
    ids = [ref] + [int(i) for i in sc.neighbors[ref]]
    gray = {ref: sc.gray[ref]}; K = {ref: sc.K[ref].copy()}; R = {ref: sc.R[ref].copy()}; Cc = {ref: sc.C[ref].copy()}
    for n, i in enumerate(ids[1:]):
        K2 = sc.K[ref].copy()
        K2[0, 0] *= FOCAL; K2[1, 1] *= FOCAL
        if n == 0:
            K2[1, 2] += SHIFT[case]
        gray[i] = tap._zoomed(sc.gray[ref], sc.K[ref], K2); K[i] = K2; R[i] = sc.R[ref].copy(); Cc[i] = sc.C[ref].copy()
    for a in gray.values():
        a.setflags(write=False)
    return dict(gray=gray, K=K, R=R, C=Cc, ids=ids, ref=ref, dmin=float(sc.dmin[ref]), dmax=float(sc.dmax[ref]), depth=None, normal=None)


@functools.lru_cache(maxsize=None)
def expected(case):
    if case not in NEW_CASES:
        return tap.expected(case)
    c = inputs(case)
    views, keep = po.make_views(c["gray"], c["K"], c["R"], c["C"], c["ids"])
    return tap._frozen(po.estimate_depth_map(views, len(c["ids"]), c["dmin"], c["dmax"], po.default_opt(seed=SEED, viewID=c["ref"], nSubResolutionLevels=0)))


def compute(e, case):
    if case not in NEW_CASES:
        return tap.compute(e, case)
    c = inputs(case)
    e.Init(False)
    got = e.EstimateDepthMap(c["gray"], c["K"], c["R"], c["C"], c["ids"], c["dmin"], c["dmax"], params=default_params(seed=SEED, nSubResolutionLevels=0))
    return list(zip(("depth", "normal", "conf"), got, expected(case)))


def run(e, case, tuning):
    """One case under one tuning on engine `e`, against the oracle bit for bit."""
    tap.set_tuning(e, TUNINGS[tuning])
    if case == "families":
        over = tap.product_defaults() if TUNINGS[tuning] is None else TUNINGS[tuning]
        for t in ("sweep2-lanes4", "sweep2-lanes4-two-views-per-lane"):      # the scene with four and with six sources (one and two views per lane on four lanes), under `tuning`
            saved = geo.TUNINGS[t]
            geo.TUNINGS[t] = over
            try:
                geo.families(e, t)
            finally:
                geo.TUNINGS[t] = saved
        return
    results = compute(e, case)
    if case in NEW_CASES:
        assert (results[0][1] > 0).mean() >= 0.5, "%s: only %.0f %% of the map is valid" % (case, 100 * (results[0][1] > 0).mean())
    tap.compare(results, "%s, %s" % (case, tuning))


@functools.lru_cache(maxsize=None)
def _prior_scene():
    return synth.make_scene(PRIOR_VIEWS, W, H, n_src=PRIOR_VIEWS - 1)


@functools.lru_cache(maxsize=None)
def prior_expected():
    """Oracle maps of the two-level photometric pass of view 0 against its six sources and of one geometric round on top (the sources' depth maps: the reference view's
    photometric map, as tests/widen_lane_order_cases.py)."""
    sc = _prior_scene()
    ids = [0] + [int(i) for i in sc.neighbors[0]]
    opt = po.default_opt(seed=SEED, viewID=0, nSubResolutionLevels=1, nEstimationGeometricIters=1)
    dmin, dmax = float(sc.dmin[0]), float(sc.dmax[0])
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
    photo = po.estimate_depth_map(views, len(ids), dmin, dmax, opt)
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps={i: photo[0] for i in ids[1:]})
    geo_maps = po.estimate_depth_map(views, len(ids), dmin, dmax, opt, geo_iter=0, depth=photo[0], normal=photo[1])
    return ids, tap._frozen(photo), tap._frozen(geo_maps)


def prior(e, tuning):
    sc = _prior_scene()
    ids, photo, geo_maps = prior_expected()
    tap.set_tuning(e, PRIOR_TUNINGS[tuning])
    p = default_params(seed=SEED, nSubResolutionLevels=1, nEstimationGeometricIters=1)
    e.Init(False)
    got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[0], sc.dmax[0], params=p)
    for a, b, name in zip(got, photo, ("depth", "normal", "conf")):
        _same(a, b, "prior, %s: photometric %s" % (tuning, name))
    assert (got[0] > 0).mean() > 0.3
    e.Init(True)
    got = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[0], sc.dmax[0], depth=photo[0].copy(), normal=photo[1].copy(),
                             src_depths={i: photo[0] for i in ids[1:]}, nGeometricIter=0, params=p)
    for a, b, name in zip(got, geo_maps, ("depth", "normal", "conf")):
        _same(a, b, "prior, %s: geometric %s" % (tuning, name))
    assert (got[0] != photo[0]).any()
