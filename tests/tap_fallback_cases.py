"""Adversarial cameras for the fallbacks of the optimistic tap path (pm_score_view, csrc/pm_kernels.hip).  The sweep kernels and the init kernel's mode 2 gather the 25 taps
of a patch through the unguarded division pm_div2_inrange and decide afterwards, from the four corner taps, between (1) redoing the patch through the guarded path (a
corner z outside [2^-40, 2^40] or start values that are not `sane`), (2) thRobust (a corner outside the image), (3) accepting the sums and (4) rechecking all 25
positions (a corner within delta of the border band, or zhi > 2 zlo).  On the suite's ordinary scenes (1) and (4) decide a few dozen evaluations in a million; the inputs
here make each of them decide a large share:

behind      one source turned to look the other way (R = diag(-1, 1, -1) R): every tap in it has z < 0 -- (1) for a third of the evaluations.  The reference has no z test
            (ScorePixelImage): a tap with z < 0 is sampled when x / z lands inside the image, so the redo returns real sums, not only thRobust.  The ground truth depth and
            normals 0 .. 89.9 degrees off the viewing ray are planted.
twin        source 1 is the reference camera itself, source 2 has the same centre and twice the focal length: the homographies do not depend on the plane, taps land on
            exact (half-)integers, patches at the border have corners exactly on the band's edge -- (4), and the `<=` of every edge test decides.
twin_shift  the twins with shifted principal points: -1 px (integers; one edge gains a column, the other loses one), +0.5 px on the doubled focal length (integers) and
            +0.5 px on a third twin (half-integers).
edge_on     two sources whose centres lie in the planted plane (z = 1.5 of the reference camera, the same for every pixel) and look along it, so that the plane's picture
            is the line x' = w - 2 resp. y' = h - 2: every tap of every patch lands on the band's edge up to the rounding of its additions, and in some 70 patches of the init
            kernel all four corners are inside and a tap between them is outside -- the one input on which (4)'s recheck changes the result ((3)'s convexity argument is exact
            but for roundings).  Half of each picture has z < 0: the guarded redo meets the same edge.
in_scene    a source whose centre stands inside the reference's depth range on its optical axis, looking sideways: hypothesis planes pass through or near its centre, z
            crosses 0 inside a patch, leaves [2^-40, 2^40], zhi > 2 zlo.  Measured on the emulator: redone + rechecked 18.1 - 20.4 % of the optimistic evaluations
            (18.2 % in the init kernel), nearly all of it redone: a corner that is inside next to one with z <= 0 is rare, the picture of such a patch is mostly outside.
own_size    `behind` with the turned source delivered at 0.8 x the size with its own K: the batch leaves the level's quad buffer (pointer addressing with clamped
            coordinates) and the init kernel scores in mode 0.
eight       nine views, 8 sources: sources 1 and 5 turned (both slots of one lane with two views per lane), source 2 the reference's twin.
geo-*       `behind` and `twin` as resident scenes: photometric pass over all views, commit, a geometric round on two views (the GEO instantiations are separate code).

Every expected value is the oracle's (po.estimate_depth_map with the same cameras, ids, planted maps and seed), computed once per case and shared by the tunings; the oracle's
behaviour on these inputs is pinned to the reference's own code by tests/test_ref_pinning.py.  All cases are one level of 96x72.  Run on the wave64 emulator, with the census
of the branches, by tests/test_emu_tap_fallbacks.py and on the device by tests/test_zz_gpu_tap_fallbacks.py."""
import ctypes as C
import functools
import types

import numpy as np

from openmvs_amd import synth
from openmvs_amd.patchmatch import default_params
from oracle import pyoracle as po
from tests.test_gpu_patchmatch import _same

W, H, SEED = 96, 72, 3
FLIP = np.diag([-1.0, 1.0, -1.0])

PHOTO_CASES = ["behind", "twin", "twin_shift", "in_scene", "edge_on", "own_size", "eight"]
GEO_CASES = ["geo-behind", "geo-twin"]
# what the census of the emulated run has to show before the comparison means anything (tests/test_emu_tap_fallbacks.py): (branch, share of the optimistic evaluations).
# in_scene: 18.1 - 20.4 % measured over the four tunings of the emulator, the floor is half of that.  geo-twin: the twins are sources of two of the scene's four reference
# views only (views 2 and 3 see ordinary neighbours besides), so the scene as a whole has to show half of twin's share.
FLOORS = {"behind": ("redone", 0.20), "own_size": ("redone", 0.20), "eight": ("redone", 0.20), "twin": ("rechecked", 0.01), "twin_shift": ("rechecked", 0.01),
          "in_scene": ("redone+rechecked", 0.09), "edge_on": ("rechecked", 0.0), "geo-behind": ("redone", 0.20), "geo-twin": ("rechecked", 0.005)}
# edge_on: the planted plane is what sits on the edge, and only the init kernel scores exactly that plane (1.52 % of its evaluations rechecked, in 74 of these 256 the
# recheck finds a tap outside between corners that are inside; the sweeps' hypotheses are off the edge by more than the taps' noise: 11 - 22 rechecks in 0.2 - 0.8 M, hence no floor on the total; under pointer addressing the init kernel scores through the guarded rows, whose per-tap tests meet the same edge)
INIT_FLOORS = {"edge_on": 0.0075}

# the emulator's tunings; the device runs DEVICE_TUNINGS (the results never depend on them)
EMU_TUNINGS = {"sweep2-lanes4": dict(wideMaxViews=-1, sweepLanes=4), "wide8": dict(wideMaxViews=64, wideHyps=8), "wide2-pointer": dict(wideMaxViews=64, wideHyps=2, quadBuffer=2),
               "sweep2-lanes8": dict(wideMaxViews=-1, sweepLanes=8)}
DEVICE_TUNINGS = {"sweep2-lanes4-buffer": dict(wideMaxViews=-1, sweepLanes=4, quadBuffer=1), "sweep2-lanes4-pointer": dict(wideMaxViews=-1, sweepLanes=4, quadBuffer=2),
                  "sweep2-lanes8-buffer": dict(wideMaxViews=-1, sweepLanes=8, quadBuffer=1), "sweep2-lanes8-pointer": dict(wideMaxViews=-1, sweepLanes=8, quadBuffer=2),
                  "wide8": dict(wideMaxViews=64, wideHyps=8, sweepLanes=-1, quadBuffer=1), "wide4": dict(wideMaxViews=64, wideHyps=4), "wide2": dict(wideMaxViews=64, wideHyps=2),
                  "default": None}


@functools.lru_cache(maxsize=None)
def _scene(n_views=4, w=W, h=H):
    return synth.make_scene(n_views, w, h, n_src=n_views - 1)


def _steep_normals(sc, ref, seed):
    """Unit normals 0 .. 89.9 degrees off the pixel's viewing ray v = ((x - cx) / fx, (y - cy) / fy, 1), turned towards the camera (n.v < 0), any azimuth."""
    r = np.random.RandomState(seed)
    K = sc.K[ref]
    ys, xs = np.mgrid[0:sc.height, 0:sc.width].astype(np.float64)
    v = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    a = np.cross(v, [0.0, 1.0, 0.0]); a /= np.linalg.norm(a, axis=-1, keepdims=True)
    b = np.cross(v, a)
    tilt = np.deg2rad(89.9) * r.rand(sc.height, sc.width)[..., None]
    az = 2 * np.pi * r.rand(sc.height, sc.width)[..., None]
    n = -np.cos(tilt) * v + np.sin(tilt) * (np.cos(az) * a + np.sin(az) * b)
    return n.astype(np.float32)


def _zoomed(img, K, K2):
    """The image a camera with the same centre and rotation and the calibration K2 sees of the picture `img` taken with K (bilinear, clamped)."""
    h, w = img.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    x = np.clip((xs - K2[0, 2]) / K2[0, 0] * K[0, 0] + K[0, 2], 0, w - 1.001); y = np.clip((ys - K2[1, 2]) / K2[1, 1] * K[1, 1] + K[1, 2], 0, h - 1.001)
    x0 = x.astype(int); y0 = y.astype(int); fx = x - x0; fy = y - y0
    g = img.astype(np.float64)
    return ((g[y0, x0] * (1 - fx) + g[y0, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1, x0] * (1 - fx) + g[y0 + 1, x0 + 1] * fx) * fy).astype(np.float32)


def _twin(sc, ref, focal=1.0, shift=0.0):
    K = sc.K[ref].copy()
    K[0, 0] *= focal; K[1, 1] *= focal; K[0, 2] += shift; K[1, 2] += shift
    return _zoomed(sc.gray[ref], sc.K[ref], K), K, sc.R[ref].copy(), sc.C[ref].copy()


def _sideways(sc, ref, along):
    """A camera on the reference's optical axis at depth `along`, looking along the reference's x axis (its image: the view's own, any picture does)."""
    Rr = sc.R[ref]
    C = sc.C[ref] + Rr.T @ np.array([0.0, 0.0, along])
    R = np.stack([-Rr[2], Rr[1], Rr[0]])            # x_cam = -z_ref, y_cam = y_ref, z_cam = x_ref: a rotation
    return R, C


def _edge_on(sc, ref, depth, edge, focal, axis=0):
    """A camera (the reference's K with the focal length `focal`) whose centre lies in the plane z = depth of the reference camera and whose image column x' = edge
    (axis 0) or row y' = edge (axis 1) is the picture of that plane: it looks along the plane, turned about the other image axis by atan((edge - c) / focal)."""
    Rr = sc.R[ref]; K = sc.K[ref].copy()
    K[0, 0] = K[1, 1] = focal
    phi = np.arctan((edge - K[axis, 2]) / focal)
    z = np.cos(phi) * Rr[axis] + np.sin(phi) * Rr[2]
    R = np.stack([np.cross(Rr[1], z), Rr[1], z]) if axis == 0 else np.stack([Rr[0], np.cross(z, Rr[0]), z])
    return K, R, sc.C[ref] + float(depth) * Rr[2]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(gray, K, R, C: per view id; ids; dmin, dmax; depth, normal: planted maps or None) of a photometric case, or the scene object of a geo case."""
    nine = case == "eight"
    sc = _scene(9 if nine else 4)
    ref = 4 if nine else 0
    n = sc.n_views
    ids = [ref] + [int(i) for i in sc.neighbors[ref]]
    gray = {i: sc.gray[i] for i in range(n)}; K = {i: sc.K[i].copy() for i in range(n)}; R = {i: sc.R[i].copy() for i in range(n)}; Cc = {i: sc.C[i].copy() for i in range(n)}
    depth = normal = None
    base = case[4:] if case.startswith("geo-") else case
    if base in ("behind", "own_size"):
        R[ids[1]] = FLIP @ R[ids[1]]
        depth = sc.gt_depth[ref].copy(); normal = _steep_normals(sc, ref, SEED)
        if base == "own_size":
            small = _scene(4, 77, 58)              # 0.8 x, its own K
            gray[ids[1]] = small.gray[ids[1]]; K[ids[1]] = small.K[ids[1]].copy()
    elif base == "twin":
        gray[ids[1]], K[ids[1]], R[ids[1]], Cc[ids[1]] = _twin(sc, ref)
        gray[ids[2]], K[ids[2]], R[ids[2]], Cc[ids[2]] = _twin(sc, ref, focal=2.0)
    elif base == "twin_shift":
        gray[ids[1]], K[ids[1]], R[ids[1]], Cc[ids[1]] = _twin(sc, ref, shift=-1.0)
        gray[ids[2]], K[ids[2]], R[ids[2]], Cc[ids[2]] = _twin(sc, ref, focal=2.0, shift=0.5)
        gray[ids[3]], K[ids[3]], R[ids[3]], Cc[ids[3]] = _twin(sc, ref, shift=0.5)
    elif base == "in_scene":
        R[ids[1]], Cc[ids[1]] = _sideways(sc, ref, IN_SCENE_ALONG * float(sc.gt_depth[ref].mean()))
        depth = sc.gt_depth[ref].copy(); normal = _steep_normals(sc, ref, SEED)
    elif base == "edge_on":
        d = np.float32(round(float(sc.gt_depth[ref].mean()), 2))
        K[ids[1]], R[ids[1]], Cc[ids[1]] = _edge_on(sc, ref, d, W - 2.0, EDGE_ON_FOCAL, axis=0)
        K[ids[2]], R[ids[2]], Cc[ids[2]] = _edge_on(sc, ref, d, H - 2.0, EDGE_ON_FOCAL, axis=1)
        depth = np.full((H, W), d, np.float32); normal = np.zeros((H, W, 3), np.float32); normal[..., 2] = -1
    elif base == "eight":
        R[ids[1]] = FLIP @ R[ids[1]]; R[ids[5]] = FLIP @ R[ids[5]]
        gray[ids[2]], K[ids[2]], R[ids[2]], Cc[ids[2]] = _twin(sc, ref)
        depth = sc.gt_depth[ref].copy(); normal = _steep_normals(sc, ref, SEED)
    else:
        raise KeyError(case)
    for a in list(gray.values()) + [a for a in (depth, normal) if a is not None]:
        a.setflags(write=False)
    if case.startswith("geo-"):
        return types.SimpleNamespace(n_views=n, width=W, height=H, gray=[gray[i] for i in range(n)], K=[K[i] for i in range(n)], R=[R[i] for i in range(n)], C=[Cc[i] for i in range(n)],
                                     dmin=sc.dmin, dmax=sc.dmax, neighbors=sc.neighbors)
    return dict(gray=gray, K=K, R=R, C=Cc, ids=ids, ref=ref, dmin=float(sc.dmin[ref]), dmax=float(sc.dmax[ref]), depth=depth, normal=normal)


# edge_on: the homography of the planted plane is the same for every pixel, and so is the offset of its float entries from the exact ones (row 0 is (w - 2) x row 2 only
# up to 2^-24): with most focal lengths every tap lands on one side of the edge.  With this one the offset is below the noise of the taps' additions: in about 40 patches per
# source all four corners are inside and a tap between them is outside (counted by restating the kernel's float operations over focal lengths 0.75 .. 1.25 x the scene's).
EDGE_ON_FOCAL = 94.234
IN_SCENE_ALONG = 1.0     # where on the optical axis the sideways camera stands, in units of the mean ground-truth depth


def _frozen(maps):
    for a in maps:
        a.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def expected(case):
    """The oracle's (depth, normal, conf) of a photometric case."""
    c = inputs(case)
    views, keep = po.make_views(c["gray"], c["K"], c["R"], c["C"], c["ids"])
    return _frozen(po.estimate_depth_map(views, len(c["ids"]), c["dmin"], c["dmax"], po.default_opt(seed=SEED, viewID=c["ref"], nSubResolutionLevels=0), depth=c["depth"], normal=c["normal"]))


def geo_views(sc):
    """The views of the geometric round: the reference view of the photometric cases and its first source -- the turned view / the twin itself."""
    return (0, int(sc.neighbors[0][0]))


@functools.lru_cache(maxsize=None)
def expected_geo(case):
    """(photometric maps of every view, geometric-round maps of geo_views()): the oracle throughout, the geometric round fed the oracle's own photometric maps."""
    sc = inputs(case)
    opt = lambda v: po.default_opt(seed=SEED, viewID=v, nSubResolutionLevels=0, nEstimationGeometricIters=1)
    photo = []
    for v in range(sc.n_views):
        ids = [v] + [int(i) for i in sc.neighbors[v]]
        views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
        photo.append(_frozen(po.estimate_depth_map(views, len(ids), float(sc.dmin[v]), float(sc.dmax[v]), opt(v))))
    geo = {}
    for v in geo_views(sc):
        ids = [v] + [int(i) for i in sc.neighbors[v]]
        views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps={u: photo[u][0] for u in range(sc.n_views)})
        geo[v] = _frozen(po.estimate_depth_map(views, len(ids), float(sc.dmin[v]), float(sc.dmax[v]), opt(v), geo_iter=0, depth=photo[v][0], normal=photo[v][1]))
    return photo, geo


@functools.lru_cache(maxsize=None)
def product_defaults():
    """The tuning a fresh engine of the library has (the suite's conftest pins the regular sweep kernel on every engine the bindings create)."""
    from openmvs_amd import patchmatch
    lib = patchmatch.load_library()
    h = C.c_void_p(); t = patchmatch.PMHipTuning()
    assert lib.pmhip_create(0, C.byref(h)) == 0
    try:
        assert lib.pmhip_get_tuning(h, C.byref(t)) == 0
    finally:
        lib.pmhip_destroy(h)
    return {k: getattr(t, k) for k, _ in patchmatch.PMHipTuning._fields_ if k != "reserved0"}


def set_tuning(e, tuning):
    want = product_defaults() if tuning is None else tuning
    got = e.tuning(**want)
    assert all(got[k] == v for k, v in want.items()), (want, got)


def check_input(case):
    """The condition on the input that needs no run: the oracle's map of the reference view is mostly valid (the fallbacks return sums that are accepted, not only thRobust)."""
    d = expected_geo(case)[0][0][0] if case.startswith("geo-") else expected(case)[0]
    assert (d > 0).mean() >= 0.5, "%s: the oracle's map has only %.0f %% valid pixels" % (case, 100 * (d > 0).mean())


def compute(e, case):
    """Run the case on engine `e`; returns [(what, got, expected)] of every map for compare()."""
    if not case.startswith("geo-"):
        c = inputs(case)
        e.Init(False)
        got = e.EstimateDepthMap(c["gray"], c["K"], c["R"], c["C"], c["ids"], c["dmin"], c["dmax"], depth=c["depth"], normal=c["normal"], params=default_params(seed=SEED, nSubResolutionLevels=0))
        return list(zip(("depth", "normal", "conf"), got, expected(case)))
    sc = inputs(case)
    photo, geo = expected_geo(case)
    p = default_params(seed=SEED, nSubResolutionLevels=0, nEstimationGeometricIters=1)
    allv = list(range(sc.n_views))
    out = []
    e.Init(False); e.scene_load(sc, n_levels=0)
    e.scene_estimate(allv, -1, p)
    for v in allv:
        out += [("photometric %s of view %d" % (name, v), a, b) for name, a, b in zip(("depth", "normal", "conf"), e.scene_get_maps(v), photo[v])]
    e.scene_commit_round(); e.Init(True)
    e.scene_estimate(list(geo_views(sc)), 0, p)
    for v in geo_views(sc):
        got = e.scene_get_maps(v)
        assert (got[0] != photo[v][0]).any(), "%s: the geometric round left view %d as it was" % (case, v)
        out += [("geometric %s of view %d" % (name, v), a, b) for name, a, b in zip(("depth", "normal", "conf"), got, geo[v])]
    return out


def compare(results, what):
    for name, got, want in results:
        _same(got, want, "%s: %s" % (what, name))


def run(e, case, what):
    check_input(case)
    compare(compute(e, case), "%s, %s" % (case, what))
