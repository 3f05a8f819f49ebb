"""Plain SGM (minResolution = 0): Match over ONE disparity range of up to 1024 entries through sgmhip_set_problem_uniform (csrc/sgm_kernels_wide.hip), and the plain loop
around it (openmvs_amd.tsgm._plain_match, sgmhip_tsgm_match with minResolution 0).  Shared by the emulated run (tests/test_emu_sgm_plain.py) and the device run
(tests/test_zz_gpu_sgm_plain.py); the host-only parts are tests/test_sgm_plain.py.

Every comparison is bit for bit against oracle.pyoracle -- cost bytes, 8-path sums, disparity, cost -- and every case first asserts, on its inputs or on the oracle's
result, that it reaches the edge it is named after.  The oracle's aggregation is the reference's loop over all previous disparities, quadratic in D: wide cases keep to
a few hundred valid pixels."""
import functools

import numpy as np

from openmvs_amd import sgm, tsgm
from oracle import pyoracle as po
from tests import sgm_cases as sc
from tests.tsgm_backends import OracleBackend

NO_DISP = 32767
CAP = 1024
# sgm_path_wide_kernel keeps s = 4, 8 or 16 entries per lane: 129 .. 256 disparities through the uniform entry, <= 512, and beyond
# item 1 of the issue, and 63 s, 64 s, 64 s + 1 for s = 8 and 16 (64 * 16 + 1 = 1025 is past the cap: a refusal; s = 4 is in NARROW_D and 257 here)
SWEEP_D = sorted({257, 258, 319, 320, 321, 511, 512, 513, 767, 1023, 1024} | {63 * 8, 64 * 8, 64 * 8 + 1, 63 * 16, 64 * 16})
NARROW_D = (1, 2, 64, 65, 128, 129, 256, 252, 254)   # item 8; 129 .. 256 aggregate with sgm_path_wide_kernel<4>: 63 * 4 too, and 254, its even D that is no multiple of 4
SHIFT = 5                                        # the planted disparity of the sweep's pair
NAMES = ("disparity", "cost", "cost volume", "8-path sums")


def tables():
    """{route: P2s}: the default table (max 60: byte deltas) and one above 255 (u16 atomic sums), as tests/test_gpu_sgm.py builds it."""
    d = po.sgm_generate_p2s()
    up = np.minimum(d.astype(np.int64) * 40 + 200, 3000).astype(np.uint16)
    assert int(d.max()) == 60 and int(up.max()) > 255
    return {"byte": d, "u16": up}


def uniform_table(vw, vh, mn, mx):
    px = np.zeros(vw * vh, sgm.PIXEL_DTYPE)
    px["idx"] = np.arange(vw * vh, dtype=np.uint64) * np.uint64(mx - mn); px["minDisp"] = mn; px["maxDisp"] = mx
    return px, vw * vh * (mx - mn), mx - mn


class Case:
    def __init__(self, name, images, mn, D, routes=("byte", "u16"), check=None):
        self.name = name; self.bgr, self.gl, self.gr = images
        self.mn, self.mx, self.D = int(mn), int(mn) + int(D), int(D)
        self.routes = routes; self.check = check
        h, w = self.gl.shape
        self.vw, self.vh = w - 6, h - 6
        self._want = {}

    def table(self):
        return uniform_table(self.vw, self.vh, self.mn, self.mx)

    def oracle(self, route):
        """(disparity, cost, cost volume, sums) of the oracle on the uniform table; computed once per process"""
        if route not in self._want:
            px, n, mxd = self.table()
            self._want[route] = po.sgm_match(self.bgr, self.gl, self.gr, px, n, mxd, 3, tables()[route])
            if self.check:
                self.check(self, self._want[route])
        return self._want[route]


def same(got, want, what):
    for nm, a, b in ((NAMES[2], got[2], want[2]), (NAMES[3], got[3], want[3]), (NAMES[0], got[0], want[0]), (NAMES[1], got[1], want[1])):
        assert np.array_equal(a, b), "%s: %s: %d of %d differ" % (what, nm, int((a != b).sum()), a.size)


def run_uniform(m, c, route):
    m.P1 = 3; m.P2s = tables()[route]
    m.set_problem_uniform(c.bgr, c.gl, c.gr, c.mn, c.mx)
    m.Match()
    return m.results(volumes=True)


def run_table(m, c, route):
    m.P1 = 3; m.P2s = tables()[route]
    m.set_problem(c.bgr, c.gl, c.gr, *c.table())
    m.Match()
    return m.results(volumes=True)


def check_case(m, c):
    """the case on every route it names through set_problem_uniform against the oracle; -> the engine's results"""
    saved = m.P1, m.P2s
    out = {}
    try:
        for route in c.routes:
            want = c.oracle(route)
            out[route] = run_uniform(m, c, route)
            same(out[route], want, "%s, D = %d, %s route" % (c.name, c.D, route))
    finally:
        m.P1, m.P2s = saved
    return out


# ---- items 1, 2: the D sweep on a 71 x 9 image (valid grid 65 x 3: one pixel past a 64-pixel chunk, lines of 1, 3 and 65 pixels) -------------------------------
@functools.lru_cache(maxsize=None)
def sweep_pair():
    return sc.stereo_pair(71, 9, SHIFT, seed=21)


@functools.lru_cache(maxsize=None)
def sweep_case(D, entry):
    """the true disparity at entry `entry` of the range ("last" = D - 2)"""
    k = D - 2 if entry == "last" else entry
    assert 0 < k < D

    def check(c, o, k=k):
        win = o[0].astype(np.int64) - c.mn
        assert (win == k).mean() > 0.5, "the planted disparity wins at entry %d: %s" % (k, np.bincount(win.ravel()).argmax())
        assert c.vw == 65 and c.vh == 3
    return Case("sweep-D%d-entry%s" % (D, entry), sweep_pair(), SHIFT - k, D, check=check)


def sweep_cases(D):
    return [sweep_case(D, e) for e in (1, 256, "last")]


# ---- item 3: the range wholly outside the right image ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def outside_case(side):
    """every window of every entry leaves the right image: all costs 255, all entries tie, the first one wins across lanes and slices"""
    images = sc.stereo_pair(27, 8, 2, seed=22)
    w = images[1].shape[1]
    mn = w if side == "right" else -w - CAP

    def check(c, o):
        assert (o[2] == 255).all() and (o[0] == c.mn).all() and c.D == CAP
        acc = o[3].reshape(-1, c.D)
        assert (acc == acc[:, :1]).all(), "every entry of a pixel ties"
    return Case("outside-" + side, images, mn, CAP, check=check)


def mirrored_case():
    """the winners on entry D - 1: the range ends where the right image's last full window does, so every entry but the last few is 255 for the rightmost pixels"""
    images = sc.stereo_pair(27, 8, 2, seed=23)
    D = 300

    def check(c, o):
        win = o[0].astype(np.int64) - c.mn
        assert (win == c.D - 1).sum() >= c.vh, "winners on the last entry: %d" % int((win == c.D - 1).sum())
    # disparity 2 is the truth: put it on the last entry
    return Case("winners-on-the-last-entry", images, 2 - (D - 1), D, check=check)


# ---- item 4: degenerate grids at D = 1024 -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_cases():
    out = []
    for vw, vh in ((1, 1), (1, 40), (40, 1)):
        def check(c, o, vw=vw, vh=vh):
            assert (c.vw, c.vh) == (vw, vh) and c.D == CAP and o[2].size == vw * vh * CAP and (o[2] != 255).any()
        # (a grid one pixel wide has a single disparity whose window lies inside the image, 0: the pair is planted there)
        out.append(Case("grid-%dx%d" % (vw, vh), sc.stereo_pair(vw + 6, vh + 6, 3 if vw > 1 else 0, seed=30 + vw), -500, CAP, check=check))
    return out


# ---- item 5: chunk boundaries along a line ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_cases():
    out = []
    for vw in (63, 64, 65, 128, 129):
        def check(c, o, vw=vw):
            assert (c.vw, c.vh) == (vw, 2) and c.D == 300 and (o[2] != 255).any()
        out.append(Case("chunk-%dx2" % vw, sc.stereo_pair(vw + 6, 8, 4, seed=40 + vw), -150, 300, check=check))
    return out


# ---- item 6: grey values that are not finite ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nonfinite_case():
    lb, lg, rg = sc.stereo_pair(40, 11, 3, seed=50)
    lg = lg.copy(); lg[2, 5] = np.nan; lg[3, 20] = np.inf          # read by the paths at valid-grid coordinates (2, 5), (3, 20) and by the windows around them

    def check(c, o):
        assert np.isnan(c.gl).sum() == 1 and np.isinf(c.gl).sum() == 1 and c.D == 300
        costs = o[2].reshape(c.vh, c.vw, c.D)
        inside = costs[:, :, 140:160]                                # disparities -10 .. 9: windows inside the image for the middle pixels
        assert (inside[0, 3] == 255).all(), "a window that holds the NaN costs 255 everywhere"
        assert (costs != 255).any()
    return Case("non-finite-grey", (lb, lg, rg), -150, 300, check=check)


# ---- item 8: D <= 256 through the new entry ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_case(D):
    return Case("narrow-D%d" % D, sc.stereo_pair(75, 9, 3, seed=60 + D % 7), -(D // 3), D,
                check=lambda c, o: _assert(c.D <= 256 and c.vw == 69 and (o[2] != 255).any()))


def _assert(v):
    assert v


def check_narrow(m, D):
    c = narrow_case(D)
    got = check_case(m, c)
    saved = m.P1, m.P2s
    try:
        for route in c.routes:
            same(run_table(m, c, route), got[route], "narrow D = %d, %s route: the table entry against the uniform entry" % (D, route))
    finally:
        m.P1, m.P2s = saved


# ---- item 7: refinement on the sums of a wide Match -----------------------------------------------------------------------------------------------------------------
def refine_cases():
    return [sweep_case(320, 256), outside_case("right"), mirrored_case()]


def check_refine(m, c):
    saved = m.P1, m.P2s
    try:
        want = c.oracle("byte")
        got = run_uniform(m, c, "byte")
        same(got, want, c.name)
        m.set_disparity(want[0])
        m.RefineDisparityMap(6, 4)
        ref = po.sgm_refine(want[0], c.table()[0], want[3], 6, 4)
        assert np.array_equal(m.results()[0], ref), "%s: refined disparities" % c.name
    finally:
        m.P1, m.P2s = saved


# ---- item 9: refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(m):
    c = narrow_case(64)
    for mn, mx in ((3, 3), (5, 2), (-500, -500 + CAP + 1), (0, 64 * 16 + 1)):
        try:
            m.set_problem_uniform(c.bgr, c.gl, c.gr, mn, mx)
        except sgm.SGMError as e:
            assert str(CAP) in str(e), str(e)
        else:
            raise AssertionError("set_problem_uniform accepted [%d, %d)" % (mn, mx))
    check_case(m, c)                                                 # an ordinary problem right afterwards
    try:
        m.plain_range(np.zeros((0, 3), np.int16))
    except sgm.SGMError:
        pass
    else:
        raise AssertionError("plain_range accepted an empty map")


# ---- the plain loop -------------------------------------------------------------------------------------------------------------------------------------------------
RANGE_TABLE = ((3, 20, -10, 56), (100, 350, 184, 716), (-300, 180, -616, 376), (0, 0, -16, 16), (-40, 32767, -96, 14), (-16, 32767, -48, 14), (32767, 32767, -18, 14))


def two_sided_seed(w, h, d):
    """-d on the left half, +d on the right half of the half-resolution valid grid"""
    sh = (int(np.rint(h * 0.5)) - 6, int(np.rint(w * 0.5)) - 6)
    s = np.full(sh, d, np.int16); s[:, :sh[1] // 2] = -d
    return s


def restated_plain(be, lb, lg, rb, rg, lm, rm, seed, n_speckle_size=100, mode=6, steps=4):
    """Steps 2-7 of the reference's plain branch (SemiGlobalMatcher.cpp:612-706), literally, over the backend's methods."""
    h, w = lg.shape
    vw, vh = w - 6, h - 6
    lm = tsgm.resize_nearest_u8(lm, w, h)[3:3 + vh, 3:3 + vw].copy(); rm = tsgm.resize_nearest_u8(rm, w, h)[3:3 + vh, 3:3 + vw].copy()     # 2: resized (identity), cropped
    i16 = lambda v: int(np.int64(v).astype(np.int16))
    lo, hi = int(seed.min()), int(seed.max())                                                                                               # 3: NO_DISP included
    num = i16(i16(hi - lo) + 16); disp = i16(lo + hi)
    mn, mx = i16(disp - num), i16(disp + num)
    be.set_problem(rb, rg, lg, *uniform_table(vw, vh, mn, mx)); be.Match()                                                                   # 4: the range as it is
    right, _ = be.results()
    be.set_problem(lb, lg, rg, *uniform_table(vw, vh, -mx, -mn)); be.Match()                                                                 # 5: negated
    left, _ = be.results()
    left = be.ConsistencyCrossCheck(left, right); right = be.ConsistencyCrossCheck(right, left)                                              # 6
    left = be.FilterSpeckles(left, n_speckle_size, 5); right = be.FilterSpeckles(right, n_speckle_size, 5)
    lm = be.ExtractMask(left, lm); rm = be.ExtractMask(right, rm)
    be.set_disparity(left); be.RefineDisparityMap(mode, steps)                                                                               # 7
    return be.results() + ((mn, mx),)


@functools.lru_cache(maxsize=None)
def loop_case(name):
    """(images and masks, seed, core window, true disparity, D) of the plain-loop cases"""
    if name == "narrow":                                             # D = 56: the kernels of sgm_kernels.hip serve
        w, h, d, s, core = 160, 96, 12, 6, (slice(10, -10), slice(30, -42))
    else:                                                            # D = 272: sgm_kernels_wide.hip
        w, h, d, s, core = 290, 16, 120, 60, (slice(None), slice(10, -130))
    lb, lg, rg = sc.stereo_pair(w, h, d, seed=4)
    rb = np.roll(lb, d, axis=1)                                      # the right colour image of the same shift, as tests/test_tsgm.py makes it
    mask = np.full((h, w), 255, np.uint8)
    seed = two_sided_seed(w, h, s)
    D = 2 * (2 * s + 16)
    assert tsgm.plain_range(seed) == (-D // 2, D // 2)
    return (lb, lg, rb, rg, mask, mask), seed, core, d, D


@functools.lru_cache(maxsize=None)
def loop_oracle(name):
    """the product loop on the oracle backend; the planted disparity is found in the core"""
    args, seed, core, d, D = loop_case(name)
    disp, cost, levels = tsgm.tsgm_match(OracleBackend(), *args, min_resolution=0, init_left_disparity=seed)
    h, w = args[1].shape
    assert levels == 1 and disp.shape == cost.shape == (h - 6, w - 6)
    c = disp[core]
    valid = c != NO_DISP
    assert valid.mean() > 0.9
    v = c[valid].astype(np.float64) / 4
    assert abs(np.median(v) - d) < 0.26 and (np.abs(v - d) < 1).mean() > 0.95
    return disp, cost


def check_loop(m, engine, name):
    """the resident call == the step-wise loop on the device backend == the loop on the oracle backend"""
    from tests.tsgm_backends import DeviceBackend
    args, seed, core, d, D = loop_case(name)
    want = loop_oracle(name)
    lb, lg, rb, rg, lm, rm = args
    disp, cost, levels = m.tsgm_match(lb, rb, lg, rg, lm, rm, min_resolution=0, init_left_disparity=seed)
    assert levels == 1
    assert np.array_equal(disp, want[0]) and np.array_equal(cost, want[1]), "%s: resident call against the oracle-backend loop" % name
    d2, c2, l2 = tsgm.tsgm_match(DeviceBackend(m, engine), *args, min_resolution=0, init_left_disparity=seed)
    assert l2 == 1 and np.array_equal(d2, disp) and np.array_equal(c2, cost), "%s: step-wise loop against the resident call" % name


def check_loop_errors(m):
    """an empty seed grid and a seed whose range is wider than the cap, through the C entry point; the engine computes right afterwards"""
    lb, lg, rg = sc.stereo_pair(40, 13, 2, seed=3)
    mask = np.full((13, 40), 255, np.uint8)
    try:
        m.tsgm_match(lb, lb, lg, rg, mask, mask, min_resolution=0)
    except sgm.SGMError as e:
        assert "empty" in str(e), str(e)
    else:
        raise AssertionError("a 13-row image has no half-resolution seed grid")
    lb, lg, rg = sc.stereo_pair(40, 20, 2, seed=3)
    mask = np.full((20, 40), 255, np.uint8)
    seed = np.zeros((4, 14), np.int16); seed[0, 0] = -300; seed[1, 1] = 300       # D = 2 (600 + 16) = 1232
    try:
        m.tsgm_match(lb, lb, lg, rg, mask, mask, min_resolution=0, init_left_disparity=seed)
    except sgm.SGMError as e:
        assert "-300" in str(e) and "300" in str(e) and "1232" in str(e) and str(CAP) in str(e), str(e)
    else:
        raise AssertionError("D = 1232 was accepted")
    d, c, lv = m.tsgm_match(lb, lb, lg, rg, mask, mask, min_resolution=0)            # no seed: [-18, 14)
    want = tsgm.tsgm_match(OracleBackend(), lb, lg, lb, rg, mask, mask, min_resolution=0)
    assert lv == 1 and np.array_equal(d, want[0]) and np.array_equal(c, want[1])


# ---- the pipeline: match_pair(min_resolution=0) on tests/data/scene ------------------------------------------------------------------------------------------------
PIPELINE_LEVEL, PIPELINE_RANGE = 2, (-38, 28)


def check_pipeline(m):
    """Pair (0, 2) of tests/data/scene at a quarter of its size (level 2: 160 x 120 images, 160 x 124 rectified), seeded from the sparse points: the host-rectified
    route, the device-rectified route and the oracle backend give the same .dimap content.  The seeded range is [-38, 28), D = 66.  The scene does not reach the wide
    kernels at any level -- the same pair seeds D = 170 at full size (640 x 479), 100 at half size -- and the oracle needs ~1 s for this level against ~15 s for the
    next; the plain loop over the wide kernels is check_loop("wide") (D = 272)."""
    from openmvs_amd import rectify, sgm_pipeline, views
    from tests import sgm_rectify_cases as rc
    A, B = 0, 2
    scn, cams, bgr, seen = rc.load_scene(PIPELINE_LEVEL)
    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    X = scn.vertices[seen[A] & seen[B]]
    avg = views.select_neighbor_views(scn, cams, A)[3]
    pts = np.nonzero(seen[A])[0]
    depths = []

    def seed(w, h):
        K, R, C, _, _ = scn.camera(A, (w, h))
        P = K @ np.hstack([R, -(R @ C)[:, None]])
        depths.append(views.triangulate_points_depth_map(K, P, scn.vertices[pts], w, h, avg_depth=avg)[0])
        return depths[-1]
    args = (bgr[A], cam(A), bgr[B], cam(B), X)
    want = sgm_pipeline.match_pair(OracleBackend(), *args, min_resolution=0, seed_depth=seed)
    # the seed the pair was given, restated: Depth2DisparityMap of the half-size depth map -> the range
    r = rectify.stereo_rectify_geometry((bgr[A].shape[1], bgr[A].shape[0]), *cam(A), (bgr[B].shape[1], bgr[B].shape[0]), *cam(B),
                                        sgm_pipeline.world_to_image3(*cam(A), X), sgm_pipeline.world_to_image3(*cam(B), X))
    H2, Q2 = rectify.scale_stereo_rectification(r["H1"], r["Q"], 0.5)
    hw, hh = sgm_pipeline.compute_resize(r["size"], 0.5)
    init = OracleBackend().Depth2DisparityMap(depths[0], np.linalg.inv(H2), np.linalg.inv(Q2), 1, (hw - 6, hh - 6))
    assert want["seeded"] and tsgm.plain_range(init) == PIPELINE_RANGE and want["disparity"].shape == (r["size"][1] - 6, r["size"][0] - 6)
    assert (want["disparity"] != NO_DISP).mean() > 0.3
    host = sgm_pipeline.match_pair(sgm_pipeline.DeviceBackend(m, None, rectify_on_device=False), *args, min_resolution=0, seed_depth=seed)
    be = sgm_pipeline.DeviceBackend(m, None)
    be.scene_set_images(bgr)
    dev = sgm_pipeline.match_pair(be, *args, min_resolution=0, seed_depth=seed, image_ids=(A, B))
    be.scene_clear()
    for nm, got in (("host-rectified", host), ("device-rectified", dev)):
        for k in ("disparity", "cost", "H", "Q"):
            assert np.array_equal(got[k], want[k]), "%s route: %s" % (nm, k)
        assert got["seeded"] and got["image_size"] == want["image_size"]
