"""Pins oracle/pm_oracle.cpp to the REFERENCE'S OWN CODE: oracle/_ref is /root/reference's DepthEstimator (FillPixelPatch, ScorePixelImage, ScorePixel,
ProcessPixel, InterpolatePixel, CorrectNormal, InitPlane; DepthMap.cpp:415-971, DepthMap.h:276-468), its pass bodies (SceneDensify.cpp:490-576),
MapMatrix2ZigzagIdx, ViewData::Init, TImage::sample, Normal2Dir / Dir2Normal, TRMatrixBase::Set and SEACAVE::Random, cut verbatim from the reference's
files at build time and compiled against a minimal OpenCV / Eigen stand-in (oracle/ref/).  Same arrays into both sides, results compared BIT FOR BIT:

  * with exp / acos / atan2 / sin / cos routed to csrc/pm_math.h on the reference's side too (libref_pm.so) the oracle must reproduce the reference's
    code exactly -- algorithm, operation order, float / double mix, overload resolution, draw order (the reference's std::mt19937 stream, GCC's
    right-to-left argument evaluation = oracle rngMode 2);
  * with libm (libref_pm_libm.so, as a reference binary) the difference is what the pm_math.h substitution costs; it is bounded here in the units
    BASELINE.json's north_star states (depth RMSE over pixels valid in both <= 1e-4 x scene diameter is NOT expected of a chaotic estimator pixel by
    pixel, so the test reports the fraction of pixels that agree and bounds the median relative difference).

Since the end of round 3 the post-filters are in the verbatim set too: DepthMapsData::RemoveSmallSegments, GapInterpolation (SceneDensify.cpp:809-1045) and FilterDepthMap
(:1049-1299), and SemiGlobalMatcher's steps around Match -- ConsistencyCrossCheck, FilterByCost, ExtractMask, FlipDirection, UpscaleMask, RefineDisparityMap
(SemiGlobalMatcher.cpp:1446-1811); oracle/filter_oracle.cpp and oracle/sgm_post_oracle.cpp must equal them bit for bit (last groups of tests).

The libraries are built where /root/reference exists (oracle/ref/build_ref.py, by __graft_entry__.build()); elsewhere the prebuilt files are used and the
tests skip if there are none."""
import ctypes as C

import numpy as np
import pytest

from openmvs_amd import synth
from oracle import pyoracle as po
from oracle import pyref as pr

pytestmark = pytest.mark.skipif(not pr.available(), reason="oracle/_ref not built (needs /root/reference)")


def _eq(a, b, what):
    for x, y, nm in zip(a, b, ("depth", "normal", "conf")):
        same = (x == y) | (np.isnan(x) & np.isnan(y))
        assert same.all(), "%s: %s differs in %d of %d values (max abs %g)" % (what, nm, int((~same).sum()), x.size, float(np.nanmax(np.abs(x - y))))


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(5, 160, 120, n_src=4)


def _views(sc, v, n_src=None, depth_maps=None):
    ids = [v] + list(sc.neighbors[v])[:n_src]
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps=depth_maps)
    return ids, views, keep


def test_the_library_is_the_pm_math_build():
    assert pr.lib().ref_math_kind() == b"pm_math" and pr.lib("libm").ref_math_kind() == b"libm"


def test_zigzag_order_is_the_reference_function():
    for w, h, stride in ((37, 29, 16), (64, 64, 64), (130, 70, 64), (9, 200, 16)):
        a = np.zeros((w * h, 2), np.uint16); b = np.zeros((w * h, 2), np.uint16)
        po.lib().orc_zigzag(w, h, stride, a.ctypes.data_as(C.POINTER(C.c_uint16)))
        pr.lib().ref_zigzag(w, h, stride, b.ctypes.data_as(C.POINTER(C.c_uint16)))
        assert np.array_equal(a, b)


def test_view_constants_are_the_reference_init(scene):
    sc = scene
    ids, views, keep = _views(sc, 0, depth_maps={i: np.ones((8, 8), np.float32) for i in range(sc.n_views)})
    for k in range(1, len(ids)):
        outs = []
        for fn in (po.lib().orc_view_init, pr.lib().ref_view_init):
            Hl = np.zeros(9); Hm = np.zeros(3); Hr = np.zeros(9); Tl = np.zeros(9, np.float32); Tm = np.zeros(3, np.float32); Tr = np.zeros(9, np.float32); Tn = np.zeros(3, np.float32)
            dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            fn(C.byref(views[0]), C.byref(views[k]), dp(Hl), dp(Hm), dp(Hr), fp(Tl), fp(Tm), fp(Tr), fp(Tn))
            outs.append((Hl, Hm, Hr, Tl, Tm, Tr, Tn))
        for a, b, nm in zip(outs[0], outs[1], ("Hl", "Hm", "Hr", "Tl", "Tm", "Tr", "Tn")):
            assert np.array_equal(a, b), nm


@pytest.mark.parametrize("seed_view", [(3, 0), (11, 2), (29, 4)])
def test_photometric_level_is_bit_identical(scene, seed_view):
    sc = scene; seed, v = seed_view
    ids, views, keep = _views(sc, v)
    h, w = sc.gray[0].shape
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    opt = po.default_opt(seed=seed, viewID=v, rngMode=2)
    args = (views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt)
    init_a = pr.orc_run_level(*args, True, 0, 0); init_b = pr.ref_run_level(*args, True, 0, 0)
    _eq(init_a, init_b, "init pass")
    a = pr.orc_run_level(*args, True, 0, 3, th_end=0.9 * 1.333); b = pr.ref_run_level(*args, True, 0, 3, th_end=0.9 * 1.333)
    _eq(a, b, "init + 3 sweeps + end")
    assert (a[0] > 0).mean() > 0.7
    # the comparison is not vacuous: the left-to-right draw order (rngMode 1) is a different stream
    c = pr.orc_run_level(views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), po.default_opt(seed=seed, viewID=v, rngMode=1), True, 0, 1)
    d = pr.ref_run_level(*args, True, 0, 1)
    assert (c[0] != d[0]).mean() > 0.3


@pytest.mark.parametrize("n_src", [1, 2, 3])
def test_source_counts(scene, n_src):
    sc = scene; v = 1
    ids, views, keep = _views(sc, v, n_src)
    h, w = sc.gray[0].shape
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    opt = po.default_opt(rngMode=2)
    args = (views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, 2, 0.9)
    _eq(pr.orc_run_level(*args), pr.ref_run_level(*args), "%d source view(s)" % n_src)


def _photometric(sc, v, opt, iters=2):
    ids, views, keep = _views(sc, v)
    h, w = sc.gray[0].shape
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    return pr.orc_run_level(views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, iters, th_end=0.9 * 1.333)


def test_geometric_round_with_neighbour_depth_maps(scene):
    """The consistency term (DepthMap.cpp:535-551): functor-bilinear sample of the neighbour's depth map, back-projection, norm(Point2f) -- the call that
    binds to SEACAVE::norm (float), which round 3's first comparison showed the oracle had restated in double."""
    sc = scene
    opt = po.default_opt(rngMode=2)
    maps = {u: _photometric(sc, u, opt) for u in range(sc.n_views)}
    for v in (0, 3):
        ids, views, keep = _views(sc, v, depth_maps={u: maps[u][0] for u in range(sc.n_views)})
        d, n, c = maps[v]
        for it in (3, 4):
            args = (views, len(ids), d, n, c, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, it, it + 1, 0.9)
            a = pr.orc_run_level(*args); b = pr.ref_run_level(*args)
            _eq(a, b, "geometric round, view %d, iteration %d" % (v, it))
            d, n, c = a


@pytest.mark.parametrize("case", ["behind", "twin", "twin_shift", "edge_on"])
def test_adversarial_cameras_of_the_tap_fallback_cases(case):
    """The cameras of tests/tap_fallback_cases.py: a source that looks the other way (every tap has z <= 0; ScorePixelImage has no z test and samples such a tap when x / z
    lands in the image), twins of the reference whose taps land exactly on the edge of the border band, a planted plane whose picture is the band's edge itself.  What the
    oracle restates for them -- and the kernels' fallbacks are compared with -- is the reference's own behaviour: init pass, then init + 3 sweeps + end."""
    from tests import tap_fallback_cases as tc
    c = tc.inputs(case)
    views, keep = po.make_views(c["gray"], c["K"], c["R"], c["C"], c["ids"])
    z = np.zeros((tc.H, tc.W), np.float32)
    d0 = z if c["depth"] is None else c["depth"]; n0 = np.zeros((tc.H, tc.W, 3), np.float32) if c["normal"] is None else c["normal"]
    args = (views, len(c["ids"]), d0, n0, z, c["dmin"], c["dmax"], po.default_opt(seed=tc.SEED, viewID=c["ref"], rngMode=2))
    _eq(pr.orc_run_level(*args, True, 0, 0), pr.ref_run_level(*args, True, 0, 0), "%s: init pass" % case)
    a = pr.orc_run_level(*args, True, 0, 3, th_end=0.9 * 1.333); b = pr.ref_run_level(*args, True, 0, 3, th_end=0.9 * 1.333)
    _eq(a, b, "%s: init + 3 sweeps + end" % case)
    assert (a[0] > 0).mean() > 0.5


def test_low_resolution_prior_and_mask(scene):
    sc = scene; v = 2
    opt = po.default_opt(rngMode=2)
    d, n, c = _photometric(sc, v, opt)
    ids, views, keep = _views(sc, v)
    h, w = d.shape
    prior = d.copy(); prior[::7, ::5] = 0                       # holes in the prior: those pixels fall back to the texture test
    args = (views, len(ids), d, n, np.zeros_like(c), float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, 2)
    _eq(pr.orc_run_level(*args, prior=prior), pr.ref_run_level(*args, prior=prior), "low-resolution prior")
    mask = np.ones((h, w), np.uint8); mask[30:60, 40:100] = 0; mask[::9, ::4] = 0
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    args = (views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, 2, 0.9)
    a = pr.orc_run_level(*args, mask=mask); b = pr.ref_run_level(*args, mask=mask)
    _eq(a, b, "ignore mask")
    assert (a[0][mask == 0] == 0).all()


@pytest.mark.parametrize("k", range(4))
def test_non_default_options(scene, k):
    sc = scene; v = 0
    kw = [dict(nRandomIters=3, fRandomSmoothBonus=0.8), dict(fNCCThresholdKeep=0.7, fRandomDepthRatio=0.01), dict(fRandomAngle1Range=30.0, fRandomAngle2Range=20.0, fRandomSmoothNormal=25.0),
          dict(fDescriptorMinMagnitudeThreshold=0.0, fRandomSmoothDepth=0.05, nRandomIters=9)][k]
    opt = po.default_opt(rngMode=2, **kw)
    ids, views, keep = _views(sc, v)
    h, w = sc.gray[0].shape
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    args = (views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, 2, opt.fNCCThresholdKeep)
    _eq(pr.orc_run_level(*args), pr.ref_run_level(*args), str(kw))


def test_adversarial_start_exercises_correct_normal_and_random_restarts(scene):
    """Start from noise: grazing and back-facing normals, depths at the range ends, costs that force the random-restart branch -- CorrectNormal's
    axis-angle rotation (DepthMap.h:447-453, Rotation.inl:701-728), InterpolatePixel's fallbacks and the `goto RefineIters` path all run."""
    sc = scene; v = 3
    rng = np.random.RandomState(5)
    h, w = sc.gray[0].shape
    dmin, dmax = float(sc.dmin[v]), float(sc.dmax[v])
    depth = rng.uniform(dmin * 0.9, dmax * 1.1, (h, w)).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, (h, w)); ph = rng.uniform(np.pi * 0.45, np.pi, (h, w))
    normal = np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], -1).astype(np.float32)
    conf = rng.uniform(0, 2, (h, w)).astype(np.float32)
    ids, views, keep = _views(sc, v)
    opt = po.default_opt(rngMode=2)
    for it in (0, 1):
        args = (views, len(ids), depth, normal, conf, dmin, dmax, opt, it == 0, it, it + 1)
        a = pr.orc_run_level(*args); b = pr.ref_run_level(*args)
        _eq(a, b, "noise start, iteration %d" % it)
        depth, normal, conf = a


def test_pixel_helpers_and_scores_on_random_planes(scene):
    """Unit level: InterpolatePixel, CorrectNormal and ScorePixel (all per-view scores) for random pixels, neighbours and planes."""
    sc = scene; v = 0
    ids, views, keep = _views(sc, v)
    rng = np.random.RandomState(17)
    h, w = sc.gray[0].shape
    opt = po.default_opt(rngMode=2)
    lo, lr = po.lib(), pr.lib()
    lo.orc_pixel_helpers.restype = C.c_int; lr.ref_pixel_helpers.restype = C.c_int; lr.ref_score_pixel.restype = C.c_int
    dmin, dmax = float(sc.dmin[v]), float(sc.dmax[v])
    nfix = 0
    for trial in range(400):
        x, y = int(rng.randint(4, w - 4)), int(rng.randint(4, h - 4))
        dx, dy = [(1, 0), (-1, 0), (0, 1), (0, -1)][trial % 4]
        nx, ny = min(max(x + dx, 4), w - 5), min(max(y + dy, 4), h - 5)
        if (nx, ny) == (x, y):
            continue
        nd = float(rng.uniform(dmin, dmax))
        t, p = rng.uniform(0, 2 * np.pi), rng.uniform(np.pi * 0.5, np.pi)
        nn = np.array([np.cos(t) * np.sin(p), np.sin(t) * np.sin(p), np.cos(p)], np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        oi = C.c_float(); oc = np.zeros(3, np.float32); osf = C.c_float(); ri = C.c_float(); rc_ = np.zeros(3, np.float32)
        assert lo.orc_pixel_helpers(views, len(ids), C.byref(opt), x, y, C.c_float(dmin), C.c_float(dmax), nx, ny, C.c_float(nd), fp(nn), C.c_float(nd), fp(nn), C.byref(oi), fp(oc), C.byref(osf)) == 0
        assert lr.ref_pixel_helpers(views, len(ids), C.byref(opt), x, y, C.c_float(dmin), C.c_float(dmax), nx, ny, C.c_float(nd), fp(nn), C.byref(ri), fp(rc_)) == 0
        assert oi.value == ri.value, "InterpolatePixel at %s" % ((x, y, nx, ny),)
        assert np.array_equal(oc, rc_), "CorrectNormal at %s: %s vs %s" % ((x, y), oc, rc_)
        nfix += int(not np.array_equal(oc, nn))
        so = np.zeros(len(ids) - 1, np.float32); sr = np.zeros(len(ids) - 1, np.float32); ao = C.c_float(); ar = C.c_float()
        r1 = lo.orc_score_pixel(views, len(ids), C.byref(opt), x, y, C.c_float(nd), fp(oc), None, fp(so), C.byref(ao))
        r2 = lr.ref_score_pixel(views, len(ids), C.byref(opt), x, y, C.c_float(nd), fp(oc), None, fp(sr), C.byref(ar))
        assert r1 == r2
        if r1 == 0:
            assert ao.value == ar.value and np.array_equal(np.sort(so), np.sort(sr)), "ScorePixel at %s" % ((x, y),)
    assert nfix > 20, "CorrectNormal was hardly exercised (%d)" % nfix


def test_libm_build_bounds_the_pm_math_substitution(scene):
    """The reference binary uses libm; the product and the oracle use csrc/pm_math.h (<= 1-3 ulp from libm).  One flipped accept decision changes how
    many numbers a pixel draws from the estimator's sequential std::mt19937, so from that pixel on the two runs see different random streams: maps of
    the two builds of the REFERENCE'S OWN code differ pixel by pixel at the level of the refinement noise -- exactly as two runs of the reference
    binary do (release builds seed from random_device).  What must hold, and is checked: the same pixels survive, the difference is
    at the noise level, and both builds are equally close to the ground truth."""
    sc = scene; v = 0
    ids, views, keep = _views(sc, v)
    h, w = sc.gray[0].shape
    z = np.zeros((h, w), np.float32); n0 = np.zeros((h, w, 3), np.float32)
    opt = po.default_opt(rngMode=2)
    args = (views, len(ids), z, n0, z, float(sc.dmin[v]), float(sc.dmax[v]), opt, True, 0, 3, 0.9)
    a = pr.ref_run_level(*args, kind="pm_math"); b = pr.ref_run_level(*args, kind="libm")
    both = (a[0] > 0) & (b[0] > 0)
    assert both.mean() > 0.7 and abs(int((a[0] > 0).sum()) - int((b[0] > 0).sum())) < 0.01 * both.sum()
    rel = np.abs(a[0][both] - b[0][both]) / b[0][both]
    assert np.median(rel) < 1e-3 and np.percentile(rel, 90) < 5e-3, (float(np.median(rel)), float(np.percentile(rel, 90)))
    gt = sc.gt_depth[v]
    ea = np.median(np.abs(a[0][both] - gt[both]) / gt[both]); eb = np.median(np.abs(b[0][both] - gt[both]) / gt[both])
    assert abs(ea - eb) < 0.25 * max(ea, eb), (float(ea), float(eb))
    rmse = float(np.sqrt(np.mean((a[0][both].astype(np.float64) - b[0][both]) ** 2))) / sc.diameter
    assert rmse < 2e-3, rmse        # 5e-4 x diameter on this 160x120 level after three sweeps: the estimator's own run-to-run noise, not a bias


# ---- SemiGlobalMatcher::Match (SemiGlobalMatcher.cpp:863-1302): cost volume, 8-path aggregation (threaded variant), winner-take-all -----------------
def _hand_built_families():
    """the families of tests/sgm_match_edge_cases.py inside the reference's domain (grey values in [0, 1], P1 <= P2, sums that fit 16 bits): the oracle is pinned where the
    buffer edges, the packing, the ties and the penalty lookup decide, and not only the engine"""
    from tests import sgm_match_edge_cases as ec
    return sorted(f for f, (_, inside) in ec.FAMILIES.items() if inside)


@pytest.mark.skipif(not pr.sgm_available(), reason="oracle/_ref/libref_sgm.so not built")
@pytest.mark.parametrize("case", [(80, 60, 5, "uniform", 0, 16), (120, 90, 7, "ragged", 0, 24), (200, 150, 9, "holes", -4, 20), (96, 64, 3, "uniform", -8, 8), (160, 120, 11, "ragged", 0, 64)]
                         + _hand_built_families())
def test_sgm_match_is_the_reference_function(case):
    from tests import sgm_cases as scs
    if isinstance(case, str):
        from tests import sgm_match_edge_cases as ec
        for p in ec.problems(case):
            want = ec.prove(p)
            for route, table in p.tables().items():
                b = pr.ref_sgm_match(p.bgr, p.gl, p.gr, p.px, p.n, p.mxd, p.P1, table)
                for x, y, nm in zip(want[route], b, ec.NAMES):
                    assert np.array_equal(x, y), "%s, %s route: %s: %d differ" % (p.name, route, nm, int((x != y).sum()))
        return
    w, h, shift, kind, lo, hi = case
    lb, lg, rg = scs.stereo_pair(w, h, shift, seed=3)
    px, n, mx = scs.ranges(w, h, kind, lo, hi)
    assert np.array_equal(po.sgm_generate_p2s(), pr.ref_sgm_generate_p2s())          # GenerateP2s, :516-524
    P2s = po.sgm_generate_p2s()
    a = po.sgm_match(lb, lg, rg, px, n, mx, 3, P2s); b = pr.ref_sgm_match(lb, lg, rg, px, n, mx, 3, P2s)
    for x, y, nm in zip(a, b, ("disparity", "cost", "cost volume", "accumulated sums")):
        assert np.array_equal(x, y), nm


# ---- the two per-map post-filters: DepthMapsData::RemoveSmallSegments / GapInterpolation (SceneDensify.cpp:809-1045) ----------------------------
def _noisy_maps(seed, w=160, h=120):
    """Depth / normal / confidence maps with what the two filters react to: terraces right at the similarity threshold (one-directional edges: IsDepthSimilar
    is not symmetric), small islands, holes of 1-10 pixels in rows and columns, zero-confidence pixels."""
    r = np.random.RandomState(seed)
    th = 0.007
    lv = (2.0 * (1 + th) ** (r.randint(0, 6, (h, w)) * r.choice([0.97, 1.0, 1.03]))).astype(np.float32)
    blk = np.kron(r.rand(h // 4, w // 4) < 0.5, np.ones((4, 4), bool))
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.where(blk, lv, (2.0 + 0.002 * xx + 0.001 * yy)).astype(np.float32)
    d[r.rand(h, w) < 0.12] = 0
    for _ in range(40):                                           # gaps of controlled length along rows and columns
        y0, x0, L = r.randint(0, h), r.randint(0, w - 12), r.randint(1, 11)
        d[y0, x0:x0 + L] = 0
        y1, x1 = r.randint(0, h - 12), r.randint(0, w)
        d[y1:y1 + L, x1] = 0
    n = np.zeros((h, w, 3), np.float32)
    ang = r.rand(h, w).astype(np.float32) * 0.5
    n[..., 0] = np.sin(ang) * 0.3; n[..., 1] = np.sin(ang) * 0.2; n[..., 2] = -np.sqrt(np.maximum(0, 1 - n[..., 0] ** 2 - n[..., 1] ** 2))
    n[d == 0] = 0
    c = np.where(d > 0, r.rand(h, w), 0).astype(np.float32)
    return d, n, c


@pytest.mark.parametrize("seed,speckle,th", [(1, 40, 0.007), (2, 100, 0.01), (3, 10, 0.02), (4, 400, 0.005)])
def test_remove_small_segments_is_the_reference_function(seed, speckle, th):
    d, n, c = _noisy_maps(seed)
    a = po.remove_small_segments(d, n, c, nSpeckleSize=speckle, fDepthDiffThreshold=th)
    b = pr.ref_remove_small_segments(d, n, c, nSpeckleSize=speckle, fDepthDiffThreshold=th)
    _eq(a, b, "RemoveSmallSegments")
    assert ((d > 0) & (a[0] == 0)).sum() > 50 and (a[0] > 0).sum() > 1000      # it removed something and kept something


@pytest.mark.parametrize("seed,gap,th", [(5, 7, 0.01), (6, 3, 0.007), (7, 12, 0.02), (8, 1, 0.01)])
def test_gap_interpolation_is_the_reference_function(seed, gap, th):
    d, n, c = _noisy_maps(seed)
    a = po.gap_interpolation(d, n, c, nIpolGapSize=gap, fDepthDiffThreshold=th)
    b = pr.ref_gap_interpolation(d, n, c, nIpolGapSize=gap, fDepthDiffThreshold=th)
    _eq(a, b, "GapInterpolation")
    assert ((d == 0) & (a[0] > 0)).sum() > (20 if gap > 1 else 0)               # it filled something


# The adversarial maps of tests/post_filter_cases.py are judged by the oracle alone on the emulator and on the device: what it does with NaN, +inf and negative
# depths, with gaps on a border and with chains of one-directional edges has to be what the reference's own text does.
@pytest.mark.parametrize("size", [(67, 37), (3, 70), (70, 3)], ids=lambda s: "%dx%d" % s)
def test_remove_small_segments_on_adversarial_maps_is_the_reference_function(size):
    from tests import post_filter_cases as cases
    n = 0
    for fth in cases.SEGMENT_THRESHOLDS:
        for k, (name, d, claim) in enumerate(cases.segment_maps(size[0], size[1], fth)):
            nrm, cnf = cases.normals_and_conf(d, 100 + k)
            for sz in cases.SPECKLE_SIZES:
                a = po.remove_small_segments(d, nrm, cnf, nSpeckleSize=sz, fDepthDiffThreshold=fth)
                b = pr.ref_remove_small_segments(d, nrm, cnf, nSpeckleSize=sz, fDepthDiffThreshold=fth)
                cases.same(a, b, "RemoveSmallSegments %s nSpeckleSize %d fDepthDiffThreshold %g" % (name, sz, fth))
                n += 1
    assert n >= 11 * 7 * 2


@pytest.mark.parametrize("size", [(67, 37), (3, 70), (70, 3)], ids=lambda s: "%dx%d" % s)
def test_gap_interpolation_on_adversarial_maps_is_the_reference_function(size):
    from tests import post_filter_cases as cases
    for trial in range(30):
        d, nrm, cnf, exact, steps = cases.gap_map(size[0], size[1], trial)
        for gap in cases.GAP_SIZES:
            for fth in cases.GAP_THRESHOLDS:
                a = po.gap_interpolation(d, nrm, cnf, nIpolGapSize=gap, fDepthDiffThreshold=fth)
                b = pr.ref_gap_interpolation(d, nrm, cnf, nIpolGapSize=gap, fDepthDiffThreshold=fth)
                cases.same(a, b, "GapInterpolation map %d nIpolGapSize %d fDepthDiffThreshold %g" % (trial, gap, fth))


# ---- the cross-view filter: DepthMapsData::FilterDepthMap (SceneDensify.cpp:1049-1299) -----------------------------------------------------------
@pytest.fixture(scope="module")
def estimated(scene):
    """Depth / confidence maps of all views of the module's scene as the oracle estimates them (photometric pass), plus a disturbed copy: noise of the size of the
    filter's thresholds, outliers in front of and behind the surface, holes -- what makes the filter average, penalise, keep and discard."""
    sc = scene
    depths, confs = {}, {}
    for v in range(sc.n_views):
        ids, views, keep = _views(sc, v)
        d, n, c = po.estimate_depth_map(views, len(ids), float(sc.dmin[v]), float(sc.dmax[v]), po.default_opt(seed=2, viewID=v))
        depths[v] = d; confs[v] = c
    r = np.random.RandomState(3)
    nd, nc = {}, {}
    for v in range(sc.n_views):
        d = depths[v].copy(); c = confs[v].copy()
        m = d > 0
        d[m] *= (1 + r.normal(0, 0.006, d.shape)[m]).astype(np.float32)
        out = m & (r.rand(*d.shape) < 0.06)
        d[out] *= r.choice(np.float32([0.8, 0.93, 1.08, 1.3]), d.shape)[out]
        hole = r.rand(*d.shape) < 0.05
        d[hole] = 0; c[hole] = 0
        c[m & ~hole] = np.maximum(c[m & ~hole], np.float32(0.01))
        nd[v] = d.astype(np.float32); nc[v] = c.astype(np.float32)
    return depths, confs, nd, nc


@pytest.mark.parametrize("bAdjust", [True, False])
@pytest.mark.parametrize("variant", ["estimated", "disturbed"])
@pytest.mark.parametrize("ref,nMinViews,nMinAdjust,th", [(0, 2, 1, 0.01), (2, 3, 2, 0.007), (4, 1, 1, 0.02)])
def test_filter_depth_map_is_the_reference_function(scene, estimated, bAdjust, variant, ref, nMinViews, nMinAdjust, th):
    sc = scene
    depths, confs, nd, nc = estimated
    D, Cf = (depths, confs) if variant == "estimated" else (nd, nc)
    nbs = [int(i) for i in sc.neighbors[ref]]
    assert (D[ref][0] == 0).all() and (D[ref][:, 0] == 0).all() and (D[ref][-1] == 0).all() and (D[ref][:, -1] == 0).all()   # (empty border: the reference's neighbour reads stay inside)
    kw = dict(bAdjust=bAdjust, nMinViewsFilter=nMinViews, nMinViewsFilterAdjust=nMinAdjust, fDepthDiffThreshold=th)
    a = po.filter_depth_map(D, Cf, sc.K, sc.R, sc.C, ref, nbs, float(sc.dmin[ref]), float(sc.dmax[ref]), **kw)
    b = pr.ref_filter_depth_map(D, Cf, sc.K, sc.R, sc.C, ref, nbs, float(sc.dmin[ref]), float(sc.dmax[ref]), **kw)
    assert a[0] == b[0] == 0
    for x, y, nm in zip(a[1:], b[1:], ("depth", "conf")):
        assert np.array_equal(x, y), "FilterDepthMap %s: %d of %d differ" % (nm, int((x != y).sum()), x.size)
    kept = (a[1] > 0).sum(); had = (D[ref] > 0).sum()
    assert 0 < kept <= had
    if variant == "disturbed":
        assert kept < had                                              # it discarded something


def _resized_view(depth, conf, K, fx, fy):
    """A depth / confidence map at another size (nearest resampling: depths stay depths) with the camera scaled like Camera::ScaleK does."""
    h, w = depth.shape
    nw, nh = int(round(w * fx)), int(round(h * fy))
    xs = np.minimum((np.arange(nw) * (w / nw)).astype(int), w - 1); ys = np.minimum((np.arange(nh) * (h / nh)).astype(int), h - 1)
    Kn = np.array(K, np.float64).copy()
    sx, sy = nw / w, nh / h
    Kn[0, 0] *= sx; Kn[1, 1] *= sy; Kn[0, 2] = (Kn[0, 2] + 0.5) * sx - 0.5; Kn[1, 2] = (Kn[1, 2] + 0.5) * sy - 0.5
    return np.ascontiguousarray(depth[ys][:, xs]), np.ascontiguousarray(conf[ys][:, xs]), Kn


@pytest.mark.parametrize("bAdjust", [True, False])
@pytest.mark.parametrize("ref", [0, 4])
def test_filter_depth_map_with_neighbours_of_other_sizes_is_the_reference_function(scene, estimated, bAdjust, ref):
    """The reference sizes every depth map on its own image (DepthMapsData::InitViews, SceneDensify.cpp:306-459); FilterDepthMap walks each neighbour's map at the
    neighbour's size (:1085) and tests free-space violations inside the neighbour's confidence map (:1181)."""
    sc = scene
    depths, confs, nd, nc = estimated
    nbs = [int(i) for i in sc.neighbors[ref]]
    D, Cf, K = dict(nd), dict(nc), [np.array(k, np.float64) for k in sc.K]
    for k, j in enumerate(nbs):
        fx, fy = [(0.75, 0.75), (1.25, 1.25), (1.0, 0.5), (1.4, 0.8)][k % 4]
        if k % 5 != 4:
            D[j], Cf[j], K[j] = _resized_view(nd[j], nc[j], sc.K[j], fx, fy)
    assert len({D[j].shape for j in nbs}) >= 3
    kw = dict(bAdjust=bAdjust, nMinViewsFilter=2, nMinViewsFilterAdjust=1, fDepthDiffThreshold=0.01)
    a = po.filter_depth_map(D, Cf, K, sc.R, sc.C, ref, nbs, float(sc.dmin[ref]), float(sc.dmax[ref]), **kw)
    b = pr.ref_filter_depth_map(D, Cf, K, sc.R, sc.C, ref, nbs, float(sc.dmin[ref]), float(sc.dmax[ref]), **kw)
    assert a[0] == b[0] == 0
    for x, y, nm in zip(a[1:], b[1:], ("depth", "conf")):
        assert np.array_equal(x, y), "FilterDepthMap %s: %d of %d differ" % (nm, int((x != y).sum()), x.size)
    assert 0 < (a[1] > 0).sum() < (D[ref] > 0).sum()


def test_filter_depth_map_refuses_too_few_neighbours(scene, estimated):
    sc = scene; depths, confs, nd, nc = estimated
    a = po.filter_depth_map(depths, confs, sc.K, sc.R, sc.C, 0, [1], 1.0, 10.0, nMinViewsFilter=2)
    b = pr.ref_filter_depth_map(depths, confs, sc.K, sc.R, sc.C, 0, [1], 1.0, 10.0, nMinViewsFilter=2)
    assert a[0] == b[0] == 1


# ---- the steps around Match: ConsistencyCrossCheck, FilterByCost, ExtractMask, UpscaleMask, FlipDirection, RefineDisparityMap (SemiGlobalMatcher.cpp:1446-1811) ----
sgm_only = pytest.mark.skipif(not pr.sgm_available(), reason="oracle/_ref/libref_sgm.so not built")
NO_DISP = np.iinfo(np.int16).max          # SemiGlobalMatcher.h: NO_DISP = DECLARE_NO_INDEX(Disparity) = the type's maximum


def _disp_maps(seed, w=97, h=61):
    r = np.random.RandomState(seed)
    base = (r.randint(-12, 13, (h, 1)) + r.randint(-2, 3, (h, w))).astype(np.int16)
    l2r = base.copy(); r2l = (-np.roll(base, 3, axis=1) + r.randint(-1, 2, (h, w))).astype(np.int16)
    l2r[r.rand(h, w) < 0.15] = NO_DISP; r2l[r.rand(h, w) < 0.15] = NO_DISP
    l2r[:, :r.randint(1, 6)] = NO_DISP                                # invalid margins, as a matcher leaves them
    cost = r.randint(0, 2000, (h, w)).astype(np.uint16)
    return l2r, r2l, cost


@sgm_only
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sgm_steps_are_the_reference_functions(seed):
    L = pr.sgm_post_lib(); kw = dict(impl=L, prefix="ref_sgm_")
    l2r, r2l, cost = _disp_maps(seed)
    for th in (0, 1, 2):
        assert np.array_equal(po.sgm_cross_check(l2r, r2l, th), po.sgm_cross_check(l2r, r2l, th, **kw)), "ConsistencyCrossCheck"
    narrow = r2l[:, :80]                                              # maps of different widths (rectified pairs are)
    assert np.array_equal(po.sgm_cross_check(l2r, narrow, 1), po.sgm_cross_check(l2r, narrow, 1, **kw))
    for th in (300, 1200):
        assert np.array_equal(po.sgm_filter_by_cost(l2r, cost, th), po.sgm_filter_by_cost(l2r, cost, th, **kw)), "FilterByCost"
    for tv in (1, 3, 6):
        m0 = po.sgm_extract_mask(l2r, None, tv); m1 = po.sgm_extract_mask(l2r, None, tv, **kw)
        assert np.array_equal(m0, m1), "ExtractMask (fresh mask)"
        assert np.array_equal(po.sgm_extract_mask(r2l, m0, tv), po.sgm_extract_mask(r2l, m0, tv, **kw)), "ExtractMask (given mask)"
        for size2x in ((2 * l2r.shape[1] + 6, 2 * l2r.shape[0] + 6), (2 * l2r.shape[1] + 7, 2 * l2r.shape[0] + 5)):
            assert np.array_equal(po.sgm_upscale_mask(m0, size2x), po.sgm_upscale_mask(m0, size2x, **kw)), "UpscaleMask"
    assert np.array_equal(po.sgm_flip_direction(l2r), po.sgm_flip_direction(l2r, **kw)), "FlipDirection"


@sgm_only
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5, 6])
def test_sgm_refine_is_the_reference_function(mode):
    from tests import sgm_cases as scs
    w, h = 96, 64
    lb, lg, rg = scs.stereo_pair(w, h, 5, seed=11)
    px, n, mx = scs.ranges(w, h, "ragged", -6, 20, seed=4)
    P2s = po.sgm_generate_p2s()
    d, c, costs, acc = po.sgm_match(lb, lg, rg, px, n, mx, 3, P2s)
    for steps in (1, 4, 7):
        a = po.sgm_refine(d, px, acc, mode=mode, steps=steps); b = pr.ref_sgm_refine(d, px, acc, mode=mode, steps=steps)
        assert np.array_equal(a, b), "RefineDisparityMap mode %d steps %d: %d of %d differ" % (mode, steps, int((a != b).sum()), a.size)


# ---- the SGM conversions around the matcher: Disparity2RangeMap (SemiGlobalMatcher.cpp:1350-1444), Depth2DisparityMap, Disparity2DepthMap, ProjectDisparity2DepthMap
#      (:1837-2039) with Image::Disparity2Depth / Depth2Disparity (Image.cpp:372-433), TImage::sampleSafe, ProjectVertex_3x3_2_2, TAccumulator: cut verbatim ----
@sgm_only
@pytest.mark.parametrize("w,h,seed", [(64, 40, 0), (97, 53, 1), (131, 77, 2)])
def test_sgm_range_map_is_the_reference_function(w, h, seed):
    from tests import sgm_post_cases as pc
    kw = dict(impl=pr.sgm_post_lib(), prefix="ref_sgm_")
    d = pc.smooth_disparity(w, h, seed)
    for extra in ((7, 6), (6, 7)):
        mask = pc.mask_map(2 * w + extra[0], 2 * h + extra[1], seed)
        for a, b in ((11, 33), (5, 7), (3, 16)):
            px0, n0, m0 = po.sgm_disparity2range_map(d, mask, a, b)
            px1, n1, m1 = po.sgm_disparity2range_map(d, mask, a, b, **kw)
            assert n0 == n1 and m0 == m1, (n0, n1, m0, m1)
            for k in ("idx", "minDisp", "maxDisp"):
                assert np.array_equal(px0[k], px1[k]), k


@sgm_only
@pytest.mark.parametrize("w,h,seed", [(64, 40, 0), (97, 53, 1)])
def test_sgm_disparity_depth_conversions_are_the_reference_functions(w, h, seed):
    from tests import sgm_post_cases as pc
    kw = dict(impl=pr.sgm_post_lib(), prefix="ref_sgm_")
    H, Q, iH, iQ = pc.rectification(seed)
    depth = (3.0 + 0.5 * np.sin(np.arange(h * w).reshape(h, w) / 50.0)).astype(np.float32)
    depth[np.random.RandomState(seed).rand(h, w) < 0.2] = 0
    cost = pc.cost_map(w - 6, h - 6, seed)
    for steps in (1, 4):
        a = po.sgm_depth2disparity_map(depth, iH, iQ, steps, (w - 6, h - 6))
        assert np.array_equal(a, po.sgm_depth2disparity_map(depth, iH, iQ, steps, (w - 6, h - 6), **kw)), "Depth2DisparityMap"
        assert (a != NO_DISP).mean() > 0.5
        for cst in (None, cost):
            da, ca = po.sgm_disparity2depth_map(a, cst, H, Q, steps, (w, h))
            db, cb = po.sgm_disparity2depth_map(a, cst, H, Q, steps, (w, h), **kw)
            assert np.array_equal(da.view(np.uint32), db.view(np.uint32)), "Disparity2DepthMap depth"
            assert cst is None or np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), "Disparity2DepthMap confidence"
        disp = po.sgm_depth2disparity_map(depth, np.eye(3), iQ, steps, (w - 6, h - 6))
        for cst in (None, cost):
            ok0, d0, r0, c0 = po.sgm_project_disparity2depth_map(disp, cst, Q, steps, (w, h))
            ok1, d1, r1, c1 = po.sgm_project_disparity2depth_map(disp, cst, Q, steps, (w, h), **kw)
            assert ok0 == ok1 and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), "ProjectDisparity2DepthMap depth"
            valid = d0 > 0                                    # (the reference leaves the range / confidence of a pixel without a depth unset)
            assert np.array_equal(r0[valid].view(np.uint32), r1[valid].view(np.uint32)), "ProjectDisparity2DepthMap range"
            assert cst is None or np.array_equal(c0[valid].view(np.uint32), c1[valid].view(np.uint32)), "ProjectDisparity2DepthMap confidence"
            assert valid.mean() > 0.3


# ---- SemiGlobalMatcher::Fuse, the per-pixel cluster fusion over the maps of ProjectDisparity2DepthMap (SemiGlobalMatcher.cpp:795-848 with PairData :744-749, cut verbatim;
#      cList's initializer-list constructor and GetMax(functor) as List.h:1396, :688-691) ----
@sgm_only
@pytest.mark.parametrize("w,h,seed,n_pairs", [(64, 40, 0, 4), (97, 53, 1, 3), (80, 60, 2, 6), (33, 21, 3, 1)])
def test_sgm_pair_fusion_is_the_reference_loop(w, h, seed, n_pairs):
    from tests.test_sgm_post import _pair_maps
    kw = dict(impl=pr.sgm_post_lib(), prefix="ref_sgm_")
    base, deps, rgs, cfs = _pair_maps(w, h, seed, n_pairs)
    # ties between clusters and ranges that exclude their own depth (depth == upper bound: ISINSIDE is half-open) on a few pixels
    deps[0][0, :8] = 2.0; rgs[0][0, :8] = (1.9, 2.0)
    if n_pairs > 1:
        deps[1][0, :8] = 2.0; rgs[1][0, :8] = (2.0, 2.1)
    any_valid = 0
    for mv in (1, 2, 3, n_pairs + 1):
        a = po.sgm_fuse_pairs(deps, rgs, cfs, mv)
        b = po.sgm_fuse_pairs(deps, rgs, cfs, mv, **kw)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "Fuse depth, minViews %d" % mv
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "Fuse confidence, minViews %d" % mv
        any_valid += int((a[0] > 0).sum())
    assert any_valid > 0


# ---- the same steps on the hand-built maps of tests/sgm_post_edge_cases.py: the oracle equals the reference's own functions where contention, ties, int16 wraps and the
#      float -> int conversions decide.  The reference is built for x86, whose conversion gives INT_MIN for NaN and for everything outside int: that is what sgmp_f2i
#      (csrc/sgm_post.h, shared by the oracle) defines, so the hostile coordinates and disparities are pinned too.  Not compared: what the reference leaves unset (range and
#      confidence of ProjectDisparity2DepthMap where it produced no depth); NaN results by position only.  The speckle filter is OpenCV's: no reference function here. ----
def _edge_params():
    from tests import sgm_post_edge_cases as ec
    return [(f, s) for f in sorted(ec.FAMILIES) if f != "speckles" for s in (ec.SMALL,) + ec.THIN]


@sgm_only
@pytest.mark.parametrize("family,size", _edge_params(), ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else v)
def test_sgm_steps_on_hand_built_maps_are_the_reference_functions(family, size):
    from tests import sgm_post_edge_cases as ec
    assert ec.check_family(ec.Steps(pr.sgm_post_lib(), "ref_sgm_"), family, size, pin=True) > 0


@sgm_only
def test_sgm_refine_on_hand_built_sums_is_the_reference_function():
    from tests import sgm_post_edge_cases as ec
    px, acc, maps = ec.refine_synthetic()
    bgr, gray, px2, n, mxd, mn, mx, maps2 = ec.refine_problem(*ec.SMALL)
    acc2 = po.sgm_match(bgr, gray, gray, px2, n, mxd, 3, po.sgm_generate_p2s())[3]
    for table, sums, dmaps in ((px, acc, maps), (px2, acc2, maps2)):
        for name, d in dmaps.items():
            for mode in range(7):
                for steps in (1, 4, 64):
                    a = po.sgm_refine(d, table, sums, mode=mode, steps=steps); b = pr.ref_sgm_refine(d, table, sums, mode=mode, steps=steps)
                    assert np.array_equal(a, b), "RefineDisparityMap %s mode %d steps %d: %d of %d differ" % (name, mode, steps, int((a != b).sum()), a.size)
