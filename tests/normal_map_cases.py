"""MVS::EstimateNormalMap on the device (csrc/pm_normal.hip: pm_normal_map_kernel behind pmhip_estimate_normal_map and pmhip_scene_estimate_normals) at the sizes
and values at which it can go wrong, against `views.estimate_normal_map` -- and `oracle.pyref.ref_estimate_normal_map`, the reference's own function, where
oracle/_ref/libref_fuse.so is built -- on uint32 views: no tolerance anywhere.  Every case states on its own inputs, or on the host result, that it reaches its edge
(which counts of similar neighbours occur, on which side of the 3 % test a pair falls, that the stride loop takes a second trip), and that the host result is finite.
Shared by tests/test_emu_normal_map.py (wave64 emulator) and tests/test_zz_gpu_normal_map.py (device)."""
import numpy as np

from openmvs_amd import views

f32 = np.float32
u32 = np.uint32
TH = f32(0.03)
MAX_BLOCKS = 4096                  # PM_NORMAL_MAX_BLOCKS of csrc/pm_host_normal.hip, restated: one pass of the capped grid covers 4096 * 256 pixels
PASS = MAX_BLOCKS * 256
SENTINEL = f32(-7.25)              # a normal map before a scene call: a value no normal has

K0 = np.array([[220.0, 0, 79.5], [0, 220.0, 59.5], [0, 0, 1]])
K_ANISO = np.array([[301.7, 0, 31.25], [0, 187.3, 20.75], [0, 0, 1]])          # k00 != k11
K_OUTSIDE = np.array([[150.0, 0, -212.5], [0, 163.0, 977.25], [0, 0, 1]])      # principal point outside the image
KS = (K0, K_ANISO, K_OUTSIDE)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same_bits(got, want, what):
    assert got.dtype == f32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: %s vs %s" % (what, bad.size, want.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


_REF = None


def _ref():
    """oracle.pyref.ref_estimate_normal_map where the reference build exists, else None."""
    global _REF
    if _REF is None:
        from oracle import pyref
        _REF = pyref.ref_estimate_normal_map if pyref.fuse_available() else False
    return _REF or None


def host(K, depth, what=""):
    """The yardstick: `views.estimate_normal_map`, finite, and equal to the reference's own function where that is built."""
    want = views.estimate_normal_map(K, depth)
    assert np.isfinite(want).all(), "%s: the host result is not finite" % what
    if _ref() is not None:
        same_bits(_ref()(K, depth), want, what + ": the reference against the numpy statement")
    return want


def check(e, K, depth, what):
    """The host-buffer entry point on one map.  Returns (device result, host result)."""
    want = host(K, depth, what)
    got = e.estimate_normal_map(K, depth)
    same_bits(got, want, what)
    return got, want


# ---- a literal walk of the neighbourhood test, for the predicates ------------------------------------------------------------------------------------
def similar_counts(depth):
    """How many neighbours pass `di > 0 and fabsf(d - di) / d < 0.03f` at every pixel with d > 0 (-1 elsewhere), pixel by pixel in float32."""
    d = np.ascontiguousarray(depth, f32)
    H, W = d.shape
    out = np.full((H, W), -1, np.int64)
    with np.errstate(all="ignore"):
        for r in range(H):
            for c in range(W):
                if not d[r, c] > 0:
                    continue
                n = 0
                for y in (-1, 0, 1):
                    for x in (-1, 0, 1):
                        if (x or y) and 0 <= r + y < H and 0 <= c + x < W:
                            di = d[r + y, c + x]
                            n += bool(di > 0 and f32(np.abs(f32(d[r, c] - di))) / d[r, c] < TH)
                out[r, c] = n
    return out


def ratio(d, di):
    with np.errstate(all="ignore"):
        return f32(np.abs(f32(f32(d) - f32(di)))) / f32(d)


# ---- sources -----------------------------------------------------------------------------------------------------------------------------------------
def surface(rng, h, w, scale=1.0, noise=2e-3, holes=0.0):
    """A seeded smooth surface times `scale` with multiplicative noise: neighbouring depths within a fraction of a per cent, so that most pixels have eight similar
    neighbours and every sum's order shows in the bits."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 4.0 + 0.011 * x + 0.007 * y + 0.05 * np.sin(x / 5.0) * np.cos(y / 7.0)
    z *= 1.0 + noise * rng.standard_normal((h, w))
    d = (z * scale).astype(f32)
    if holes:
        d[rng.random((h, w)) < holes] = 0
    return d


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------------------
SMALL = ((1, 1), (1, 7), (7, 1))                                         # (h, w): never three neighbours
WIDTHS = (63, 64, 65, 255, 256, 257)                                     # around the wave and the block, three rows; and transposed


def never_three_neighbours(e):
    rng = np.random.default_rng(11)
    for h, w in SMALL:
        d = surface(rng, h, w)
        assert similar_counts(d).max() < 3 and (d > 0).all()
        got, want = check(e, K0, d, "%d x %d" % (w, h))
        assert not got.any() and not want.any()


def two_by_two(e):
    d = np.array([[2.0, 2.01], [2.02, 1.99]], f32)
    assert (similar_counts(d) == 3).all()                                # every pixel is a corner: exactly three neighbours, det = 3
    got, want = check(e, K0, d, "2 x 2")
    assert (np.abs(want).sum(-1) > 0).all(), "2 x 2: det = 3 gives a normal at every pixel"


def three_by_three(e):
    d = surface(np.random.default_rng(12), 3, 3)
    cnt = similar_counts(d)
    assert cnt[1, 1] == 8 and cnt[0, 0] == 3 and cnt[0, 1] == 5
    got, want = check(e, K_ANISO, d, "3 x 3")
    assert (np.abs(want).sum(-1) > 0).all()


def width_case(e, n, transpose):
    rng = np.random.default_rng(100 + n)
    d = surface(rng, 3, n, holes=0.05)
    if transpose:
        d = np.ascontiguousarray(d.T)
    _, want = check(e, K0, d, "%d x %d" % (d.shape[1], d.shape[0]))
    assert (np.abs(want).sum(-1) > 0).mean() > 0.5


def row_end_case(e):
    """A width that is no multiple of 4, more than one block, the last rows short of a block: groups of consecutive pixels cross row ends everywhere."""
    d = surface(np.random.default_rng(13), 11, 103, holes=0.05)
    assert d.shape[1] % 4 and d.size % 256 and d.size > 4 * 256
    check(e, K_OUTSIDE, d, "103 x 11")


def stride_case(e):
    """More pixels than one pass of the capped grid: the kernel's stride loop takes a second trip (device only: a million fibres are slow on the emulator)."""
    h, w = 1027, 1031
    assert PASS < h * w < 2 * PASS
    d = surface(np.random.default_rng(14), h, w, holes=0.1)
    _, want = check(e, K0, d, "%d x %d, past one pass of the grid" % (w, h))
    assert (np.abs(want[-2:]).sum(-1) > 0).any(), "the last rows, which only the second trip reaches, hold normals"


# ---- validity ---------------------------------------------------------------------------------------------------------------------------------------------
def zeros_and_negatives(e):
    rng = np.random.default_rng(15)
    got, _ = check(e, K0, np.zeros((9, 70), f32), "all-zero map")
    assert not got.any()
    d = -surface(rng, 9, 70)
    got, _ = check(e, K0, d, "negative depths")
    assert not got.any()
    d = surface(rng, 9, 70)
    d[rng.random(d.shape) < 0.3] *= -1                                   # negative neighbours of positive centres do not count
    _, want = check(e, K0, d, "mixed signs")
    assert not want[d < 0].any() and want[d > 0].any()


def checkerboard_counts(e):
    """Holes in a checkerboard and at random beside it: the count of similar neighbours takes every value 0 ... 8."""
    rng = np.random.default_rng(16)
    d = surface(rng, 40, 90)
    yy, xx = np.mgrid[0:40, 0:90]
    d[:, :30][((yy + xx) % 2 == 0)[:, :30]] = 0                           # checkerboard: the diagonal neighbours only
    d[:, 30:60][rng.random((40, 30)) < 0.5] = 0
    d[:, 60:][rng.random((40, 30)) < 0.8] = 0
    cnt = similar_counts(d)
    hist = np.bincount(cnt[cnt >= 0], minlength=9)
    assert (hist > 0).all(), hist
    _, want = check(e, K0, d, "checkerboard")
    has = np.abs(want).sum(-1) > 0
    assert not has[(cnt >= 0) & (cnt < 3)].any() and has[cnt >= 3].all()  # three similar neighbours of a 3 x 3 window are never collinear through the centre: det != 0


def two_and_three_neighbours(e):
    two = np.zeros((3, 3), f32); two[1, 1] = 5; two[0, 0] = 5.01; two[2, 1] = 4.99
    three = two.copy(); three[1, 2] = 5.02
    assert similar_counts(two)[1, 1] == 2 and similar_counts(three)[1, 1] == 3
    got, _ = check(e, K0, two, "exactly two similar neighbours")
    assert not got[1, 1].any()
    got, _ = check(e, K0, three, "exactly three similar neighbours")
    assert got[1, 1].any()


def non_finite(e):
    """NaN and +Inf as centre and as neighbour: a zero normal there, the pixels around them as if they were holes."""
    rng = np.random.default_rng(17)
    base = surface(rng, 12, 70)
    for name, v in (("NaN", f32(np.nan)), ("+Inf", f32(np.inf))):
        d = base.copy(); hole = base.copy()
        for r, c in ((0, 0), (5, 33), (6, 34), (11, 69), (3, 64)):
            d[r, c] = v; hole[r, c] = 0
        want = host(K0, d, name)
        assert not want[~np.isfinite(d)].any(), "%s: the host result at the pixel is zero" % name
        same_bits(want, host(K0, hole, name + " as a hole"), name + ": the neighbours see a hole")
        same_bits(e.estimate_normal_map(K0, d), want, name + " depths")


# ---- the 3 % test ------------------------------------------------------------------------------------------------------------------------------------------
def threshold_pairs(magnitude):
    """Pairs (d, di) near `magnitude` whose float ratio fabsf(d - di) / d is one ulp below 0.03f, equals it, and is one ulp above: {-1, 0, 1: (d, di)}.  Found by a
    search: d over consecutive floats, di over the few floats around d * 0.97 (d - di is exact there, so the ratio is one rounded division)."""
    lo, hi = np.nextafter(TH, f32(0)), np.nextafter(TH, f32(1))
    found = {}
    d = f32(magnitude)
    for _ in range(20000):
        d = np.nextafter(d, f32(np.inf))
        di = f32(d - f32(d * TH))
        for _ in range(3):
            di = np.nextafter(di, f32(0))
        for _ in range(7):
            r = ratio(d, di)
            key = -1 if r == lo else 0 if r == TH else 1 if r == hi else None
            if key is not None and key not in found:
                found[key] = (d, di)
            di = np.nextafter(di, f32(np.inf))
        if len(found) == 3:
            return found
    raise AssertionError("no pair at each of the three ratios near %g" % magnitude)


def threshold_case(e, magnitude):
    """A 3 x 3 tile per pair: the centre d, one neighbour di, the other seven d itself.  Whether di counts shows in the centre's normal."""
    pairs = threshold_pairs(magnitude)
    outcomes = {}
    for key, (d, di) in sorted(pairs.items()):
        r = ratio(d, di)
        assert (r < TH) == (key < 0) and (r == TH) == (key == 0), (key, r)
        tile = np.full((3, 3), d, f32); tile[0, 2] = di
        gone = tile.copy(); gone[0, 2] = 0
        got, want = check(e, K_ANISO, tile, "ratio %+d ulp at %g" % (key, magnitude))
        as_hole = host(K_ANISO, gone)[1, 1]
        outcomes[key] = not np.array_equal(bits(want[1, 1]), bits(as_hole))          # True: the neighbour was counted
        assert got[1, 1].any()
    assert outcomes == {-1: True, 0: False, 1: False}, outcomes                    # strict <: equality is not similar


MAGNITUDES = (1e-3, 1.0, 1e6)


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------------------------
SCALES = (1e-3, 1e-1, 1.0, 1e2, 1e4, 1e6)


def arithmetic_case(e, scale):
    rng = np.random.default_rng(int(np.log10(scale)) + 40)
    for k, K in enumerate(KS):
        d = surface(rng, 21, 67, scale=scale, holes=0.08)
        _, want = check(e, K, d, "surface x %g, K %d" % (scale, k))
        assert (np.abs(want).sum(-1) > 0).mean() > 0.5


def tilted_plane_case(e):
    """The host result on a plane n . X = 3 approaches the plane's normal (a check of the yardstick, not a tolerance on the device); the device gives the host's bits."""
    K = K0
    n = np.array([0.3, -0.2, 1.0]); n /= np.linalg.norm(n)
    y, x = np.mgrid[0:40, 0:60].astype(np.float64)
    ray = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x)], -1)
    d = (3.0 / (ray @ n)).astype(f32)                                    # depth along z of the plane
    _, want = check(e, K, d, "plane")
    got = want[1:-1, 1:-1].astype(np.float64)
    got /= np.linalg.norm(got, axis=-1, keepdims=True)
    cos = np.abs(got @ n)
    assert cos.min() > 0.999, cos.min()


# ---- the scene entry point -------------------------------------------------------------------------------------------------------------------------------
def scene_case(e):
    """Three views, the middle one with its own size and K: the listed views get their normals at their own size, the other keeps the sentinel, depth and
    confidence stay as installed."""
    rng = np.random.default_rng(18)
    w, h = 70, 23
    sizes = [(w, h), (41, 37), (w, h)]
    Ks = [K0, K_ANISO, K_OUTSIDE]
    R = np.eye(3); C = np.zeros(3)
    e.scene_create(3, w, h, 0)
    maps = []
    for i, (sw, sh) in enumerate(sizes):
        gray = np.zeros((sh, sw), f32)
        (e.scene_set_view_sized if (sw, sh) != (w, h) else e.scene_set_view)(i, gray, Ks[i], R, C, 0.1, 100.0, [j for j in range(3) if j != i])
        d = surface(rng, sh, sw, holes=0.1); c = rng.random((sh, sw)).astype(f32)
        e.scene_set_maps(i, d, np.full((sh, sw, 3), SENTINEL, f32)); e.scene_set_conf(i, c)
        maps.append((d, c))
    e.scene_estimate_normals([])                                          # no view: a no-op
    for i in range(3):
        assert (e.scene_get_maps(i)[1] == SENTINEL).all()
    e.scene_estimate_normals([2, 1])
    for i, (d, c) in enumerate(maps):
        gd, gn, gc = e.scene_get_maps(i)
        same_bits(gd, d, "depth of view %d" % i); same_bits(gc, c, "confidence of view %d" % i)
        if i == 0:
            assert (gn == SENTINEL).all(), "a view that was not listed keeps its normals"
        else:
            same_bits(gn, host(Ks[i], d, "scene view %d" % i), "scene view %d" % i)
    e.scene_estimate_normals(np.array([0], np.int64))
    same_bits(e.scene_get_maps(0)[1], host(Ks[0], maps[0][0]), "scene view 0")


def error_cases(e, error):
    """Refusals: each leaves a reason, launches nothing and is followed by a call that succeeds."""
    rng = np.random.default_rng(19)
    w, h = 30, 20
    e.scene_create(2, w, h, 0)
    for i in range(2):
        e.scene_set_view(i, np.zeros((h, w), f32), K0, np.eye(3), np.zeros(3), 0.1, 100.0, [1 - i])
    d = surface(rng, h, w)
    e.scene_set_maps(0, d, np.full((h, w, 3), SENTINEL, f32))
    for ids, code, word in (([0, 2], -1, "not a view"), ([-1], -1, "not a view"), ([0, 1], -4, "no depth map")):
        try:
            e.scene_estimate_normals(ids)
        except error as ex:
            assert "pmhip error %d" % code in str(ex) and word in str(ex), str(ex)
        else:
            raise AssertionError("%s was accepted" % (ids,))
        assert (e.scene_get_maps(0)[1] == SENTINEL).all(), "a refused call launches nothing"
    e.scene_estimate_normals([0])
    same_bits(e.scene_get_maps(0)[1], host(K0, d), "after the refusals")
    for shape in ((3, 0), (0, 3)):
        try:
            e.estimate_normal_map(K0, np.zeros(shape, f32))
        except error as ex:
            assert "pmhip error -1" in str(ex) and "pmhip_estimate_normal_map" in str(ex), str(ex)
        else:
            raise AssertionError("an empty map was accepted")
    check(e, K0, d, "after w = 0")


# ---- interleaved sizes on one engine ------------------------------------------------------------------------------------------------------------------------
def interleaved_sizes(e):
    """One engine, large and small maps in turn: nothing of a call outlives it."""
    rng = np.random.default_rng(20)
    for h, w in ((50, 300), (2, 2), (300, 50), (1, 1), (7, 257), (50, 300)):
        check(e, KS[(h + w) % 3], surface(rng, h, w, holes=0.1), "%d x %d in turn" % (w, h))


# ---- resume: a .dmap stored without normals ---------------------------------------------------------------------------------------------------------------
def resume_case(e, tmp_dir, monkeypatch):
    """densify.compute_depth_maps with every view's depthNNNN.dmap on disk, two of them written without normals: those get their normals from
    `scene_estimate_normals` on the engine (counted on the binding), the resident maps equal the host's, and a stored normal map is installed as it is."""
    import os
    from openmvs_amd import densify, dmap, synth
    from openmvs_amd.patchmatch import PMHipParams, PatchMatchHIP
    sc = synth.make_scene(4, 32, 24, n_src=2)
    sc.sizes = [(32, 24)] * 4
    rng = np.random.default_rng(21)
    d = str(tmp_dir)
    os.makedirs(d, exist_ok=True)
    stored = {}
    for v in range(4):
        depth = surface(rng, 24, 32, holes=0.1); conf = rng.random((24, 32)).astype(f32)
        normal = None if v in (1, 3) else np.full((24, 32, 3), SENTINEL, f32)
        dmap.save(os.path.join(d, dmap.depth_file_name(v)), "x.jpg", [v] + [int(i) for i in sc.neighbors[v]], (32, 24), sc.K[v], sc.R[v], sc.C[v], 1.0, 9.0, depth, normal, conf)
        stored[v] = (depth, normal, conf)
    calls = []
    real = PatchMatchHIP.scene_estimate_normals
    monkeypatch.setattr(PatchMatchHIP, "scene_estimate_normals", lambda self, ids: (calls.append([int(i) for i in ids]), real(self, ids))[1])
    e.scene_load(sc, n_levels=0)
    p = PMHipParams(); p.nEstimationGeometricIters = 0
    assert densify.compute_depth_maps(e, [0, 1, 2, 3], p, n_optimize=0, scene=sc, dmap_dir=d) == [0, 1, 2, 3]
    assert calls == [[1], [3]], calls
    for v, (depth, normal, conf) in stored.items():
        gd, gn, gc = e.scene_get_maps(v)
        same_bits(gd, depth, "resumed depth %d" % v); same_bits(gc, conf, "resumed confidence %d" % v)
        same_bits(gn, host(sc.K[v], depth, "resumed view %d" % v) if normal is None else normal, "resumed normals %d" % v)


# ---- mode -2 through to the cloud -------------------------------------------------------------------------------------------------------------------------------
def mode2_options():
    """The options of tests/test_sgm_real.py::test_sgm_modes_of_dense_reconstruction: a quarter of the resolution (160 x 120), two views per image."""
    from openmvs_amd import optdense
    opt = optdense.defaults()
    opt.nResolutionLevel = 2; opt.nMinResolution = 80; opt.nNumViews = 2; opt.nEstimateNormals = 2; opt.fViewMinScore = 0.0
    return opt


def mode2_yardstick(be, mvs, pair_dir, opt, mvs_out):
    """Today's pieces called one by one: `fuse_scene`'s maps with their numpy normals installed by scene_set_maps / scene_set_conf, the same filters, fusion and finish,
    the archive written to `mvs_out`.  Returns ({image: resident (depth, normal, conf) at the end}, cloud)."""
    from openmvs_amd import densify, mvsi, sgm_pipeline
    from openmvs_amd import views as _views
    e = be.e
    sv = densify.load_scene(mvs, opt=opt)
    sc = mvsi.load(mvs)
    cams = _views.Cameras(sc, sv.sizes[:len(sc.images)])
    nbs = {i: sv.all_view_scores[i] for i in sv.ids if len(sv.all_view_scores.get(i, ()))}
    sizes = {i: tuple(sv.sizes[i]) for i in nbs}
    fused = sgm_pipeline.fuse_scene(be, cams, sizes, nbs, pair_dir, n_views=int(opt.nNumViews), f_min_score_ratio=float(opt.fViewMinScoreRatio),
                                    f_min_score=float(opt.fViewMinScore), min_views=2, estimate_normals=True)
    e.scene_load(sv, n_levels=int(opt.nSubResolutionLevels))
    th = float(opt.fDepthDiffThreshold)
    for i in sorted(fused):
        depth, normal, conf = fused[i]
        sv.dmin[i], sv.dmax[i] = 1e-4, float(np.finfo(f32).max)
        e.scene_set_view(i, None, sv.K[i], sv.R[i], sv.C[i], sv.dmin[i], sv.dmax[i], sv.neighbors[i])
        e.scene_set_maps(i, depth, np.zeros(depth.shape + (3,), f32) if normal is None else normal)
        e.scene_set_conf(i, conf)
        if int(opt.nOptimize) & densify.REMOVE_SPECKLES:
            e.scene_remove_small_segments([i], int(opt.nSpeckleSize), th)
        if int(opt.nOptimize) & densify.FILL_GAPS:
            e.scene_gap_interpolation([i], int(opt.nIpolGapSize), th)
    if int(opt.nOptimize) & densify.ADJUST_FILTER:
        e.scene_filter(sorted(fused), bool(opt.bFilterAdjust), int(opt.nMinViewsFilter), int(opt.nMinViewsFilterAdjust), th, commit=True)
    maps = {i: e.scene_get_maps(i) for i in sorted(fused)}
    cloud = densify.fuse_depth_maps(e, sv, opt, bgr=sv.bgr)
    cloud = densify.finish_point_cloud(e, (sv, None), opt, False, 0.0, cloud=cloud)
    densify.save_dense_scene(mvs, mvs_out, cloud, sv)
    return maps, cloud


def mode2_case(be, mvs, work_dir, error=ValueError):
    """Mode -1 once, then mode -2 with `mvs_out` against the yardstick: byte-identical archives, every depthNNNN.dmap equal to the host composition, a cloud."""
    import os
    from openmvs_amd import dmap, sgm_pipeline
    opt = mode2_options()
    assert int(opt.nOptimize) == 7, "speckles, gaps and the cross-view filter all run"
    pairs = os.path.join(str(work_dir), "sgm")
    assert len(sgm_pipeline.dense_reconstruction(be, mvs, pairs, -1, opt, min_resolution=40)) >= 4
    new_out, old_out = os.path.join(str(work_dir), "new_dense.mvs"), os.path.join(str(work_dir), "old_dense.mvs")
    cloud = sgm_pipeline.dense_reconstruction(be, mvs, pairs, -2, opt, mvs_out=new_out)
    assert cloud["nPoints"] > 0 and cloud["normals"] is not None and len(cloud["points"]) == cloud["nPoints"]
    files = {i: dmap.load(os.path.join(pairs, dmap.depth_file_name(i))) for i in range(4)}
    maps, old_cloud = mode2_yardstick(be, mvs, pairs, opt, old_out)
    assert sorted(maps) == [0, 1, 2, 3]
    for i, (depth, normal, conf) in maps.items():
        f = files[i]
        same_bits(f["depth_map"], depth, "depth%04d.dmap" % i); same_bits(f["normal_map"], normal, "normals of depth%04d.dmap" % i)
        same_bits(f["confidence_map"], conf, "confidence of depth%04d.dmap" % i)
        assert f["depth_min"] == f32(1e-4) and f["depth_max"] == np.finfo(f32).max and (depth > 0).mean() > 0.1 and np.abs(normal).sum(-1).astype(bool).mean() > 0.1
    assert old_cloud["nPoints"] == cloud["nPoints"]
    with open(new_out, "rb") as a, open(old_out, "rb") as b:
        assert a.read() == b.read(), "the dense archives differ"
    # the limit: without normal maps the reference fuses with a constant normal, which the engine's fusion does not have
    opt0 = mode2_options(); opt0.nEstimateNormals = 0
    try:
        sgm_pipeline.dense_reconstruction(be, mvs, pairs, -2, opt0, mvs_out=new_out)
    except ValueError as ex:
        assert "nEstimateNormals" in str(ex)
    else:
        raise AssertionError("mvs_out with nEstimateNormals = 0 was accepted")
