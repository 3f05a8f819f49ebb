"""Adversarial inputs for the depth-map post-filters (csrc/pm_filter.hip through pmhip_scene_remove_small_segments / _gap_interpolation / _filter) and the SGM
speckle filter (csrc/sgm_post.hip through sgmhip_filter_speckles), shared by the emulator suite (tests/test_emu_post_filter_edges.py) and the device suite
(tests/test_zz_gpu_post_filter_edges.py).  These are the kernels with races to lose: a lock-free union-find with compressing finds, 64-bit atomicMin splats with
the tie-break packed into the key, a host replay over a device-built edge list.  Their other tests feed them estimated maps of the synthetic scene; the maps
here are built for what those never contain -- every neighbouring pair a one-directional edge, one giant component, n singletons, components of exactly the
speckle size, gaps on every border and of exactly the gap size, z-tests that tie.

Every expected value comes from the sequential oracle (oracle.pyoracle), every comparison is exact (floats through their uint32 view, so NaN compares too), and
every check first asserts on the oracle's result alone that its input does what it claims: a degenerate generator must not pass silently."""
import functools

import numpy as np

from oracle import pyoracle as po

F = np.float32
SMALL = (67, 37)            # odd both ways; 2479 pixels = 38 full waves and one of 47 lanes
LARGE = (331, 211)          # device only: 69 841 pixels, ~1090 waves in 273 blocks
MEDIUM = (131, 77)          # device only, the two full ramps: at 331 x 211 the host replay walks 139 000 edges and 70 000 components through std::map, 0.5 s a call
FULL_RAMPS = ("ramp_rising", "ramp_falling")
THIN = ((3, 70), (70, 3))   # the narrowest maps the engine holds (pmhip_scene_set_view_sized: at least 3 x 3)
THIN_SCENE = ((9, 70), (70, 9))   # ... and the narrowest scenes (pmhip_scene_create: at least 2 * nSizeHalfWindow + 1 both ways), for the cross-view filter
THIN_SGM = ((1, 70), (70, 1))
SPECKLE_SIZES = (0, 1, 39, 40, 41, 100, 100000)
SEGMENT_THRESHOLDS = (0.01, 0.002)
GAP_SIZES = (0, 1, 7, 9)
GAP_THRESHOLDS = (0.01, 0.001)
SGM_SPECKLES = ((100, 5), (10, 1), (0, 0), (5000, 50), (39, 2))     # (maxSpeckleSize, maxDiff)
NO_DISP = 32767
Z0 = 2.0


def same(got, want, what, names=("depth", "normal", "conf")):
    for a, b, nm in zip(got, want, names):
        a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, nm, a.shape, b.shape)
        ne = a.view(np.uint32) != b.view(np.uint32) if a.dtype == np.float32 else a != b
        assert not ne.any(), "%s: %s differs from the oracle at %d of %d elements (first at %s)" % (what, nm, int(ne.sum()), ne.size, tuple(int(v) for v in np.argwhere(ne)[0]))


# ---- an engine that holds maps of a given size -----------------------------------------------------------------------------------------------------------
class _Views:
    """What PatchMatchHIP.scene_load reads of a scene: n pinhole cameras side by side with empty images (no test here estimates anything)."""

    def __init__(self, n, w, h):
        self.n_views, self.width, self.height = n, w, h
        self.gray = [np.zeros((h, w), F) for _ in range(n)]
        self.K = [np.array([[float(w), 0, w / 2.0], [0, float(w), h / 2.0], [0, 0, 1]]) for _ in range(n)]
        self.R = [np.eye(3) for _ in range(n)]
        self.C = [np.array([0.1 * i, 0.0, 0.0]) for i in range(n)]
        self.dmin = [0.5] * n; self.dmax = [10.0] * n
        self.neighbors = [np.array([j for j in range(n) if j != i], np.int32) for i in range(n)]


def load_maps_of(engine, w, h):
    """View 0 of the engine's scene gets maps of w x h: the scene's own size where a scene can be that small, a view with its own size below that."""
    W, H = max(w, 9), max(h, 9)
    sc = _Views(2, W, H)
    engine.scene_load(sc, n_levels=0)
    if (W, H) != (w, h):
        engine.scene_set_view_sized(0, np.zeros((h, w), F), sc.K[0], sc.R[0], sc.C[0], 0.5, 10.0, sc.neighbors[0])
    assert engine.view_size(0) == (w, h)


def normals_and_conf(d, seed):
    """Unit normals away from (0, 0, -1) and confidences in (0.1, 1) on the valid pixels (depth > 0), zeros elsewhere -- what an estimate leaves."""
    r = np.random.RandomState(seed)
    h, w = d.shape
    n = r.normal(size=(h, w, 3)); n[..., 2] = -np.abs(n[..., 2]) - 0.2
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    c = r.uniform(0.1, 1.0, (h, w)).astype(F)
    ok = d > 0
    n[~ok] = 0; c[~ok] = 0
    return n, c


# ---- RemoveSmallSegments -----------------------------------------------------------------------------------------------------------------------------------
def _similar(a, b, th):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(a - b) / a < th                      # IsDepthSimilar in float, as the kernels and the oracle evaluate it


def asymmetric_share(d, th):
    """Share of the 4-connected neighbouring pairs of valid pixels that are similar in exactly one direction."""
    one = tot = 0
    for a, b in ((d[:, :-1], d[:, 1:]), (d[:-1], d[1:])):
        ok = (a > 0) & (b > 0)
        one += int(((_similar(a, b, th) != _similar(b, a, th)) & ok).sum()); tot += int(ok.sum())
    return one / max(tot, 1)


def ramp_ratio(th):
    """q with q - 1 >= th and (q - 1) / q < th: a step that is similar seen from the larger depth and not from the smaller one.  (q - 1) / q < th holds for
    q - 1 = k * th with 1 <= k < 1 / (1 - th); k = 1 + th / 2 leaves th / 2 relative margin either way, against 2^-23 / th of rounding in the float depths."""
    return 1.0 + float(th) * (1.0 + float(th) / 2)


def raster_islands(w, h, sizes, value):
    """Islands of exactly sizes[k] pixels each: full rows from the top, the last row of an island cut short, one empty row between islands (in a map too flat
    for that: the same along the columns).  None if they do not fit."""
    d = np.zeros((h, w), value.dtype)
    y = 0
    for s in sizes:
        if s == 0:
            continue
        rows = -(-s // w)
        if y + rows > h:
            if w > h:
                t = raster_islands(h, w, sizes, value)
                return None if t is None else np.ascontiguousarray(t.T)
            return None
        flat = d[y:y + rows].reshape(-1); flat[:s] = value
        y += rows + 1
    return d


def terraces(w, h, seed, th):
    """The mix the older tests use: levels right at the similarity threshold on 4 x 4 blocks over a smooth plane, 10 % holes."""
    r = np.random.RandomState(seed)
    lv = (2.0 * (1 + float(th)) ** (r.randint(0, 6, (h, w)) * r.choice([0.97, 1.0, 1.03]))).astype(F)
    blk = np.kron(r.rand(-(-h // 4), -(-w // 4)) < 0.5, np.ones((4, 4), bool))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.where(blk, lv, 2.0 + 0.002 * xx + 0.001 * yy).astype(F)
    d[r.rand(h, w) < 0.1] = 0
    return d


def segment_maps(w, h, fth):
    """(name, depth map, claim) for RemoveSmallSegments at fDepthDiffThreshold = fth.  claim(nSpeckleSize) -> number of pixels the sequential filter keeps, or None."""
    th = F(fth) * F(0.7)
    q = ramp_ratio(th)
    n = w * h
    yy, xx = np.mgrid[0:h, 0:w]
    whole = lambda m: (lambda sz: m if m >= sz else 0)            # one segment of m pixels: removed iff m < nSpeckleSize
    each = lambda m, cnt: (lambda sz: m * cnt if m >= sz else 0)  # cnt segments of m pixels each
    out = []
    # every pair one-directional, every pixel its own mutual component: the edge list holds 2wh - w - h pairs.  Depth similarity points downhill, and the seeds
    # come in column-major order: rising, every seed finds its lower neighbours claimed already (n segments of 1); falling, the first seed reaches everything
    out.append(("ramp_rising", (2.0 * q ** (xx + yy).astype(np.float64)).astype(F), each(1, n)))
    out.append(("ramp_falling", (2.0 * q ** -(xx + yy).astype(np.float64)).astype(F), whole(n)))
    # constant along y: the columns are mutual components of h pixels, linked by one-directional edges -- the segment sizes are sums the host replay forms
    out.append(("xramp_rising", (2.0 * q ** xx.astype(np.float64)).astype(F), each(h, w)))
    out.append(("xramp_falling", (2.0 * q ** -xx.astype(np.float64)).astype(F), whole(n)))
    # columns in pairs one ratio apart, 5 % between pairs: high -> low makes segments of two columns, low -> high of one (and an odd last column stays alone)
    pair = 2.0 * 1.05 ** (xx // 2).astype(np.float64)
    out.append(("xpairs_down", (pair * q ** -(xx % 2).astype(np.float64)).astype(F), lambda sz: (2 * h * (w // 2) if 2 * h >= sz else 0) + (h * (w % 2) if h >= sz else 0)))
    out.append(("xpairs_up", (pair * q ** (xx % 2).astype(np.float64)).astype(F), each(h, w)))
    out.append(("flat", np.full((h, w), 2.0, F), whole(n)))        # one component: every union contends for root 0, the flatten pass sees one root per wave
    s = np.zeros((h, w), F); s[::2] = 2.0
    for k, y in enumerate(range(1, h, 2)):
        s[y, (w - 1) if k % 2 == 0 else 0] = 2.0
    if h % 2 == 0:
        s[h - 1] = 0                                               # (no dangling connector below the last full row)
    out.append(("serpentine", s, whole(int((s > 0).sum()))))       # one component of about n / 2 pixels and maximal depth
    out.append(("checkerboard", np.where((xx + yy) % 2 == 0, 2.0, 3.0).astype(F), each(1, n)))
    isl = raster_islands(w, h, (40, 39), F(2.0))
    if isl is not None:
        out.append(("islands_40_39", isl, lambda sz: (40 if 40 >= sz else 0) + (39 if 39 >= sz else 0)))   # pins the strict <
    sp = np.full((h, w), 2.0, F)
    sp[h // 5, w // 3] = np.nan; sp[h // 4, w // 2] = np.inf; sp[h // 3, w // 4] = -1.0
    sp[h // 2:h // 2 + 2, w // 2:w // 2 + 2] = np.nan
    out.append(("special_values", sp, None))
    out.append(("terraces", terraces(w, h, 5, th), None))
    return out


def segments_equal_the_oracle(engine, size, maps=None):
    """Every map of segment_maps (or those named in `maps`) at every speckle size and threshold; returns the number of filter calls compared."""
    w, h = size
    load_maps_of(engine, w, h)
    ran = 0
    for fth in SEGMENT_THRESHOLDS:
        th = F(fth) * F(0.7)
        for k, (name, d, claim) in enumerate(segment_maps(w, h, fth)):
            if maps is not None and name not in maps:
                continue
            nrm, cnf = normals_and_conf(d, 100 + k)
            share = asymmetric_share(d, th)
            if name.startswith("ramp_"):
                assert share == 1.0, (name, fth, share)             # the edge list is full
            if name.startswith("xramp_") or name.startswith("xpairs_"):
                assert 0 < share < 1 and asymmetric_share(d[:1], th) >= (0.49 if "pairs" in name else 1.0), (name, fth, share)
            if name in ("flat", "serpentine", "checkerboard", "islands_40_39"):
                assert share == 0.0, (name, share)
            if name == "serpentine":
                assert (d > 0).sum() >= 0.45 * d.size or min(w, h) < 9, name
            if name == "special_values":
                assert np.isnan(d).sum() == 5 and np.isinf(d).sum() == 1 and (d < 0).sum() == 1
            for sz in SPECKLE_SIZES:
                what = "RemoveSmallSegments %s %dx%d nSpeckleSize %d fDepthDiffThreshold %g" % (name, w, h, sz, fth)
                want = po.remove_small_segments(d, nrm, cnf, nSpeckleSize=sz, fDepthDiffThreshold=fth)
                if claim is not None:
                    assert int((want[0] > 0).sum()) == claim(sz), (what, int((want[0] > 0).sum()), claim(sz))
                engine.scene_set_maps(0, d, nrm); engine.scene_set_conf(0, cnf)
                engine.scene_remove_small_segments([0], nSpeckleSize=sz, fDepthDiffThreshold=fth)
                same(engine.scene_get_maps(0), want, what)
                ran += 1
    return ran


# ---- GapInterpolation --------------------------------------------------------------------------------------------------------------------------------------
def _runs(limit, lengths, first=2, sep=2):
    """Start positions for gaps of these lengths along a line of `limit` pixels, `sep` valid pixels between them and after the last; those that fit."""
    out = []; at = first
    for L in lengths:
        if at + L + sep > limit:
            break
        out.append((at, L)); at += L + sep
    return out


def gap_map(w, h, trial):
    """A nearly flat map with rectangular holes on and off the borders, and gaps of controlled length on the borders, where the other pass cannot fill them:
    row 0 (the column pass finds no valid pixel above), column 0 and the last column (the row pass finds none beside), the last row.  Returns depth, normal, conf
    and the claims: exact = [(axis, line, start, length)] gaps between equal depths, filled iff length <= nIpolGapSize; steps = [(start, ratio, fth)] gaps of
    3 pixels in the last row whose ends differ by ratio x the similarity threshold at fDepthDiffThreshold = fth."""
    r = np.random.RandomState(1000 + trial)
    d = (2.0 + 0.01 * r.rand(h, w)).astype(F)
    for _ in range(max(25, 25 * w * h // (SMALL[0] * SMALL[1]))):
        hh, ww = min(r.randint(1, 10), h), min(r.randint(1, 10), w)
        y = [0, h - hh, r.randint(0, h - hh + 1), r.randint(0, h - hh + 1)][r.randint(4)]      # anchored at a border as often as inside, per axis
        x = [0, w - ww, r.randint(0, w - ww + 1), r.randint(0, w - ww + 1)][r.randint(4)]
        d[y:y + hh, x:x + ww] = [0, 0, -1.0][r.randint(3)]
    if trial % 5 == 0:
        d[r.randint(0, h), :] = 0; d[:, r.randint(0, w)] = 0
    hole = lambda k: F(0 if k % 2 == 0 else -1.0)
    exact = []
    lengths = sorted({g + e for g in GAP_SIZES for e in (-1, 0, 1) if g + e > 0})      # 1, 2, 6, 7, 8, 9, 10
    d[0, :min(w, 2 + sum(L + 2 for L in lengths))] = 2.0
    for x0, L in _runs(w, lengths):
        d[0, x0:x0 + L] = hole(L); exact.append((0, 0, x0, L))
    for col, part in ((0, lengths[:4]), (w - 1, lengths[4:])):
        d[1:min(h, 2 + sum(L + 2 for L in part)), col] = 2.0
        for y0, L in _runs(h, part):
            d[y0:y0 + L, col] = hole(L); exact.append((1, col, y0, L))
    steps = []
    cases = [(ratio, fth) for fth in GAP_THRESHOLDS for ratio in (0.99, 1.01)]
    if h >= 3 and w >= 4 + 5 * len(cases):
        d[h - 1, 1:2 + 5 * len(cases)] = 2.0
        for k, (ratio, fth) in enumerate(cases):
            x0 = 2 + 5 * k
            d[h - 1, x0:x0 + 3] = hole(k); d[h - 1, x0 + 3] = F(2.0 * (1.0 + ratio * float(F(fth) * F(2.5))))
            steps.append((x0, ratio, fth))
    nrm, cnf = normals_and_conf(d, 2000 + trial)
    return d, nrm, cnf, exact, steps


def gaps_equal_the_oracle(engine, size, n_maps=30):
    w, h = size
    load_maps_of(engine, w, h)
    border = np.zeros((h, w), bool); border[0] = border[-1] = True; border[:, 0] = border[:, -1] = True
    ran = n_exact = n_steps = 0
    for trial in range(n_maps):
        d, nrm, cnf, exact, steps = gap_map(w, h, trial)
        assert np.abs(nrm[d > 0] - F([0, 0, -1])).max() > 0.5                  # Normal2Dir / Dir2Normal run on something other than (0, 0, -1)
        for gap in GAP_SIZES:
            for fth in GAP_THRESHOLDS:
                what = "GapInterpolation map %d %dx%d nIpolGapSize %d fDepthDiffThreshold %g" % (trial, w, h, gap, fth)
                want = po.gap_interpolation(d, nrm, cnf, nIpolGapSize=gap, fDepthDiffThreshold=fth)
                filled = ~(d > 0) & (want[0] > 0)
                if gap == 0:
                    assert not filled.any(), what
                else:
                    assert filled.any(), what
                    assert (border & ~(d > 0) & ~(want[0] > 0)).any(), what          # a gap that touches a border stays
                for axis, line, at, L in exact:
                    got = filled[line, at:at + L] if axis == 0 else filled[at:at + L, line]
                    assert got.all() if L <= gap else not got.any(), (what, axis, line, at, L)
                    n_exact += 1
                for x0, ratio, made in steps:
                    similar = ratio * float(F(made) * F(2.5)) < float(F(fth) * F(2.5))
                    got = filled[h - 1, x0:x0 + 3]
                    assert got.all() if (similar and gap >= 3) else not got.any(), (what, x0, ratio, made)
                    n_steps += 1
                engine.scene_set_maps(0, d, nrm); engine.scene_set_conf(0, cnf)
                engine.scene_gap_interpolation([0], nIpolGapSize=gap, fDepthDiffThreshold=fth)
                same(engine.scene_get_maps(0), want, what)
                ran += 1
    assert n_exact > 0 and (n_steps > 0 or w < 24)
    return ran


# ---- FilterDepthMap ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synth(n, w, h):
    from openmvs_amd import synth
    return synth.make_scene(n, w, h, n_src=n - 1)


def filter_equals_the_oracle(engine, size):
    """Five slots on the camera of view 0 of the synthetic scene: 1 = the same camera, 2 = translated along its x axis by 3 * Z0 / fx (three pixels at depth Z0),
    3 = turned half round about its y axis (its points fall behind the others), 4 = the same pose with maps of 1.25 x the size.  With depth maps that are
    constant Z0 (then with holes, then with two levels) nearly every z-test of the splat is a tie, and the confidence has to be the last source pixel's in raster
    order."""
    w, h = size
    base = _synth(5, w, h); big = _synth(5, w * 5 // 4, h * 5 // 4)
    bw, bh = big.width, big.height
    K0, R0, C0 = base.K[0].copy(), base.R[0].copy(), base.C[0].copy()
    K = {v: K0 for v in range(4)}; K[4] = big.K[0].copy()
    R = {v: R0 for v in range(5)}; R[3] = np.diag([-1.0, 1.0, -1.0]) @ R0
    Cc = {v: C0 for v in range(5)}; Cc[2] = C0 + R0.T @ np.array([3 * Z0 / K0[0, 0], 0.0, 0.0])
    shape = {v: (h, w) for v in range(4)}; shape[4] = (bh, bw)
    dmin, dmax = 0.5, 10.0
    engine.scene_load(base, n_levels=0)
    engine.scene_set_view_sized(4, np.zeros((bh, bw), F), K[4], R[4], Cc[4], dmin, dmax, [0])
    assert engine.view_size(4) == (bw, bh) and engine.view_size(0) == (w, h)
    configs = (                                         # name, neighbours, views filtered, nMinViewsFilter
        ("ties", {0: [1, 2], 1: [0, 2], 2: [0, 1], 3: [0], 4: [0]}, [0, 1, 2], 2),
        ("behind", {0: [1, 2, 3], 1: [0, 2], 2: [0, 1], 3: [0, 1], 4: [0]}, [0, 1, 2, 3], 2),
        ("other_size", {0: [1, 2, 4], 1: [0, 2], 2: [0, 1], 3: [0], 4: [0, 1, 2]}, [0, 1, 2, 4], 2),
        ("too_few_views", {0: [1, 2], 1: [0, 2], 2: [0, 1], 3: [0], 4: [0]}, [0, 1, 2], 3),
    )
    r = np.random.RandomState(1)
    ran = 0
    for variant in ("constant", "holes", "two_levels"):
        dep, cnf = {}, {}
        for v in range(5):
            d = np.full(shape[v], Z0, F)
            if variant != "constant":
                d[r.rand(*shape[v]) < 0.2] = 0
            if variant == "two_levels":
                d = np.where((r.rand(*shape[v]) < 0.3) & (d > 0), F(Z0 * 1.005), d).astype(F)
            c = r.uniform(0.1, 1.0, shape[v]).astype(F); c[d == 0] = 0
            dep[v] = d; cnf[v] = c
        for name, nbs, views, min_views in configs:
            for v in range(5):
                engine.scene_set_view(v, None, K[v], R[v], Cc[v], dmin, dmax, np.asarray(nbs[v], np.int32))
            for adjust in (True, False):
                for v in range(5):
                    engine.scene_set_maps(v, dep[v], np.zeros(shape[v] + (3,), F)); engine.scene_set_conf(v, cnf[v])
                engine.scene_filter(views, bAdjust=adjust, nMinViewsFilter=min_views)
                for v in views:
                    what = "FilterDepthMap %s %s %dx%d bAdjust %s view %d" % (variant, name, w, h, adjust, v)
                    rc, od, oc = po.filter_depth_map(dep, cnf, K, R, Cc, v, nbs[v], dmin, dmax, bAdjust=adjust, nMinViewsFilter=min_views, nCalibratedImages=5)
                    gd, _, gc = engine.scene_get_maps(v)
                    if name == "too_few_views":
                        assert rc == 1, what                                   # the reference declines; the engine leaves the maps as they are
                        od, oc = dep[v], cnf[v]
                    else:
                        assert rc == 0, what
                    same((gd, gc), (od, oc), what, names=("depth", "conf"))
                    if name == "ties" and v == 0:
                        assert (od > 0).sum() > 0.3 * od.size, what
                        if adjust:
                            assert (oc[od > 0] != cnf[v][od > 0]).any(), what    # a confidence that came out of the splat
                    if name == "behind" and v == 3:
                        assert not (od > 0).any(), what                        # nothing lands in front of the turned camera: no neighbour agrees
                    ran += 1
    return ran


# ---- SGM FilterSpeckles ------------------------------------------------------------------------------------------------------------------------------------
def speckle_maps(w, h, mx, df):
    """(name, disparity map, claim) for FilterSpeckles(maxSpeckleSize = mx, maxDiff = df); claim = number of pixels the filter leaves valid, or None."""
    n = w * h
    yy, xx = np.mgrid[0:h, 0:w]
    whole = lambda m: (m if m > mx else 0)                                    # this filter erases at <=
    out = [("flat", np.full((h, w), 7, np.int16), whole(n))]
    s = np.full((h, w), NO_DISP, np.int16); s[::2] = 7
    for k, y in enumerate(range(1, h, 2)):
        s[y, (w - 1) if k % 2 == 0 else 0] = 7
    if h % 2 == 0:
        s[h - 1] = NO_DISP
    out.append(("serpentine", s, whole(int((s != NO_DISP).sum()))))
    out.append(("checkerboard", np.where((xx + yy) % 2 == 0, -3, -3 + df + 1).astype(np.int16), n if mx < 1 else 0))
    out.append(("all_invalid", np.full((h, w), NO_DISP, np.int16), 0))
    out.append(("stairs_by_maxdiff", (df * (xx + yy) - 40).astype(np.int16), whole(n)))
    assert (df + 1) * (w + h) - 40 < NO_DISP
    out.append(("stairs_by_maxdiff_plus_1", ((df + 1) * (xx + yy) - 40).astype(np.int16), n if mx < 1 else 0))
    isl = raster_islands(w, h, (mx, mx + 1), np.int16(11))
    if isl is not None:
        isl[isl == 0] = NO_DISP
        out.append(("islands_at_and_above_the_size", isl, mx + 1))
    return out


def speckles_equal_the_oracle(matcher, size):
    w, h = size
    ran = n_islands = 0
    for mx, df in SGM_SPECKLES:
        for name, d, claim in speckle_maps(w, h, mx, df):
            what = "FilterSpeckles %s %dx%d maxSpeckleSize %d maxDiff %d" % (name, w, h, mx, df)
            want = po.sgm_filter_speckles(d, mx, df)
            assert int((want != NO_DISP).sum()) == claim, (what, int((want != NO_DISP).sum()), claim)
            got = matcher.FilterSpeckles(d, mx, df)
            assert got.dtype == want.dtype and np.array_equal(got, want), "%s: %d pixels differ" % (what, int((got != want).sum()))
            ran += 1; n_islands += name.startswith("islands")
    assert n_islands >= 2
    return ran
