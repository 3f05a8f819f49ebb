"""The level resamplers at the end of csrc/pm_kernels.hip -- pm_area_kernel, pm_upsample_kernel, pm_nearest_down_kernel, pm_nearest_up_f_kernel, pm_mask_level_kernel,
pm_skew_kernel, pm_quad_kernel -- each launched once through `PatchMatchHIP.resample` (pmhip_resample: production's launch helper, production's grid) at every small
size at which its rule can go wrong, against walks written here from the rule's statement.  The walks call neither oracle/ nor the engine; the oracle's resamplers are
then compared with the walks as a second check, so that the two restatements pin each other.  Shared by tests/test_emu_resample.py (wave64 emulator) and
tests/test_zz_gpu_resample.py (device).

The rules, as OpenCV states them (imgproc/src/resize.cpp; OpenCV itself is not available to the suite, see DESIGN.md 5 "Unpinned by necessity"):
  size      cv::resize(src, dst, Size(), 1/f, 1/f): dsize = cvRound(ssize / f), ties to even.
  nearest   resize: inv_scale = dsize / ssize; resizeNN: ifx = 1. / inv_scale, sx = min(cvFloor(dx * ifx), ssize - 1).  In double.
  linear    scale = 1. / inv_scale; fx = (float)((dx + 0.5) * scale - 0.5); sx = cvFloor(fx); fx -= sx; sx < 0: fx = 0, sx = 0; sx >= ssize - 1: fx = 0, sx = ssize - 1;
            a pixel is (S(y0,x0) a0 + S(y0,x1) a1) b0 + (S(y1,x0) a0 + S(y1,x1) a1) b1 with a1 = fx, a0 = 1.f - fx, x1 = min(x0 + 1, ssize - 1), in float.
  area      integer factor f: a full f x f block is ((a + b) + (c + d)) * 0.25f for f = 2, else the row-major running sum * (1.f / (f * f)); a block cut by the right or
            bottom border is (float)sum / count of the pixels there are, and every pixel of a cut bottom row takes that path, full width or not."""
import numpy as np

f32 = np.float32
u32 = np.uint32
FILL = 0x7FC0BEEF          # the destination before a launch: a NaN no kernel produces
AREA_FACTORS = (2, 4, 8)
UP_WIDTHS = range(10, 82)
UP_HEIGHTS = (11, 12, 13)  # coarse 6 each: 2s - 1, 2s, 2s + 1
MASK_WIDTHS = range(36, 301)
SKEW_SIZES = (9, 10, 33, 64, 65, 130)
# what the issue measured over W <= 300 with a level of at least 9 columns; the tests recompute this from the two formulas and compare
KNOWN_DISAGREEMENTS = {(58, 2), (86, 2), (174, 2), (194, 2), (116, 3), (164, 3), (172, 3), (174, 3), (194, 3), (261, 3), (291, 3)}


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------------------
def cv_round(v):
    return int(np.rint(v))                                     # ties to even


def scaled(n, f):
    return cv_round(n / f)


def nn_index(d, dn, sn):
    """The one nearest rule (csrc/pm_math.h pm_nn_index), in Python doubles."""
    return min(int(np.floor(d * (1.0 / (dn / sn)))), sn - 1)


def nn_index_old(d, dn, sn):
    """What the kernels and the oracle computed before: ifx = sn / dn."""
    return min(int(np.floor(d * (sn / dn))), sn - 1)


def nn_axis(dn, sn, rule=nn_index):
    return np.array([rule(d, dn, sn) for d in range(dn)], np.int64)


def linear_coef(d, dn, sn, scale=None):
    scale = 1.0 / (dn / sn) if scale is None else scale
    f = f32((d + 0.5) * scale - 0.5)
    s = int(np.floor(f))
    f = f32(f - f32(s))
    if s < 0:
        f, s = f32(0), 0
    if s >= sn - 1:
        f, s = f32(0), sn - 1
    return s, f


def linear_axis(dn, sn):
    c = [linear_coef(d, dn, sn) for d in range(dn)]
    return np.array([s for s, _ in c], np.int64), np.array([a for _, a in c], f32)


# ---- sources -----------------------------------------------------------------------------------------------------------------------------------------
def textured(rng, shape):
    """Seeded float32 over 1e-3 .. 1e4 with exact zeros (holes) and -0: the order of a sum shows in the bits."""
    v = (10.0 ** rng.uniform(-3.0, 4.0, shape)).astype(f32)
    r = rng.random(shape)
    v[r < 0.06] = f32(0.0)
    v[(r >= 0.06) & (r < 0.09)] = f32(-0.0)
    return v


def coded(sw, sh, channels=1):
    """value = (y * sw + x) [* channels + c]: exact in float32, every source pixel its own value."""
    assert sw * sh * channels < 1 << 24
    v = np.arange(sw * sh * channels, dtype=f32)
    return v.reshape((sh, sw) if channels == 1 else (sh, sw, channels))


def mask_pattern(sw, sh):
    """8-bit, never 0, horizontally adjacent pixels differ by 7 and vertically adjacent ones by 13 (mod 251)."""
    y, x = np.mgrid[0:sh, 0:sw]
    return ((x * 7 + y * 13) % 251 + 1).astype(np.uint8)


def filled(n):
    return np.full(n, FILL, u32).view(f32)


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    assert g.size == w.size, "%s: %d values, %d expected" % (what, g.size, w.size)
    if g.dtype == f32:
        g, w = g.view(u32), w.view(u32)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: %s vs %s" % (what, bad.size, g.size, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


# ---- walks -------------------------------------------------------------------------------------------------------------------------------------------
def area_branch(x, y, sw, sh, f):
    """Which statement of the rule gives destination pixel (x, y)."""
    if y * f >= sh or x * f >= sw:
        return "outside"
    row_cut, col_cut = y * f + f > sh, x >= sw // f
    return "both" if row_cut and col_cut else "bottom" if row_cut else "right" if col_cut else "full"


def area_walk(src, f):
    """src (sh, sw) float32.  The full blocks are summed in the rule's order, all blocks at once (one IEEE single addition per numpy addition); the cut ones pixel by pixel."""
    sh, sw = src.shape
    dw, dh = scaled(sw, f), scaled(sh, f)
    out = np.zeros((dh, dw), f32)
    fw, fh = sw // f, sh // f                                  # blocks that lie inside
    nw, nh = min(fw, dw), min(fh, dh)
    blk = src[:nh * f, :nw * f].reshape(nh, f, nw, f)
    if f == 2:
        out[:nh, :nw] = ((blk[:, 0, :, 0] + blk[:, 0, :, 1]) + (blk[:, 1, :, 0] + blk[:, 1, :, 1])) * f32(0.25)
    else:
        s = np.zeros((nh, nw), f32)
        for j in range(f):
            for k in range(f):
                s = s + blk[:, j, :, k]
        out[:nh, :nw] = s * f32(f32(1.0) / f32(f * f))
    for y in range(dh):
        for x in range(dw):
            b = area_branch(x, y, sw, sh, f)
            if b == "full":
                continue
            if b == "outside":
                out[y, x] = 0
                continue
            s, n = f32(0), 0
            for j in range(f):
                for k in range(f):
                    if y * f + j < sh and x * f + k < sw:
                        s = f32(s + src[y * f + j, x * f + k]); n += 1
            out[y, x] = f32(s / f32(n))
    return out


def area_mean64(src, f):
    sh, sw = src.shape
    dw, dh = scaled(sw, f), scaled(sh, f)
    out = np.zeros((dh, dw), np.float64)
    for y in range(dh):
        for x in range(dw):
            b = src[y * f:y * f + f, x * f:x * f + f].astype(np.float64)
            out[y, x] = b.mean() if b.size else 0.0
    return out


def nearest_walk(src, dw, dh, rule=nn_index):
    sh, sw = src.shape[:2]
    return src[nn_axis(dh, sh, rule)][:, nn_axis(dw, sw, rule)]


def nearest_down_axis(dn, sn, f):
    """fx = 1 / f is given, so ifx = f exactly: min(d * f, sn - 1)."""
    return np.array([min(d * f, sn - 1) for d in range(dn)], np.int64)


def linear_walk(src, dw, dh):
    sh, sw = src.shape
    x0, a1 = linear_axis(dw, sw)
    y0, b1 = linear_axis(dh, sh)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    a0, b0 = (f32(1) - a1)[None, :], (f32(1) - b1)[:, None]
    a1, b1 = a1[None, :], b1[:, None]
    t0 = src[y0][:, x0] * a0 + src[y0][:, x1] * a1
    t1 = src[y1][:, x0] * a0 + src[y1][:, x1] * a1
    return (t0 * b0 + t1 * b1).astype(f32)


def skew_walk(src):
    """dst[((u + v) mod w) * h + v] = src[v * w + u]"""
    h, w = src.shape
    v, u = np.mgrid[0:h, 0:w]
    out = filled(w * h)
    out[((u + v) % w) * h + v] = src
    return out


def quad_walk(src):
    """dst[(u + v) * h + v] = {I(u, v), I(u + 1, v), I(u, v + 1), I(u + 1, v + 1)}, neighbours clamped at the border; the other entries of the (w + h - 1) * h are not written."""
    h, w = src.shape
    v, u = np.mgrid[0:h, 0:w]
    u1, v1 = np.minimum(u + 1, w - 1), np.minimum(v + 1, h - 1)
    out = filled((w + h - 1) * h * 4).reshape(-1, 4)
    out[(u + v) * h + v] = np.stack([src[v, u], src[v, u1], src[v1, u], src[v1, u1]], axis=-1)
    return out


# ---- the sweeps --------------------------------------------------------------------------------------------------------------------------------------
def area_sizes(f):
    return [(w, h) for w in range(4 * f, 6 * f + 1) for h in range(4 * f, 6 * f + 1)]


def mask_pairs(levels=(1, 2, 3)):
    """(W, l, dw) of the mask-level sweep: every W in 36 .. 300, dw = cvRound(W / 2^l) >= 9."""
    return [(W, l, scaled(W, 1 << l)) for l in levels for W in MASK_WIDTHS if scaled(W, 1 << l) >= 9]


def disagreements():
    """The (W, l) of the sweep at which ifx = sw / dw and ifx = 1 / (dw / sw) pick different columns, from the two formulas."""
    return {(W, l) for W, l, dw in mask_pairs() if not np.array_equal(nn_axis(dw, W, nn_index_old), nn_axis(dw, W))}


def _oracle():
    from oracle import pyoracle
    return pyoracle


def area_cases(engine, f):
    """Every (w, h) in 4f .. 6f squared, one image and three: the kernel's bits are the walk's, the walk is within f^2 ulp of the float64 mean (f^2 rounded operations: the
    additions and the final scale or division), and the oracle's resizeArea is the walk."""
    rng = np.random.default_rng(100 + f)
    seen = set()
    for w, h in area_sizes(f):
        dw, dh = scaled(w, f), scaled(h, f)
        imgs = textured(rng, (3, h, w))
        want = np.stack([area_walk(im, f) for im in imgs])
        for y in range(dh):
            for x in range(dw):
                seen.add(area_branch(x, y, w, h, f))
        if w / f - w // f == 0.5 and dw == w // f:
            seen.add("tie rounds down")
        if w / f - w // f == 0.5 and dw == w // f + 1:
            seen.add("tie rounds up")
        mean = area_mean64(imgs[0], f)
        ulp = np.spacing(np.abs(mean).astype(f32)).astype(np.float64)
        assert np.all(np.abs(want[0].astype(np.float64) - mean) <= f * f * ulp), "area f=%d %dx%d: the walk strays from the float64 mean" % (f, w, h)
        same_bits(_oracle().resize_area(imgs[0], f), want[0], "oracle resizeArea f=%d %dx%d" % (f, w, h))
        for n in (1, 3):
            got = engine.resample(engine.RESAMPLE_AREA, imgs[:n], (w, h), filled(n * dw * dh), (dw, dh), arg=f, n_img=n)
            same_bits(got, want[:n], "area f=%d %dx%d x%d" % (f, w, h, n))
    assert {"full", "right", "bottom", "both", "tie rounds down", "tie rounds up"} <= seen, seen      # (predicate on the walk alone: every branch occurs)
    return seen


def nearest_down_cases(engine, f):
    """The sizes of the area sweep.  The sn - 1 clamp is never the active bound at dn = cvRound(sn / f): (dn - 1) f <= sn - 1 there (asserted on the walk); the kernel's
    clamp is kept for the reference's statement, and this sweep cannot tell whether it is there."""
    for w, h in area_sizes(f):
        dw, dh = scaled(w, f), scaled(h, f)
        assert (dw - 1) * f <= w - 1 and (dh - 1) * f <= h - 1
        xs, ys = nearest_down_axis(dw, w, f), nearest_down_axis(dh, h, f)
        depth, normal = coded(w, h), coded(w, h, 3)
        want = np.concatenate([depth[ys][:, xs].ravel(), normal[ys][:, xs].ravel()])
        got = engine.resample(engine.RESAMPLE_NEAREST_DOWN, np.concatenate([depth.ravel(), normal.ravel()]), (w, h), filled(4 * dw * dh), (dw, dh), arg=f)
        same_bits(got, want, "nearest-down f=%d %dx%d" % (f, w, h))
        same_bits(_oracle().resize_nearest_down(depth, f), depth[ys][:, xs], "oracle resizeNearestDown f=%d %dx%d" % (f, w, h))


def upsample_pairs(transpose):
    """((sw, sh), (dw, dh)): every fine width 10 .. 81 over its coarse cvRound(w / 2), against the heights 11, 12, 13 over 6; or the transpose."""
    for w in UP_WIDTHS:
        for h in UP_HEIGHTS:
            s, d = (scaled(w, 2), scaled(h, 2)), (w, h)
            yield (s[::-1], d[::-1]) if transpose else (s, d)


def upsample_cases(engine, nearest_depth, transpose):
    """pm_upsample_kernel's three outputs: the depth (INTER_LINEAR of a textured map, or with nearestDepth the nearest pixel of an index-coded one), the normal at the
    nearest index, and the prior == the depth, bit for bit."""
    rng = np.random.default_rng(200 + 2 * nearest_depth + transpose)
    for (sw, sh), (dw, dh) in upsample_pairs(transpose):
        depth = coded(sw, sh) if nearest_depth else textured(rng, (sh, sw))
        normal = coded(sw, sh, 3)
        wd = nearest_walk(depth, dw, dh) if nearest_depth else linear_walk(depth, dw, dh)
        wn = nearest_walk(normal, dw, dh)
        got = engine.resample(engine.RESAMPLE_UPSAMPLE, np.concatenate([depth.ravel(), normal.ravel()]), (sw, sh), filled(5 * dw * dh), (dw, dh), arg=nearest_depth)
        what = "upsample %dx%d -> %dx%d nearestDepth=%d" % (sw, sh, dw, dh, nearest_depth)
        P = dw * dh
        same_bits(got[:P], wd, what + " depth")
        same_bits(got[P:4 * P], wn, what + " normal")
        same_bits(got[4 * P:], got[:P], what + " prior")
        same_bits(_oracle().resize_nearest(depth, dw, dh) if nearest_depth else _oracle().resize_linear(depth, dw, dh), wd, "oracle " + what)


def upsample_predicates():
    """On the walk alone: over the pairs of the sweep each clamp of the linear rule decides at least once per axis, and both forms of the scale give the same float
    coefficients and the same nearest index (consecutive levels: gcd(s, 2s +- 1) = 1)."""
    for transpose in (0, 1):
        low = [False, False]; high = [False, False]
        for (sw, sh), (dw, dh) in upsample_pairs(transpose):
            for axis, (sn, dn) in enumerate(((sw, dw), (sh, dh))):
                for d in range(dn):
                    raw = int(np.floor(f32((d + 0.5) * (1.0 / (dn / sn)) - 0.5)))
                    low[axis] |= raw < 0
                    high[axis] |= raw >= sn - 1
                    s0, a0 = linear_coef(d, dn, sn)
                    s1, a1 = linear_coef(d, dn, sn, scale=sn / dn)
                    assert s0 == s1 and a0.view(u32) == a1.view(u32) and nn_index(d, dn, sn) == nn_index_old(d, dn, sn), (sn, dn, d)
        assert all(low) and all(high), (low, high)


def _nearest_gather(engine, kind, sizes, dsizes, what):
    (sw, sh), (dw, dh) = sizes, dsizes
    if kind == engine.RESAMPLE_MASK_LEVEL:
        src, dst = mask_pattern(sw, sh), np.zeros(dw * dh, np.uint8)
    else:
        src, dst = coded(sw, sh), filled(dw * dh)
    want = nearest_walk(src, dw, dh)
    same_bits(engine.resample(kind, src, (sw, sh), dst, (dw, dh)), want, "%s %dx%d -> %dx%d" % (what, sw, sh, dw, dh))
    return src, want


def _collect(bad, key, fn, *args):
    """Run one size of a sweep; a mismatch is noted under `key` and the sweep goes on, so that a failure names every size at which the rule is wrong."""
    try:
        fn(*args)
    except AssertionError as e:
        bad.append((key, str(e)))


def mask_level_cases(engine, transpose, level):
    """pm_mask_level_kernel at every W in 36 .. 300 -> cvRound(W / 2^level) >= 9, the other axis 9 -> 9; or the transpose."""
    bad = []
    for W, l, dw in mask_pairs((level,)):
        s, d = ((9, W), (9, dw)) if transpose else ((W, 9), (dw, 9))
        _collect(bad, (W, dw), _nearest_gather, engine, engine.RESAMPLE_MASK_LEVEL, s, d, "mask level %d" % l)
    assert not bad, "mask level %d: wrong at the (W, dw) %s; first: %s" % (level, [k for k, _ in bad], bad[0][1])


def nearest_up_cases(engine, transpose, level):
    """pm_nearest_up_f_kernel over the sizes of the mask sweep; where the two rules differ also the pair in reverse (14 -> 58).  The oracle's resizeNearest is the walk."""
    dis = disagreements()

    def one(s, d):
        src, want = _nearest_gather(engine, engine.RESAMPLE_NEAREST_UP, s, d, "nearest")
        same_bits(_oracle().resize_nearest(src, d[0], d[1]), want, "oracle resizeNearest %dx%d -> %dx%d" % (s + d))
    bad = []
    for W, l, dw in mask_pairs((level,)):
        for a, b in ((W, dw), (dw, W)) if (W, l) in dis else ((W, dw),):
            s, d = ((9, a), (9, b)) if transpose else ((a, 9), (b, 9))
            _collect(bad, (a, b), one, s, d)
    assert not bad, "nearest: wrong at the (sn, dn) %s; first: %s" % ([k for k, _ in bad], bad[0][1])


def disagreement_predicate():
    """Recomputed from the two formulas: the old rule and the one rule pick different columns at exactly the eleven listed (W, level) of the sweep; in the reverse direction
    some of them differ too (14 -> 58)."""
    dis = disagreements()
    assert dis == KNOWN_DISAGREEMENTS, sorted(dis ^ KNOWN_DISAGREEMENTS)
    back = {(scaled(W, 1 << l), W) for W, l in dis if not np.array_equal(nn_axis(W, scaled(W, 1 << l), nn_index_old), nn_axis(W, scaled(W, 1 << l)))}
    assert (14, 58) in back, sorted(back)                                    # (some of the eleven differ in reverse too, not all: 44 -> 174 does not)
    assert nn_index(7, 14, 58) == 28 and nn_index_old(7, 14, 58) == 29 and nn_index(15, 20, 164) == 123 and nn_index_old(15, 20, 164) == 122


def skew_quad_cases(engine, kind):
    """All pairs of w, h in 9, 10, 33, 64, 65, 130, one image and three, index-coded, against the index formulas of the kernels' comments; quad's clamped right column and
    bottom row are looked at by name, and the entries of a quad image that no pixel owns keep the fill."""
    quad = kind == engine.RESAMPLE_QUAD
    for w in SKEW_SIZES:
        for h in SKEW_SIZES:
            for n in (1, 3):
                src = coded(w, h * n).reshape(n, h, w)          # (images differ: an image read at another's offset shows)
                want = np.stack([(quad_walk if quad else skew_walk)(im) for im in src])
                got = engine.resample(kind, src, (w, h), filled(want.size), (w, h), n_img=n)
                same_bits(got, want, "%s %dx%d x%d" % ("quad" if quad else "skew", w, h, n))
                if quad:
                    q = got.reshape(n, w + h - 1, h, 4)       # [image][u + v][v]
                    for im in range(n):
                        for v in range(h):                       # right column u = w - 1: I(u + 1, .) is I(u, .)
                            e = q[im, w - 1 + v, v]
                            assert e[0] == src[im, v, w - 1] and e[1] == e[0] and e[3] == e[2] == src[im, min(v + 1, h - 1), w - 1]
                        for u in range(w):                       # bottom row v = h - 1: I(., v + 1) is I(., v)
                            e = q[im, u + h - 1, h - 1]
                            assert e[0] == src[im, h - 1, u] and e[2] == e[0] and e[3] == e[1] == src[im, h - 1, min(u + 1, w - 1)]


# ---- grid-stride loops: device only (one 1025 x 1024 destination is 1 049 600 outputs, just above 4096 blocks of 256) ----------------------------------
def grid_stride_case(engine, name):
    dw, dh = 1025, 1024
    if name == "mask_level":
        _nearest_gather(engine, engine.RESAMPLE_MASK_LEVEL, (2050, 2048), (dw, dh), "mask level")
    elif name == "nearest_up":
        _nearest_gather(engine, engine.RESAMPLE_NEAREST_UP, (scaled(dw, 2), scaled(dh, 2)), (dw, dh), "nearest")
    elif name == "nearest_down":
        w, h = 2050, 2048
        assert (scaled(w, 2), scaled(h, 2)) == (dw, dh)
        xs, ys = nearest_down_axis(dw, w, 2), nearest_down_axis(dh, h, 2)
        depth, normal = coded(w, h), coded(w, h, 3)
        got = engine.resample(engine.RESAMPLE_NEAREST_DOWN, np.concatenate([depth.ravel(), normal.ravel()]), (w, h), filled(4 * dw * dh), (dw, dh), arg=2)
        same_bits(got, np.concatenate([depth[ys][:, xs].ravel(), normal[ys][:, xs].ravel()]), "nearest-down, second trip")
    elif name == "upsample":
        sw, sh = scaled(dw, 2), scaled(dh, 2)
        depth, normal = textured(np.random.default_rng(7), (sh, sw)), coded(sw, sh, 3)
        got = engine.resample(engine.RESAMPLE_UPSAMPLE, np.concatenate([depth.ravel(), normal.ravel()]), (sw, sh), filled(5 * dw * dh), (dw, dh), arg=0)
        P = dw * dh
        same_bits(got[:P], linear_walk(depth, dw, dh), "upsample, second trip: depth")
        same_bits(got[P:4 * P], nearest_walk(normal, dw, dh), "upsample, second trip: normal")
        same_bits(got[4 * P:], got[:P], "upsample, second trip: prior")
    elif name == "area_65535":
        # pm_area_kernel's grid stops at 65535 blocks = 16 776 960 outputs; 16 images of 1025 x 1024 are 16 793 600: the smallest whole-image count above it at this size
        n, w, h = 16, 2050, 2048
        assert n * dw * dh > 65535 * 256 >= (n - 1) * dw * dh
        src = np.random.default_rng(8).random((n, h, w), dtype=f32)
        b = src.reshape(n, dh, 2, dw, 2)
        want = ((b[:, :, 0, :, 0] + b[:, :, 0, :, 1]) + (b[:, :, 1, :, 0] + b[:, :, 1, :, 1])) * f32(0.25)
        same_bits(engine.resample(engine.RESAMPLE_AREA, src, (w, h), filled(n * dw * dh), (dw, dh), arg=2, n_img=n), want, "area, second trip of 65535 blocks")
    else:
        raise KeyError(name)


GRID_STRIDE = ("mask_level", "nearest_up", "nearest_down", "upsample", "area_65535")


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------------
E2E_SIZE = (86, 58)            # levels 43 x 29 and 22 x 14: both axes of level 2 are among the eleven pairs


def e2e_mask():
    """One-pixel stripes in both directions, placed so that the two rules read them differently at level 2."""
    w, h = E2E_SIZE
    m = np.full((h, w), 255, np.uint8)
    m[:, 42] = 0; m[28, :] = 0              # read at level 2 by the one rule (column 11, row 7), missed by ifx = sw / dw (43, 29)
    m[:, 17] = 0; m[10, :] = 0              # one that neither rule reads at level 2, one that only level 1 reads
    return m


def level_mask(mask, level, rule=nn_index):
    h, w = mask.shape
    return nearest_walk(mask, scaled(w, 1 << level), scaled(h, 1 << level), rule)


def e2e_predicate():
    """On numpy alone: the level-2 mask of the end-to-end case under the old rule differs from the one under the one rule, in a pixel that changes between ignored and processed."""
    m = e2e_mask()
    new, old = level_mask(m, 2), level_mask(m, 2, nn_index_old)
    assert new.shape == (14, 22) and ((new == 0) != (old == 0)).any()
    assert np.array_equal(level_mask(m, 1), level_mask(m, 1, nn_index_old))          # consecutive levels: unaffected


def e2e_case(engine, scene):
    """86 x 58 with nSubResolutionLevels = 2 and a striped ignore mask: the engine's depth, normal and confidence are the oracle's bit for bit (as test_ignore_mask_parity), and
    the level masks the engine derives from this mask (pm_mask_level_kernel, levels 1 and 2) are the walk's -- the part that still holds the rule when kernel and oracle change together."""
    from openmvs_amd.patchmatch import default_params
    po = _oracle()
    sc = scene
    assert (sc.width, sc.height) == E2E_SIZE
    m = e2e_mask()
    for l in (1, 2):
        want = level_mask(m, l)
        got = engine.resample(engine.RESAMPLE_MASK_LEVEL, m, E2E_SIZE, np.zeros(want.size, np.uint8), want.shape[::-1])
        same_bits(got, want, "level-%d mask of the end-to-end case" % l)
    engine.Init(False)
    ids = [0] + list(sc.neighbors[0])
    got = engine.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[0], sc.dmax[0], params=default_params(seed=3, nSubResolutionLevels=2), mask=m)
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids)
    want = po.estimate_depth_map_masked(views, len(ids), float(sc.dmin[0]), float(sc.dmax[0]), po.default_opt(seed=3, viewID=0, nSubResolutionLevels=2), m, mask_mode=True)
    for k, what in enumerate(("depth", "normal", "conf")):
        same_bits(got[k], want[k], "86 x 58, striped mask: " + what)
    assert not got[0][m == 0].any() and (got[0][m != 0] > 0).mean() > 0.5


def e2e_scene():
    from openmvs_amd import synth
    return synth.make_scene(5, E2E_SIZE[0], E2E_SIZE[1], n_src=4)


# ---- the deviation that stays --------------------------------------------------------------------------------------------------------------
def label_route_agrees_at_level0_size():
    """The reference resamples the label file to every level's size directly; the engine is handed the level-0 mask and resamples that.  With a label image of level 0's
    size the first resampling is the identity, so the two routes agree: on the walk alone, for every (W, level) of the mask sweep, per axis."""
    for W, l, dw in mask_pairs():
        direct = nn_axis(dw, W)                                             # label file (W wide) -> level l
        level0 = nn_axis(W, W)                                              # label file -> level 0: every column itself
        assert np.array_equal(level0, np.arange(W)) and np.array_equal(level0[nn_axis(dw, W)], direct), (W, l)
    # (a label file of another size: two resamplings in a row are not one -- 300 columns -> 58 -> 14 against 300 -> 14)
    assert not np.array_equal(nn_axis(58, 300)[nn_axis(14, 58)], nn_axis(14, 300))
