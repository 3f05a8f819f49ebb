"""Hand-built inputs for the tSGM steps around Match (openmvs_amd/csrc/sgm_post.h, sgm_post.hip, and the device scan of sgm_tsgm.hip): the branches that the maps of
tests/sgm_post_cases.py (noise around one disparity, a smooth sine, a near-identity homography) never reach -- cells that a whole row contends for, distance ties down to
the bit, values that leave int and int16_t, windows with 0..3 or 1680 values, ranges exactly at their limits.

A case is (name, step, args, check, pin): `step` names a method of the backend (the names of openmvs_amd.sgm.SemiGlobalMatcherHIP; `Steps` below gives the oracle, the
host-loop emulation and the reference library the same face), `check(want)` asserts ON THE ORACLE'S RESULT AND THE INPUTS ALONE that the edge the case is named after is
reached, `pin` says whether the reference's own function is defined on the input and has the step at all.  `run` returns the results as a list of arrays and `same` compares two such lists
over every element; the one exception is a NaN result (0 * inf where a projection hits a pixel centre, NaN inputs): its position must coincide, its sign and payload are
not compared (x86 and the GPU produce different ones)."""
import numpy as np

from oracle import pyoracle as po

NO = 32767
SMALL = (67, 37)
THIN = ((3, 70), (70, 3))
LARGE = (131, 83)
INT_LIMIT = 2147483648.0


def must(cond):
    assert cond
    return True


class Case:
    def __init__(self, name, step, args, check=None, pin=True):
        self.name, self.step, self.args, self.check, self.pin = name, step, args, check, pin


class Steps:
    """The oracle's steps (or, with impl / prefix, the host-loop emulation's or the reference library's) under the method names of SemiGlobalMatcherHIP."""

    def __init__(self, impl=None, prefix="orc_sgm_"):
        self.kw = dict(impl=impl, prefix=prefix)

    def ConsistencyCrossCheck(self, a, b, th=1): return po.sgm_cross_check(a, b, th, **self.kw)
    def ExtractMask(self, d, m=None, tv=3): return po.sgm_extract_mask(d, m, tv, **self.kw)
    def UpscaleMask(self, m, size): return po.sgm_upscale_mask(m, size, **self.kw)
    def FlipDirection(self, d): return po.sgm_flip_direction(d, **self.kw)
    def Disparity2RangeMap(self, d, m, a=5, b=7): return po.sgm_disparity2range_map(d, m, a, b, **self.kw)
    def Depth2DisparityMap(self, depth, iH, iQ, steps, size): return po.sgm_depth2disparity_map(depth, iH, iQ, steps, size, **self.kw)
    def Disparity2DepthMap(self, d, c, H, Q, steps, size): return po.sgm_disparity2depth_map(d, c, H, Q, steps, size, **self.kw)
    def ProjectDisparity2DepthMap(self, d, c, Q, steps, size): return po.sgm_project_disparity2depth_map(d, c, Q, steps, size, **self.kw)
    def FusePairs(self, deps, rgs, cfs, mv=2): return po.sgm_fuse_pairs(deps, rgs, cfs, mv, **self.kw)
    def FilterSpeckles(self, d, mx=100, df=5): return po.sgm_filter_speckles(d, mx, df, **self.kw)


ORACLE = Steps()


def run(case, be):
    """-> the step's results as a list of arrays (None where the step returns none)."""
    res = getattr(be, case.step)(*case.args)
    if case.step == "Disparity2RangeMap":
        px, n, mx = res
        return [px["idx"].copy(), px["minDisp"].copy(), px["maxDisp"].copy(), np.array([n, mx], np.int64)]
    if case.step == "ProjectDisparity2DepthMap":
        return [np.array([int(res[0])])] + list(res[1:])
    return list(res) if isinstance(res, tuple) else [res]


def same(got, want, what, skip=None):
    """Every element of every array; NaN results only by position.  skip: per array, a boolean map of elements the reference leaves unset (pinning only)."""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, (what, k)
            continue
        a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            na, nb = np.isnan(a), np.isnan(b)
            ne = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
        else:
            ne = a != b
        if skip is not None and skip[k] is not None:
            ne &= ~skip[k]
        assert not ne.any(), "%s: output %d differs at %d of %d elements (first at %s: %r vs %r)" % (
            what, k, int(ne.sum()), ne.size, tuple(int(v) for v in np.argwhere(ne)[0]), a[tuple(np.argwhere(ne)[0])], b[tuple(np.argwhere(ne)[0])])


def pin_skip(case, want):
    """What the reference leaves unset: range and confidence of ProjectDisparity2DepthMap where it produced no depth."""
    if case.step != "ProjectDisparity2DepthMap":
        return None
    nod = want[1] == 0
    return [None, None, np.repeat(nod[..., None], 2, -1), None if want[3] is None else nod]


# ---- FlipDirection ----------------------------------------------------------------------------------------------------------------------------------------
def flip_cases(w, h):
    out = []
    xs = np.arange(w)
    for x0 in sorted({0, w // 2, w - 1}):
        d = np.tile((x0 - xs).astype(np.int16), (h, 1))                     # every pixel of a row targets column x0: w offers on each of x0 - 1, x0, x0 + 1

        def chk(want, d=d, x0=x0):
            assert int((xs + d[0] == x0).sum()) == w                         # every source offers to x0 - 1, x0, x0 + 1: w offers on x0, 3w on the three cells
            assert np.all(want[0][:, x0] == -(x0 - (w - 1)))                 # the largest column wins
        out.append(Case("flip_funnel_to_%d" % x0, "FlipDirection", (d,), chk))
    d = np.full((h, w), NO, np.int16)
    kinds = (-2, -1, 0, w - 1, w, w + 1)                                       # c + d: one and two outside either border, and the border columns
    for i in range(w * h):
        d[i // w, i % w] = kinds[i % len(kinds)] - i % w
    out.append(Case("flip_clipped_at_both_borders", "FlipDirection", (d,),
                    lambda want, d=d: must([int(((np.arange(w) + d == k)).sum()) > 0 for k in kinds].count(True) == len(kinds))))
    e = np.full((h, w), NO, np.int16)
    e.flat[::3] = -32768; e.flat[1::3] = -32767; e.flat[2::5] = 32766; e[-1, -1] = 0
    out.append(Case("flip_extreme_disparities", "FlipDirection", (e,), lambda want: must((want[0][-1, -1] == 0))))
    out.append(Case("flip_all_invalid", "FlipDirection", (np.full((h, w), NO, np.int16),), lambda want: must(np.all(want[0] == NO))))
    one = np.array([[0], [NO], [5], [-1], [1]], np.int16)
    out.append(Case("flip_width_1", "FlipDirection", (one,), lambda want: must(list(want[0][:, 0]) == [0, NO, NO, 1, -1])))
    return out


def flip_widest():
    """One row of 65534 columns, the widest the 16-bit column key holds: the extreme disparities land inside the map here (-(-32768) wraps to -32768, -(-32767) is NO_DISP's
    own value), and the last column carries the largest key."""
    w = 65534
    d = np.full((1, w), NO, np.int16)
    d[0, 40000] = -32768; d[0, 50000] = -32767; d[0, 100] = 32766; d[0, w - 1] = 0; d[0, w - 2] = 1; d[0, 0] = 0

    def chk(want):
        r = want[0][0]
        assert r[40000 - 32768] == -32768 and r[50000 - 32767] == NO and r[100 + 32766] == -32766 and r[w - 1] == 0 and r[w - 2] == 0 and r[0] == 0
    return Case("flip_65534_columns", "FlipDirection", (d,), chk)


# ---- ConsistencyCrossCheck --------------------------------------------------------------------------------------------------------------------------------
def cross_cases(w, h):
    out = []
    for wr in sorted({max(1, w - 5), w, w + 4}):
        for th in (0, 1, 3):
            l2r = np.full((h, w), NO, np.int16); r2l = np.full((h, wr), NO, np.int16)
            e = (-th - 1, -th, 0, th, th + 1)
            for r in range(h):
                d0 = r % 7 - 3
                for x in range(wr):
                    r2l[r, x] = NO if (x + r) % 11 == 10 else -d0 + e[(x + 2 * r) % 5]
                for c in range(w):
                    k = (r * w + c) % 8
                    l2r[r, c] = (-c - 1, -c, wr - 1 - c, wr - c)[k] if k < 4 else (NO if k == 7 and c % 3 == 0 else d0)

            def chk(want, l2r=l2r, r2l=r2l, wr=wr, th=th):
                cc = np.arange(w)[None, :] + l2r.astype(np.int64)
                ok = l2r != NO
                for v in (-1, 0, wr - 1, wr):
                    assert int((ok & (cc == v)).sum()) > 0, ("no c + d at", v)
                ins = ok & (cc >= 0) & (cc < wr)
                rr, cx = np.nonzero(ins)
                rd = r2l[rr, cc[ins]].astype(np.int64)
                s = np.abs(l2r[ins].astype(np.int64) + rd)[rd != NO]
                assert (s == th).any() and (s == th + 1).any(), "|l + r| at thCross and one above"
                kept = want[0] != NO
                assert kept.any() and (ok & ~kept).any()
            out.append(Case("cross_wr%d_th%d" % (wr, th), "ConsistencyCrossCheck", (l2r, r2l, th), chk))
    return out


# ---- ExtractMask / UpscaleMask ----------------------------------------------------------------------------------------------------------------------------
def mask_cases(w, h):
    out = []
    for tv in (1, 3, w + 5):
        d = np.full((h, w), NO, np.int16)
        counts = []
        for r in range(h):
            n = (0, tv - 1, tv, 2 * tv - 1, w, 2)[r % 6]                     # 2 tv - 1: both scans stop on the same (tv-th) valid pixel
            n = max(0, min(n, w))
            cols = np.linspace(0, w - 1, n).round().astype(int) if n else np.array([], int)
            cols = np.unique(cols)
            d[r, cols] = 4
            counts.append(len(cols))
        given = np.full((h, w), 255, np.uint8); given[(np.arange(h)[:, None] * 5 + np.arange(w)[None, :] * 3) % 7 == 0] = 0

        def chk(want, counts=counts, tv=tv):
            have = set(counts)
            assert 0 in have and (tv > w or {tv - 1, tv} <= have) and (2 * tv - 1 > w or h < 4 or 2 * tv - 1 in have), (tv, sorted(have))      # (three rows hold three kinds)
        out.append(Case("mask_fresh_th%d" % tv, "ExtractMask", (d, None, tv), chk))
        out.append(Case("mask_given_th%d" % tv, "ExtractMask", (d, given, tv), chk))
        out.append(Case("mask_given_all_invalid_th%d" % tv, "ExtractMask", (d, np.zeros((h, w), np.uint8), tv), lambda want: must((not want[0].any()))))
    m = np.where((np.arange(h)[:, None] + 2 * np.arange(w)[None, :]) % 3 == 0, 0, 255).astype(np.uint8)
    for dw in (5, 6, 7, 8):
        for dh in (5, 6, 7, 8):
            out.append(Case("upscale_%d_%d" % (dw, dh), "UpscaleMask", (m, (2 * w + dw, 2 * h + dh)), None))
    return out


# ---- Disparity2RangeMap -----------------------------------------------------------------------------------------------------------------------------------
def window(d, r, c):
    """The valid values Disparity2RangeMap sees around low-resolution pixel (r, c), sorted."""
    hw = 20 if d[r, c] == NO else 3
    v = d[max(0, r - hw):r + hw + 1, max(0, c - hw):c + hw + 1].ravel()
    return np.sort(v[v != NO].astype(np.int64))


def range_masks(w, h):
    m = np.full((2 * h + 6, 2 * w + 7), 255, np.uint8)
    for r, c in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (h // 2, 0), (0, w // 2)):
        m[2 * r + 3, 2 * c + 3] = 0                                             # single pixels cut out, on every border
    return m


def range_cases(w, h):
    out = []
    yy, xx = np.mgrid[0:h, 0:w]
    mask = range_masks(w, h)
    maps = []
    line = np.full(max(w, h), NO, np.int16)                                      # along the long side, on the border line: one value, a pair and a triple, each out of
    line[1] = 9; line[9:11] = (4, 6); line[18:21] = (-5, -7, 30)                 # the others' 7 x 7 windows; beyond position 41 a 41 x 41 window is empty
    s = np.full((h, w), NO, np.int16)
    if w >= h: s[0, :] = line[:w]
    else: s[:, 0] = line[:h]
    maps.append(("sparse", s, lambda st: {0, 1, 2, 3} <= set(st["n"])))
    neg = np.where((xx + yy) % 2 == 0, -3, -2).astype(np.int16); neg[(yy % 3 == 0) & (xx % 3 == 0)] = NO
    maps.append(("negative_odd_middle_sum", neg, lambda st: any(n >= 3 and n % 2 == 0 and (a + b) < 0 and (a + b) % 2 for n, a, b in zip(st["n"], st["m0"], st["m1"]))))
    flat = np.full((h, w), 7, np.int16); flat[h // 2, w // 2] = NO; flat[0, 0] = flat[0, w - 1] = flat[h - 1, 0] = flat[h - 1, w - 1] = NO
    full = min(41, w) * min(41, h) - 1                                           # the widest window this map holds: 1680 equal values from 41 x 41 on (the 1681st, the centre, is the hole)
    maps.append(("flat_with_single_holes", flat, lambda st: max(st["n"]) == full and all(st["span"][i] == 0 for i in range(len(st["n"])) if st["n"][i] >= 3)))
    ext = np.where((xx + yy) % 3 == 0, -32768, np.where((xx + yy) % 3 == 1, 32766, 0)).astype(np.int16); ext[(yy % 4 == 1) & (xx % 5 == 2)] = NO
    maps.append(("int16_extremes", ext, lambda st: 65534 in st["span"] and -32768 in st["lo"] and 32766 in st["hi"]))
    big = np.where((xx + yy) % 2 == 0, 20000, 20001).astype(np.int16); big[(yy % 4 == 1) & (xx % 5 == 2)] = NO
    maps.append(("median_times_2_wraps", big, lambda st: min(st["lo"]) >= 16384))
    for k in (2, 3, 5, 6, 16, 17, 32, 33):                                       # (max - min) * 2 one below / above minNumDisp = 5, 11 and at / above 32 (valid centre), 64 (hole)
        t = (40 + k * ((xx + yy) % 2)).astype(np.int16); t[(yy * w + xx) % 37 == 18] = NO
        maps.append(("two_values_%d_apart" % k, t, lambda st, k=k: any(sp == k and hole for sp, hole in zip(st["span"], st["hole"])) and any(sp == k and not hole for sp, hole in zip(st["span"], st["hole"]))))
    ramp = (((xx * 3 + yy) * 400) % 30000 - 15000).astype(np.int16); ramp[(yy % 4 == 1) & (xx % 6 == 2)] = NO
    maps.append(("wide_ramp", ramp, lambda st: max(st["span"]) * 2 > 32767))
    for name, d, pred in maps:
        def chk(want, d=d, pred=pred, name=name):
            st = dict(n=[], m0=[], m1=[], span=[], lo=[], hi=[], hole=[])
            step = 1 if w * h < 3000 else 3
            for r, c in sorted({(r, c) for r in range(0, h, step) for c in range(0, w, step)} | {(h // 2, w // 2), (0, 1), (1, 0)}):
                if True:
                    v = window(d, r, c); n = len(v)
                    st["n"].append(n); st["hole"].append(d[r, c] == NO)
                    st["m0"].append(int(v[n // 2 - 1]) if n >= 2 else 0); st["m1"].append(int(v[n // 2]) if n >= 1 else 0)
                    st["span"].append(int(v[-1] - v[0]) if n else -1); st["lo"].append(int(v[0]) if n else 0); st["hi"].append(int(v[-1]) if n else 0)
            assert pred(st), name
            lo = want[1].reshape(mask.shape); hi = want[2].reshape(mask.shape)
            assert lo[3, 3] == NO and hi[2 * (h - 1) + 3, 2 * (w - 1) + 3] == NO                # the cut-out pixels have no range
        for a, b in ((11, 33), (5, 7)):
            out.append(Case("range_%s_%d_%d" % (name, a, b), "Disparity2RangeMap", (d, mask, a, b), chk))
    return out


# ---- Depth2DisparityMap / Disparity2DepthMap --------------------------------------------------------------------------------------------------------------
def project_h(H, xs, ys):
    """sgmp_project_h / ProjectVertex_3x3_2_2 in numpy: (u, v) as float32 for integer grids xs, ys."""
    H = np.asarray(H, np.float64)
    with np.errstate(all="ignore"):
        z = H[2, 0] * xs + H[2, 1] * ys + H[2, 2]
        iz = np.where(z == 0, 1e14, 1.0 / np.where(z == 0, 1.0, z))
        return ((H[0, 0] * xs + H[0, 1] * ys + H[0, 2]) * iz).astype(np.float32), ((H[1, 0] * xs + H[1, 1] * ys + H[1, 2]) * iz).astype(np.float32)


def outside_int(*arrs):
    return sum(int((~(np.abs(a.astype(np.float64)) < INT_LIMIT)).sum()) for a in arrs)       # NaN counts too


def shift_h(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)


Q_ID = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 600.0], [0, 0, -1 / 0.3, 1e-3]], np.float64)      # Disparity2Depth: w = d / 0.3 + 1e-3, z = 600 - d
NAN, INF = float("nan"), float("inf")


def conversion_cases(w, h):
    out = []
    yy, xx = np.mgrid[0:h, 0:w]
    cost = ((xx * 37 + yy * 91) % 2600).astype(np.uint16)
    # -- Disparity2DepthMap: the homography's third row vanishes on a pixel column (row); the two border columns (rows) differ in validity
    for axis, col in (("column", min(10, w - 1)), ("row", min(10, h - 1))):
        H = np.array([[1, 0, 0], [0, 1, 0], [1, 0, -col]], np.float64) if axis == "column" else np.array([[1, 0, 0], [0, 1, 0], [0, 1, -col]], np.float64)
        for first_valid in (True, False):
            d = np.full((h, w), NO, np.int16)
            if axis == "column":
                d[:, 0 if first_valid else w - 1] = 8; d[:, 1:w - 1] = ((xx + yy) % 9)[:, 1:w - 1]
            else:
                d[0 if first_valid else h - 1, :] = 8; d[1:h - 1, :] = ((xx + yy) % 9)[1:h - 1, :]

            def chk(want, H=H, axis=axis):
                u, v = project_h(H, xx, yy)
                assert outside_int(u - 3, v - 3) >= (h if axis == "column" else w) - 1
            for cst in (None, cost):
                out.append(Case("d2depth_vanishing_%s_%s_valid_%s" % (axis, "first" if first_valid else "last", "cost" if cst is not None else "nocost"),
                                "Disparity2DepthMap", (d, cst, H, Q_ID, 4, (w, h)), chk))
    dsp = (((xx * 5 + yy * 3) % 23) - 6).astype(np.int16); dsp[(xx + 2 * yy) % 5 == 0] = NO
    dsp.flat[::17] = -32768; dsp.flat[5::19] = 32766
    for name, H in (("nan", [[1, 0, NAN], [0, 1, 0], [0, 0, 1]]), ("inf", [[INF, 0, 0], [0, 1, 0], [0, 0, 1]]), ("minus_inf_row", [[1, 0, 0], [0, 1, -INF], [0, 0, 1]]),
                    ("nan_third_row", [[1, 0, 0], [0, 1, 0], [NAN, 0, 1]])):
        H = np.array(H, np.float64)
        out.append(Case("d2depth_H_%s" % name, "Disparity2DepthMap", (dsp, cost, H, Q_ID, 4, (w, h)), lambda want, H=H: must(outside_int(*project_h(H, xx, yy)) >= min(w, h))))
    # every combination of valid neighbours, coordinates between -1 and 0 (truncation, not floor) and on the last column / row
    r = np.random.RandomState(w * 100 + h)
    half = dsp.copy(); half[r.rand(h, w) < 0.5] = NO

    def quads(valid, u, v):
        lx = np.clip(np.trunc(u).astype(int), 0, w - 1); ly = np.clip(np.trunc(v).astype(int), 0, h - 1)
        lx1 = np.clip(np.trunc(u).astype(int) + 1, 0, w - 1); ly1 = np.clip(np.trunc(v).astype(int) + 1, 0, h - 1)
        return set((valid[ly, lx] * 1 + valid[ly, lx1] * 2 + valid[ly1, lx] * 4 + valid[ly1, lx1] * 8).ravel().tolist())
    for sx, sy in ((3.5, 3.5), (2.5, 3.25), (3.0, 3.0)):
        H = shift_h(sx, sy)

        def chk(want, H=H, sx=sx):
            u, v = project_h(H, xx, yy); u = u - 3; v = v - 3
            q = quads(half != NO, u, v)
            assert len(q) >= (16 if min(w, h) > 3 else 8), sorted(q)
            if sx < 3:
                assert ((u > -1) & (u < 0)).any()
            assert (np.trunc(u) >= w - 1).any() or sx < 3
        out.append(Case("d2depth_neighbour_combinations_%g_%g" % (sx, sy), "Disparity2DepthMap", (half, cost, H, Q_ID, 4, (w, h)), chk))
    # -- Depth2DisparityMap: output grid = the depth map's own grid, (c + 3, r + 3) mapped back by the shift
    dep = (2.0 + 0.01 * ((xx * 7 + yy * 13) % 50)).astype(np.float32)
    hostile = np.array([NAN, INF, -INF, -1.0, 1e-30, 3e38, 1e-40, 0.0], np.float32)
    dep.flat[::3] = hostile[np.arange(dep.flat[::3].size) % hostile.size]
    dep[r.rand(h, w) < 0.35] = 0
    iQ = np.linalg.inv(Q_ID)
    for sx, sy in ((-3.0, -3.0), (-2.5, -2.5), (-3.5, -3.25)):
        def chk(want, sx=sx, sy=sy):
            u, v = project_h(shift_h(sx, sy), xx + 3, yy + 3)
            assert len(quads(dep > 0, u, v)) >= (16 if min(w, h) > 3 else 8)
        for steps in (1, 4, 64):
            out.append(Case("depth2d_hostile_depths_%g_%g_steps%d" % (sx, sy, steps), "Depth2DisparityMap", (dep, shift_h(sx, sy), iQ, steps, (w, h)), chk))
    for axis, col in (("column", min(10, w - 1)), ("row", min(10, h - 1))):
        H = np.array([[1, 0, 0], [0, 1, 0], [1, 0, -col - 3]], np.float64) if axis == "column" else np.array([[1, 0, 0], [0, 1, 0], [0, 1, -col - 3]], np.float64)
        for first_valid in (True, False):
            dd = (2.0 + 0.01 * ((xx + yy) % 9)).astype(np.float32)
            if axis == "column":
                dd[:, w - 1 if first_valid else 0] = 0
            else:
                dd[h - 1 if first_valid else 0, :] = 0
            out.append(Case("depth2d_vanishing_%s_%s_valid" % (axis, "first" if first_valid else "last"), "Depth2DisparityMap", (dd, H, iQ, 4, (w, h)),
                            lambda want, H=H, axis=axis: must(outside_int(*project_h(H, xx + 3, yy + 3)) >= (h if axis == "column" else w) - 1)))
    for name, H in (("nan", [[1, 0, NAN], [0, 1, 0], [0, 0, 1]]), ("inf", [[INF, 0, 0], [0, 1, 0], [0, 0, 1]])):
        out.append(Case("depth2d_H_%s" % name, "Depth2DisparityMap", (dep, np.array(H, np.float64), iQ, 4, (w, h)), None))
    # |w| one step either side of the 1e-7 guard, and disparity * steps beyond int16 and beyond int on both sides: invQ with w = depth, z = -+1000 -> disparity = +-1000 / depth
    g = np.float32(1e-7)
    edge = np.array([np.nextafter(g, np.float32(0)), g, np.nextafter(g, np.float32(1)), 1e-6, 1e-4, 1000 / 40000.0, 1000 / 32767.5, 1000 / 8191.9, 0.5, 2.0, 3e38, 1e-30], np.float32)
    de = edge[(xx + yy * w) % edge.size].astype(np.float32)
    for sign in (1.0, -1.0):
        iQe = np.zeros((4, 4)); iQe[0, 0] = iQe[1, 1] = 1; iQe[3, 2] = 1.0; iQe[2, 3] = -1000.0 * sign

        def chk(want, sign=sign):
            with np.errstate(all="ignore"):
                wv = de.astype(np.float64)
                disp = (-((-1000.0 * sign) / wv)).astype(np.float32)
            ok = np.abs(wv) >= 1e-7
            assert (~ok).any() and ok[de == g].all() and not ok[de == edge[0]].any()               # the guard is straddled by one float
            v = np.floor(disp[ok] * np.float32(4) + np.float32(.5)).astype(np.float64)
            assert (np.abs(v) >= INT_LIMIT).any() and ((np.abs(v) >= 32768) & (np.abs(v) < INT_LIMIT)).any()
            assert ((v < 0).any()) == (sign < 0)
        for steps in (4, 64):
            out.append(Case("depth2d_guard_and_overflow_%s_steps%d" % ("plus" if sign > 0 else "minus", steps), "Depth2DisparityMap", (de, shift_h(-3, -3), iQe, steps, (w, h)), chk if steps == 4 else None))
    return out


# ---- ProjectDisparity2DepthMap ----------------------------------------------------------------------------------------------------------------------------
def q_proj(px=(0, 0, 0, 0), py=(0, 1, 0, 0), z=(0, 0, 0, 1), wq=(0, 0, -0.05, 1)):
    """Q rows as the projection reads them on (x, y, -d, 1): image x, image y (both times 1 / z_raw), z_raw, w; depth = z_raw / w."""
    return np.array([px, py, z, wq], np.float64)


def proj_sources(d, Q, steps):
    """sgmp_disparity2depth_pt in numpy for every valid source: (depth float32, ux, uy float32) and the validity map."""
    h, w = d.shape
    yy, xx = np.mgrid[0:h, 0:w]
    x = xx + 3.0; y = yy + 3.0
    dv = (d.astype(np.float32) / np.float32(steps)).astype(np.float64)
    with np.errstate(all="ignore"):
        ww = Q[3, 0] * x + Q[3, 1] * y - Q[3, 2] * dv + Q[3, 3]
        z = (Q[2, 0] * x + Q[2, 1] * y - Q[2, 2] * dv + Q[2, 3]) / ww
        nrm = 1.0 / (ww * z)
        ux = ((Q[0, 0] * x + Q[0, 1] * y - Q[0, 2] * dv + Q[0, 3]) * nrm).astype(np.float32)
        uy = ((Q[1, 0] * x + Q[1, 1] * y - Q[1, 2] * dv + Q[1, 3]) * nrm).astype(np.float32)
    ok = (d != NO) & ~(np.abs(ww) < 1e-7) & ~(z < 1e-7)
    return z.astype(np.float32), ux, uy, ok


def projection_cases(w, h):
    out = []
    yy, xx = np.mgrid[0:h, 0:w]
    dw, dh = w + 6, h + 6
    cost = ((xx * 37 + yy * 91) % 2600).astype(np.uint16)
    only = lambda d, r, c: np.where((yy == r) & (xx == c), d, NO).astype(np.int16)
    prj = lambda d, Q, steps=1, cst=cost: run(Case("", "ProjectDisparity2DepthMap", (d, cst, Q, steps, (dw, dh))), ORACLE)
    # a Q that ignores u: a whole row lands on one point, every distance bit-equal; the depth tells the winner
    for frac in (0.25, 0.5, 0.0):
        Q = q_proj(px=(0, 0, 0, min(10, w) + frac), py=(0, 1, 0, frac))
        d = (1 + xx % 200).astype(np.int16)

        def chk(want, Q=Q, d=d, frac=frac):
            z, ux, uy, ok = proj_sources(d, Q, 1)
            assert ok.all() and len(set(ux.ravel().view(np.uint32).tolist())) == 1 and all(len(set(uy[r].view(np.uint32).tolist())) == 1 for r in range(h))
            first = prj(np.where(xx == 0, d, NO).astype(np.int16), Q)             # the sources of column 0 alone
            same(want, first, "the smallest source index wins every cell")
            if w > 1 and frac != 0.5:                                             # (at 0.5 every result is the NaN of an exact hit)
                rev = prj(d[:, ::-1].copy(), Q, cst=cost[:, ::-1].copy())
                assert not np.array_equal(rev[1].view(np.uint32), want[1].view(np.uint32)), "the same map in reverse column order gives another result"
            if frac == 0.5:
                assert np.isnan(want[1]).any()                                   # exact hits on pixel centres: weight 0, 0 * inf
            if frac == 0.25:
                assert (want[1] > 0).sum() >= h - 2 and (np.float32(min(10, w) - 1) - (ux[0, 0] - np.float32(.5))) == np.float32(-0.75)      # |distance| = 0.75 exactly is still inside: such offers join the averages
        out.append(Case("proj_row_funnel_%g" % frac, "ProjectDisparity2DepthMap", (d, cost, Q, 1, (dw, dh)), chk))
    # distances one ulp apart: u = 8.25 - d * 2^-20 (one float step per disparity at that magnitude)
    Q = q_proj(px=(0, 0, 2.0 ** -20, 8.25), py=(0, 1, 0, 0.25))
    d = (1 + (xx * 3 + yy) % 4).astype(np.int16)

    def chk_ulp(want, Q=Q, d=d):
        z, ux, uy, ok = proj_sources(d, Q, 1)
        b = np.sort(np.unique(ux.view(np.uint32)))
        assert len(b) == 4 and np.all(np.diff(b.astype(np.int64)) == 1)
    out.append(Case("proj_distances_one_ulp_apart", "ProjectDisparity2DepthMap", (d, cost, Q, 1, (dw, dh)), chk_ulp))
    # two sources mirrored about a pixel centre, depths 9 % apart: the quadrant tie decides, the first quadrant (the source to the right... ddx >= 0) keeps it
    Q = q_proj(px=(0, 0, 0.25, 5.0), py=(0, 1, 0, 0.5))                          # u = 5 - 0.25 d: 4.75 and 4.25, a quarter to either side of pixel 4's centre
    r0 = h // 2
    if w >= 2:
        a = only(1, r0, 0); b = only(3, r0, 1); both = np.where(a != NO, a, b).astype(np.int16)

        def chk_mirror(want, a=a, b=b, Q=Q):
            ra, rb = prj(a, Q), prj(b, Q)
            y = r0 + 3
            assert ra[1][y, 4] > 0 and rb[1][y, 4] > 0 and abs(ra[1][y, 4] - rb[1][y, 4]) / ra[1][y, 4] > 0.02
            z, ux, uy, ok = proj_sources(np.where(a != NO, a, b).astype(np.int16), Q, 1)
            assert (4 - (ux[r0, 0] - np.float32(.5))) == -(4 - (ux[r0, 1] - np.float32(.5))) != 0       # mirrored: equal distances, opposite signs
            winner = ra if (4 - (ux[r0, 0] - np.float32(.5))) >= 0 else rb       # quadrant 0 (ddx >= 0) is visited first and '>' keeps it
            assert want[1][y, 4].view(np.uint32) == winner[1][y, 4].view(np.uint32)
        out.append(Case("proj_mirrored_quadrant_tie", "ProjectDisparity2DepthMap", (both, cost, Q, 1, (dw, dh)), chk_mirror))
        # depth ratios one float either side of 2 %: the centre source has disparity 0 (depth 1 / Q15 = 2), the other one disparity 1 and depth 1 / (0.5 + k), k by bisection
        for side in ("inside", "outside"):
            Dc = np.float32(2.0)
            ratio = lambda x: np.float32(np.abs(Dc - np.float32(x))) / Dc < np.float32(0.02)
            lo, hi = np.float32(2.0), np.float32(2.1)                            # ratio(lo) true, ratio(hi) false: bisect on floats
            while np.nextafter(lo, hi) != hi:
                mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
                if ratio(mid): lo = mid
                else: hi = mid
            target = lo if side == "inside" else hi
            klo, khi = -0.1, 0.0                                                 # depth(k) = 1 / (0.5 + k) falls with k
            for _ in range(200):
                k = (klo + khi) / 2
                v = np.float32(1.0 / (0.5 + k))
                if v == target: break
                if v > target: klo = k
                else: khi = k
            Q2 = q_proj(px=(0, 0, 0.375, 4.625), py=(0, 1, 0, 0.5), wq=(0, 0, -k, 0.5))      # u - 0.5 = 4.125 (d = 0: the centre of pixel 4's cell) and 3.75 (d = 1), in two quadrants
            a = only(0, r0, 0); b = only(1, r0, 1); both = np.where(a != NO, a, b).astype(np.int16)

            def chk_ratio(want, a=a, b=b, Q2=Q2, target=target, side=side):
                z, ux, uy, ok = proj_sources(np.where(a != NO, a, b).astype(np.int16), Q2, 1)
                assert z[r0, 0] == Dc and z[r0, 1] == target and bool(ratio(target)) == (side == "inside") and bool(ratio(np.nextafter(target, np.float32(3 if side == "inside" else 0)))) != (side == "inside")
                ra = prj(a, Q2)
                y = r0 + 3
                mixed = want[1][y, 4].view(np.uint32) != ra[1][y, 4].view(np.uint32)
                assert mixed == (side == "inside"), "the second source joins the average only inside 2 %"
            out.append(Case("proj_depth_ratio_one_ulp_%s_2_percent" % side, "ProjectDisparity2DepthMap", (both, cost, Q2, 1, (dw, dh)), chk_ratio))
    # projections outside the map on every side and coordinates outside int / not numbers
    d = (((xx + yy) % 5)).astype(np.int16); d[(xx + yy) % 7 == 0] = NO
    for name, Q in (("left_top", q_proj(px=(1, 0, 0, -6.5), py=(0, 1, 0, -7.25))), ("right_bottom", q_proj(px=(1, 0, 0, 6.5), py=(0, 1, 0, 7.75))),
                    ("beyond_int", q_proj(px=(1e9, 0, 0, -3e9), py=(0, 1e10, 0, 0))), ("minus_beyond_int", q_proj(px=(-1e10, 0, 0, 0), py=(0, -1e10, 0, 0))),
                    ("nan", q_proj(px=(NAN, 0, 0, 0), py=(0, 1, 0, 0))), ("inf", q_proj(px=(1, 0, 0, 0), py=(0, INF, 0, 0)))):
        def chk_out(want, Q=Q, name=name, d=d):
            z, ux, uy, ok = proj_sources(d, Q, 4)
            if name in ("left_top", "right_bottom"):
                fx, fy = np.floor(ux[ok]), np.floor(uy[ok])
                assert ((fx < -1) | (fy < -1) | (fx > dw) | (fy > dh)).any() and ((want[1] > 0).any() or min(w, h) <= 3)       # (a three-pixel map leaves as a whole)
            else:
                assert outside_int(ux[ok], uy[ok]) > 0
        out.append(Case("proj_%s" % name, "ProjectDisparity2DepthMap", (d, cost, Q, 4, (dw, dh)), chk_out))
    out.append(Case("proj_no_valid_disparity", "ProjectDisparity2DepthMap", (np.full((h, w), NO, np.int16), cost, q_proj(px=(1, 0, 0, 0)), 4, (dw, dh)),
                    lambda want: must((want[0][0] == 0 and not want[1].any()))))
    out.append(Case("proj_extreme_disparities", "ProjectDisparity2DepthMap", (np.where((xx + yy) % 2 == 0, -32768, 32766).astype(np.int16), None, q_proj(px=(1, 0, 0, 0), wq=(0, 0, -1e-6, 1)), 1, (dw, dh)), None))
    return out


# ---- pair fusion ------------------------------------------------------------------------------------------------------------------------------------------
def fusion_cases(w, h, n_pairs=32):
    n = w * h
    kind = np.arange(n).reshape(h, w) % 9
    deps = [np.zeros((h, w), np.float32) for _ in range(n_pairs)]
    rgs = [np.zeros((h, w, 2), np.float32) for _ in range(n_pairs)]
    cfs = [np.full((h, w), 0.01 * (p + 1), np.float32) for p in range(n_pairs)]
    for p in range(n_pairs):
        D, R = deps[p], rgs[p]
        D[kind == 0] = 2.0; R[kind == 0] = (1.9, 2.1)                            # one cluster of every pair
        D[kind == 1] = 2.0; R[kind == 1] = (1.9, 2.0) if p % 2 == 0 else (2.0, 2.1)   # half-open ranges that exclude / include their own depth: a chain of clusters, equal counts
        D[kind == 2] = 2.0 + 0.001 * p; R[kind == 2] = (2.0 + 0.001 * p, 3.0)    # depth on the lower bound (inside)
        D[kind == 3] = 3.0 - 0.001 * p; R[kind == 3] = (3.0 - 0.001 * p - 0.0004, 3.0 - 0.001 * p)    # depth on the upper bound (outside): every pair founds a cluster, the first wins
        D[kind == 4] = 2.0; R[kind == 4] = (2.5, 1.5) if p % 3 == 0 else (1.5, 2.5)   # inverted ranges
        D[kind == 5] = 2.0; R[kind == 5] = (NAN, NAN) if p % 3 == 1 else (1.5, 2.5)   # ranges that are not numbers
        D[kind == 6] = NAN if p == 0 else 0.0; R[kind == 6] = (1.5, 2.5)         # a depth that is not a number (NaN <= 0 is false: it founds a cluster of its own)
        D[kind == 7] = -2.0 if p % 2 else 0.0; R[kind == 7] = (-3.0, 3.0)        # negative and zero depths only
        D[kind == 8] = 2.0 + 0.3 * (p % 3); R[kind == 8] = (1.9 + 0.3 * (p % 3), 2.1 + 0.3 * (p % 3))   # three clusters of 11, 11, 10
    out = []
    for mv in (1, 32, 33):
        def chk(want, mv=mv):
            d = want[0]
            assert np.all((d[kind == 0] > 0) == (mv <= n_pairs)) and not d[kind == 7].any()
            if mv == 1:
                assert np.all(d[kind == 3] == np.float32(3.0)) and np.all(np.isclose(d[kind == 8], 2.0)) and (d[kind == 1] > 0).all()
                assert np.isnan(d[kind == 6]).all()
        out.append(Case("fuse_%d_pairs_min_views_%d" % (n_pairs, mv), "FusePairs", (deps, rgs, cfs, mv), chk))
    return out


# ---- FilterSpeckles ---------------------------------------------------------------------------------------------------------------------------------------
def speckle_cases(w, h):
    from tests import post_filter_cases as pf
    out = []
    serp = [d for name, d, _ in pf.speckle_maps(w, h, 0, 0) if name == "serpentine"][0]
    if w > h:                                                                    # along the long side
        serp = [d for name, d, _ in pf.speckle_maps(h, w, 0, 0) if name == "serpentine"][0].T.copy()
    L = int((serp != NO).sum())
    yy, xx = np.mgrid[0:h, 0:w]
    for mx in (0, 1, L - 1, L):
        for df in (0, 65535):
            def chk(want, mx=mx):
                assert int((want[0] != NO).sum()) == (L if mx < L else 0)        # one component of exactly L pixels
            out.append(Case("speckle_serpentine_%d_%d" % (mx, df), "FilterSpeckles", (serp, mx, df), chk, pin=False))
    for df in (0, 5, 50, 65535):
        ramp = (min(df, 300) * (xx + yy) - 3000).astype(np.int16)
        for mx in (0, 1, w * h - 1, w * h):
            out.append(Case("speckle_ramp_by_maxdiff_%d_%d" % (df, mx), "FilterSpeckles", (ramp, mx, df),
                            lambda want, mx=mx: must(int((want[0] != NO).sum()) == (w * h if mx < w * h else 0)), pin=False))
        if 0 < df < 65535:
            steep = ((df + 1) * (xx + yy) - 3000).astype(np.int16)
            out.append(Case("speckle_ramp_above_maxdiff_%d" % df, "FilterSpeckles", (steep, 1, df), lambda want: must((want[0] == NO).all()), pin=False))
    checker = np.where((xx + yy) % 2 == 0, 7, NO).astype(np.int16)               # diagonal contacts only
    ext = np.where((xx + yy) % 2 == 0, -32768, 32766).astype(np.int16)           # differences of 65534
    for mx in (0, 1):
        out.append(Case("speckle_diagonal_contacts_%d" % mx, "FilterSpeckles", (checker, mx, 65535), lambda want, mx=mx: must(int((want[0] != NO).sum()) == (0 if mx else int((checker != NO).sum()))), pin=False))
    out.append(Case("speckle_extremes_one_component", "FilterSpeckles", (ext, w * h - 1, 65535), lambda want: must((want[0] != NO).all()), pin=False))
    out.append(Case("speckle_extremes_isolated", "FilterSpeckles", (ext, 1, 65533), lambda want: must((want[0] == NO).all()), pin=False))
    n = 5                                                                         # regions of exactly maxSpeckleSize and one more, along the long side
    line = np.full(max(w, h), NO, np.int16); line[0:n] = 10; line[n + 1:2 * n + 2] = 10
    m = np.full((h, w), NO, np.int16)
    if w >= h: m[0, :] = line[:w]
    else: m[:, 0] = line[:h]
    out.append(Case("speckle_regions_at_and_above_the_size", "FilterSpeckles", (m, n, 0), lambda want: must(int((want[0] != NO).sum()) == n + 1), pin=False))
    return out


FAMILIES = dict(flip=flip_cases, cross=cross_cases, masks=mask_cases, ranges=range_cases, conversions=conversion_cases, projection=projection_cases, fusion=fusion_cases,
                speckles=speckle_cases)


def cases(family, size):
    return FAMILIES[family](*size)


def check_family(be, family, size, pin=False, predicates=True):
    """Every case of a family at a size: the predicate on the oracle's result, then `be` against the oracle (pin: the reference library, on the cases it is defined on;
    otherwise twice, so that a state left behind on the engine would show).  -> the number of comparisons."""
    ran = 0
    for c in cases(family, size):
        if pin and not c.pin:
            continue
        what = "%s %dx%d" % ((c.name,) + tuple(size))
        want = run(c, ORACLE)
        if c.check and predicates:
            c.check(want)
        for k in range(1 if pin else 2):
            same(run(c, be), want, what + (", second call" if k else ""), pin_skip(c, want) if pin else None)
            ran += 1
    return ran


# ---- RefineDisparityMap on a hand-built resident problem --------------------------------------------------------------------------------------------------
def refine_problem(w, h):
    """Images and a pixel table whose sums have what the fits branch on: left == right, so the 8-path sum at disparity 0 is 0 under non-zero neighbours.  Ranges of 1, 2, 3
    and 5 disparities around 0; three disparity maps inside every pixel's own range (the engine does not check that: see DESIGN.md): its minimum, its last, the middle."""
    from openmvs_amd import sgm
    r = np.random.RandomState(w + h)
    gray = (r.randint(0, 2, (h, w)) * 255).astype(np.float32)                     # black and white: the contrast at which identical patches cost exactly 0
    gray[:, w // 3:2 * (w // 3)] = 90                                            # a flat third: every sum 0 (0 / 0 in the half-fits, three equal sums in the middle)
    gray[:, 2 * (w // 3):] = np.where(np.arange(w - 2 * (w // 3)) % 3 == 2, 200, 50)[None, :]      # stripes of period 3: disparities 1 and 2 cost the same, 0 and 3 nothing
    bgr = np.full((h, w, 3), 128, np.uint8)                                      # one colour: the bilateral weights are the spatial ones alone
    gray = gray / np.float32(255)                                                # (Match indexes its penalty table by 255 * the gray step: gray lives in [0, 1])
    vw, vh = w - 6, h - 6
    lo_hi = ((0, 1), (0, 2), (-1, 1), (-1, 2), (-2, 3), (0, 3), (-2, 1), (0, 4), (-1, 3), (-3, 1))
    k = (np.arange(vw * vh) * 3 // 2) % len(lo_hi)
    mn = np.array([lo_hi[i][0] for i in k], np.int16).reshape(vh, vw); mx = np.array([lo_hi[i][1] for i in k], np.int16).reshape(vh, vw)
    px, n, mxd = sgm.make_pixels(mn, mx)
    maps = {"minimum": mn.copy(), "last": (mx - 1).astype(np.int16), "middle": ((mn.astype(int) + mx - 1) // 2).astype(np.int16), "zero": np.clip(0, mn, mx - 1).astype(np.int16),
            "upper_middle": np.minimum((mn.astype(int) + mx) // 2, mx - 1).astype(np.int16)}
    for m in maps.values():
        m.flat[::13] = NO
    return bgr, gray, px, n, mxd, mn, mx, maps


def refine_predicates(acc, px, mn, mx, maps):
    """On the oracle's sums: a zero neighbour under a non-zero centre at a range end, equal neighbours on either and on both sides, a centre that is not the minimum."""
    idx = px["idx"].astype(np.int64).reshape(mn.shape)
    st = dict(zero_other=0, eq_prev=0, eq_next=0, eq_both=0, wraps=0, widths=set())
    for name, d in maps.items():
        for (r, c), v in np.ndenumerate(d):
            if v == NO: continue
            lo, hi = int(mn[r, c]), int(mx[r, c]); st["widths"].add(hi - lo)
            assert lo <= v < hi, "a disparity outside its pixel's range would read out of bounds"
            if hi - lo < 2: continue
            a = acc[idx[r, c]:idx[r, c] + hi - lo].astype(np.int64); i = v - lo
            if v == lo: st["zero_other"] += int(a[i + 1] == 0 and a[i] != 0)
            elif v + 1 == hi: st["zero_other"] += int(a[i - 1] == 0 and a[i] != 0)
            else:
                st["eq_prev"] += int(a[i - 1] == a[i] != a[i + 1]); st["eq_next"] += int(a[i + 1] == a[i] != a[i - 1]); st["eq_both"] += int(a[i - 1] == a[i] == a[i + 1])
                st["wraps"] += int(a[i - 1] < a[i] or a[i + 1] < a[i])
    return st


def refine_synthetic():
    """Sums written by hand (the oracle, the host-loop emulation and the reference take them as an argument; the engine only has those of its own Match, where three equal
    sums in a row did not occur): every combination of five values before, at and after the disparity, in the middle and at both ends of ranges of 2 and 3.
    -> (pixel table, sums, {name: disparities})"""
    from openmvs_amd import sgm
    vals = (0, 1, 7, 40000, 65535)
    trip = [(a, b, c) for a in vals for b in vals for c in vals]
    mn = np.zeros((1, 2 * len(trip)), np.int16); mx = np.zeros_like(mn); acc = []
    for i, t in enumerate(trip):
        mx[0, 2 * i] = 3; acc += list(t)                                         # range [0, 3): d = 0, 1, 2
        mx[0, 2 * i + 1] = 2; acc += [t[0], t[1]]                                # range [0, 2): d = 0, 1
    px, n, _ = sgm.make_pixels(mn, mx)
    maps = {"first": mn.copy(), "last": (mx - 1).astype(np.int16), "second": np.ones_like(mn)}
    return px, np.array(acc, np.uint16), maps
