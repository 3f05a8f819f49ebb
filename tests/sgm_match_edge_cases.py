"""Hand-built problems for SemiGlobalMatcher::Match (csrc/sgm_kernels.hip, csrc/sgm_kernels_sub.hip): every problem sits on an edge the kernels are built around -- the
[-MD, 2 MD) line buffer of the path step, the byte and half-word packing at odd idx, the chunk and flush arithmetic, the first-minimum tie rule, the penalty lookup --
and carries a predicate that proves it does.  A predicate is evaluated on the problem's own inputs (`walk` restates which pixels follow which along the eight
directions, with the ranges and the penalty index of every step) or on the oracle's result, never on the engine's, and it is asserted before anything is compared.

check_family runs every problem of a family in the four mappings of work to lanes (one wavefront per line, sub-groups of 8, 16 and 32 lanes) and on both aggregation
routes -- the penalties as given if none exceeds 255 (one byte per direction and entry, summed by sgm_sum_wta_kernel) and the same table with one entry raised to 256
(u16 sums by atomic adds, sgm_wta_sub_kernel); an entry no step uses where there is one, so both routes must give the same integers -- and compares the cost volume, the
8-path sums, the disparity and the cost with oracle.pyoracle.sgm_match bit for bit.  Used on the emulated library (tests/test_emu_sgm_match_edges.py), on the device
(tests/test_zz_gpu_sgm_match_edges.py) and, for the families inside the reference's domain, to pin the oracle itself (tests/test_ref_pinning.py)."""
import numpy as np

from openmvs_amd import sgm
from oracle import pyoracle as po
from tests import sgm_cases as sc

MAPPINGS = (0, 8, 16, 32)                                            # set_sub_group_kernels: 0 = one wavefront per line
DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))   # (dx, dy) of the eight paths
MAX_P2 = max(p for p in range(65536) if 8 * (255 + p) <= 65535)     # the largest penalty whose eight-path sum fits 16 bits
assert MAX_P2 == 7936
F = np.float32


def p2_index(DI):
    """sgmp_p2_index (csrc/sgm_post.h) restated: (the index Match uses, |ROUND2INT(255 DI)| as the reference would index -- None if DI is not finite)."""
    x = F(255) * F(DI)
    if not np.isfinite(x):
        return 255, None
    raw = abs(int(np.floor(np.float64(F(x + F(0.5))))))
    return min(raw, 255), raw


class Problem:
    def __init__(self, name, bgr, gl, gr, mn, mx, P1=3, P2s=None, check=None, kernel=None, routes=None):
        self.name = name
        self.bgr = np.ascontiguousarray(bgr, np.uint8); self.gl = np.ascontiguousarray(gl, np.float32); self.gr = np.ascontiguousarray(gr, np.float32)
        self.mn = np.ascontiguousarray(mn, np.int16); self.mx = np.ascontiguousarray(mx, np.int16)
        h, w = self.gl.shape
        assert self.bgr.shape == (h, w, 3) and self.gr.shape == (h, w) and self.mn.shape == self.mx.shape == (h - 6, w - 6), name
        self.px, self.n, self.mxd = sgm.make_pixels(self.mn, self.mx)
        assert self.n > 0 and 0 < self.mxd <= 256, name
        self.P1 = P1; self.P2s = po.sgm_generate_p2s() if P2s is None else np.ascontiguousarray(P2s, np.uint16)
        self.check = check            # check(problem, oracle result of the first route) asserts the predicate
        self.kernel = kernel          # the path kernel the wide mapping must take on the byte route (dispatch rule below), where the case is about that
        self.only = routes            # None: every route the table allows
        self._walk = None; self._oracle = {}

    @property
    def nd(self):
        return self.mx.astype(np.int64) - self.mn.astype(np.int64)

    def walk(self):
        """{direction: [line, ...]}, a line = [(x, y, rpMin, rpMax, rsMin, rsMax, index, raw index), ...] over its valid pixels in path order: ACCUM_PIXELS
        (SemiGlobalMatcher.cpp:1065-1082) without the sums.  A line starts wherever the pixel before it lies outside the grid (the threaded variant's start sets)."""
        if self._walk is None:
            vh, vw = self.mn.shape
            out = {}
            for dx, dy in DIRS:
                lines = []
                for y0 in range(vh):
                    for x0 in range(vw):
                        if 0 <= x0 - dx < vw and 0 <= y0 - dy < vh:
                            continue
                        x, y, rp, Ip, line = x0, y0, (0, 0), F(0.5), []
                        while 0 <= x < vw and 0 <= y < vh:
                            lo, hi = int(self.mn[y, x]), int(self.mx[y, x])
                            if lo < hi:
                                g = self.gl[y, x]                    # the valid-grid coordinate on the full image: the reference's quirk (:1078)
                                with np.errstate(invalid="ignore", over="ignore"):
                                    i, raw = p2_index(F(g - Ip))
                                line.append((x, y, rp[0], rp[1], lo, hi, i, raw))
                                rp, Ip = (lo, hi), g
                            x += dx; y += dy
                        lines.append(line)
                out[(dx, dy)] = lines
            self._walk = out
        return self._walk

    def steps(self, d=None):
        w = self.walk()
        return [s for k in (w if d is None else [d]) for line in w[k] for s in line]

    def used(self):
        return sorted({s[6] for s in self.steps()})

    def tables(self):
        """{route: P2s}: "byte" = the table as given (max <= 255), "u16" = an entry raised to 256 (a table above 255 as given)."""
        t = {}
        if int(self.P2s.max()) <= 255:
            t["byte"] = self.P2s
            free = [i for i in range(255, -1, -1) if i not in set(self.used())]
            up = self.P2s.copy(); up[free[0] if free else int(np.argmax(self.P2s))] = 256
            t["u16"] = up
        else:
            t["u16"] = self.P2s
        return {k: v for k, v in t.items() if self.only is None or k in self.only}

    def same_integers(self):
        """both routes exist and the raised entry is one no step uses"""
        return len(self.tables()) == 2 and len(self.used()) < 256

    def oracle(self, route):
        if route not in self._oracle:
            self._oracle[route] = po.sgm_match(self.bgr, self.gl, self.gr, self.px, self.n, self.mxd, self.P1, self.tables()[route])
        return self._oracle[route]

    def uniform(self):
        return bool((self.mn == self.mn.flat[0]).all() and (self.mx == self.mx.flat[0]).all() and self.mxd > 0)

    def path_kernel(self, lanes, route):
        """sgmLaunchPaths (csrc/sgm_engine.hip) restated: the engine does not report which kernel it launched, so the rule stands here and its inputs are the problem's."""
        D = self.mxd
        if lanes:
            return "sub<%d,%d>" % (lanes, 64 if D <= 64 else 256)
        NK = 1 if D <= 64 else (2 if D <= 128 else 4)
        if self.uniform() and NK <= 2:
            return "uniform<%d,%s>" % (NK, "staged" if route == "byte" and D % 16 == 0 else ("even" if D % 2 == 0 else "odd"))
        return "path<%d>" % NK


# ---- images -----------------------------------------------------------------------------------------------------------------------------------------
def textured(vw, vh, seed=0, shift=2):
    return sc.stereo_pair(vw + 6, vh + 6, shift, seed=seed)


def flat(vw, vh, v):
    g = np.full((vh + 6, vw + 6), v, np.float32)
    return np.full((vh + 6, vw + 6, 3), int(round(float(v) * 255)), np.uint8), g, g.copy()


def grid(vw, vh):
    return np.meshgrid(np.arange(vw), np.arange(vh))                  # x, y of the valid grid


def ragged(vw, vh, lo=-4, widest=12, seed=0):
    """ranges of 1 .. widest disparities placed by a fixed arithmetic pattern (no pixel invalid)"""
    x, y = grid(vw, vh)
    nd = 1 + (x * 7 + y * 13 + seed * 5 + (x * y) % 3) % widest
    mn = lo + (x * 3 + y * 5 + seed) % 5
    return mn.astype(np.int16), (mn + nd).astype(np.int16)


def count(p, pred, d):
    return sum(1 for s in p.steps(d) if pred(*s))


# ---- range geometry along a line ------------------------------------------------------------------------------------------------------------------------
def fam_overlap():
    """Neighbours alternate between [a, a+W) and [a+W-1, a+2W-1): one common disparity, the previous line is read W-1 entries to either side -- Lp[k-1] and Lp[k+1] touch
    the outermost slots of the three-segment buffer when W is the buffer's width (64, 128, 256: NK = 1, 2, 4; sub-kernel buffers of 64 and 256)."""
    out = []
    for W in (64, 128, 256):
        for axis in ("x", "y"):
            vw, vh = (9, 5) if axis == "x" else (5, 9)
            x, y = grid(vw, vh)
            par = (x if axis == "x" else y) & 1
            a = 3 - W                                                 # the common disparity is 2: inside the image for most pixels, so its costs are textured
            mn = np.where(par == 0, a, a + W - 1); mx = mn + W
            lb, lg, rg = textured(vw, vh, seed=W + len(out))
            sees = {d for d in DIRS if d[0 if axis == "x" else 1] != 0}

            def check(p, o, W=W, sees=sees):
                hit = {d: count(p, lambda x, y, pl, ph, sl, sh, i, r: min(ph, sh) - max(pl, sl) == 1 and abs(sl - pl) == W - 1, d) for d in DIRS}
                assert {d for d in DIRS if hit[d] > 0} == sees, hit
                assert {s[4] - s[2] for s in p.steps() if s[3] > s[2]} >= {W - 1, 1 - W}, "both the step up and the step down"
            out.append(Problem("overlap-W%d-%s" % (W, axis), lb, lg, rg, mn, mx, check=check, kernel="path<%d>" % (W // 64 if W < 256 else 4)))
    return out


def fam_touching():
    """rpMax == rsMin and the mirror: no common disparity by exactly one; then chains whose range shifts by one disparity per pixel."""
    out = []
    for n in (5, 64):
        for axis in ("x", "y"):
            vw, vh = (10, 4) if axis == "x" else (4, 10)
            x, y = grid(vw, vh)
            par = (x if axis == "x" else y) & 1
            mn = np.where(par == 0, 2 - n, 2); mx = mn + n
            lb, lg, rg = textured(vw, vh, seed=n + len(out))
            sees = {d for d in DIRS if d[0 if axis == "x" else 1] != 0}

            def check(p, o, sees=sees):
                up = {d: count(p, lambda x, y, pl, ph, sl, sh, i, r: ph > pl and ph == sl, d) for d in DIRS}
                down = {d: count(p, lambda x, y, pl, ph, sl, sh, i, r: ph > pl and sh == pl, d) for d in DIRS}
                assert {d for d in DIRS if up[d] > 0 and down[d] > 0} == sees, (up, down)
            out.append(Problem("touching-%d-%s" % (n, axis), lb, lg, rg, mn, mx, check=check))
    for k, (cx, cy) in enumerate(((1, 2), (2, 1), (1, -1))):
        vw, vh = 11, 8
        x, y = grid(vw, vh)
        mn = -6 + cx * x + cy * y + (8 if cy < 0 else 0); mx = mn + 9 + (x + y) % 2
        lb, lg, rg = textured(vw, vh, seed=40 + k)

        def check(p, o):
            one = {d: count(p, lambda x, y, pl, ph, sl, sh, i, r: ph > pl and abs(sl - pl) == 1, d) for d in DIRS}
            assert sum(1 for d in DIRS if one[d] > 0) >= 4, one
        out.append(Problem("chain-%d-%d" % (cx, cy), lb, lg, rg, mn, mx, check=check))
    return out


def fam_narrow():
    """Ranges of 1, 2, 0 and negative width among wide neighbours: idx at all four residues mod 4 (the cost kernels pack four bytes to a dword, the sums two to a word),
    numCosts divisible by 4 and not (the two branches of sgm_sum_wta_kernel)."""
    out = []
    widths = (1, 2, 0, 17, 1, -3, 2, 40, 1, 3, -1, 2, 70, 1, 18, 0, 5, 2, 33)
    for rem in (0, 1, 2, 3):
        vw, vh = 11, 7
        x, y = grid(vw, vh)
        nd = np.array(widths)[(x * 5 + y * 7 + rem) % len(widths)]
        mn = -3 + (x + 2 * y) % 4
        total = int(np.maximum(nd, 0).sum()) - max(int(nd[-1, -1]), 0)
        nd[-1, -1] = 4 + (rem - total - 4) % 4                       # the last pixel sets numCosts mod 4
        mx = mn + nd
        lb, lg, rg = textured(vw, vh, seed=60 + rem)

        def check(p, o, rem=rem):
            nd = p.nd.ravel()
            assert p.n % 4 == rem
            assert (nd < 0).any() and (nd == 0).any() and (nd == 1).any() and (nd == 2).any() and (nd > 64).any()
            for wd in (1, 2):
                assert {int(i) & 3 for i in p.px["idx"][nd == wd]} == {0, 1, 2, 3}, "width %d at every residue of idx" % wd
            assert {int(i) & 3 for i in p.px["idx"][nd > 16]} == {0, 1, 2, 3}
        out.append(Problem("narrow-rem%d" % rem, lb, lg, rg, mn, mx, check=check))
    return out


def fam_int16():
    """Ranges at the int16 limits: every window lies outside the image, every cost is 255, the winner is the first entry."""
    out = []
    for n in (1, 7, 64):
        vw, vh = 9, 6
        x, y = grid(vw, vh)
        kind = (x + 2 * y) % 4                                        # 0, 2: ordinary, 1: at -32768, 3: at 32767
        mn, mx = ragged(vw, vh, seed=n)
        mn = np.where(kind == 1, -32768, np.where(kind == 3, 32767 - n, mn)).astype(np.int64); mx = np.where(kind % 2 == 1, mn + n, mx)
        lb, lg, rg = textured(vw, vh, seed=70 + n)

        def check(p, o, kind=kind, n=n):
            d, c, costs, acc = o
            assert int(p.mn.min()) == -32768 and int(p.mx.max()) == 32767
            ext = (kind % 2 == 1).ravel()
            for i in np.flatnonzero(ext):
                a = int(p.px["idx"][i])
                assert (costs[a:a + n] == 255).all()
            assert np.array_equal(d.ravel()[ext], p.mn.ravel()[ext]), "the first entry wins"
            assert (costs != 255).any()
        out.append(Problem("int16-%d" % n, lb, lg, rg, mn, mx, check=check))
    return out


def fam_holes():
    out = []
    vw, vh = 12, 9
    x, y = grid(vw, vh)
    lb, lg, rg = textured(vw, vh, seed=80)
    mn, mx = ragged(vw, vh, seed=1)
    frame = (x == 0) | (y == 0) | (x == vw - 1) | (y == vh - 1)
    mxf = np.where(frame, mn, mx)

    def check_frame(p, o, vw=vw, vh=vh):
        firsts = [line[0] for lines in p.walk().values() for line in lines if line]
        assert firsts and all(0 < s[0] < vw - 1 and 0 < s[1] < vh - 1 for s in firsts) and (p.nd[1:-1, 1:-1] > 0).all()
    out.append(Problem("holes-invalid-frame", lb, lg, rg, mn, mxf, check=check_frame))
    last = (x == vw - 1) & (y == vh - 1)
    for nm, a, b in (("empty", mn, np.where(last, mn + 5, mn)), ("no-disp", np.where(last, mn, 32767), np.where(last, mn + 5, 32767)), ("negative", mn, np.where(last, mn + 5, mn - 4))):
        def check_last(p, o):
            assert (p.nd.ravel()[:-1] <= 0).all() and p.nd.ravel()[-1] == 5 and len(p.steps()) == 8
        out.append(Problem("holes-only-the-last-pixel-%s" % nm, lb, lg, rg, a, b, check=check_last))
    # invalid runs exactly one table chunk long that start on a chunk boundary: 64 pixels for a wavefront per line, 8 / 16 / 32 for the sub-groups
    for L in (8, 16, 32, 64):
        for tr in (False, True):
            vw, vh = (3 * L, 3) if not tr else (3, 3 * L)
            x, y = grid(vw, vh)
            along = y if tr else x
            mn, mx = ragged(vw, vh, widest=6, seed=L)
            mx = np.where(along // L == 1, mn, mx)
            lb, lg, rg = textured(vw, vh, seed=90 + L)

            def check_run(p, o, L=L, tr=tr):
                for d in ((0, 1), (0, -1)) if tr else ((1, 0), (-1, 0)):                  # in both directions the line starts a whole number of chunks before the run
                    for line in p.walk()[d]:
                        t = [abs((s[1] if tr else s[0]) - (line[0][1] if tr else line[0][0])) for s in line]
                        assert t == list(range(L)) + list(range(2 * L, 3 * L))
            out.append(Problem("holes-run-%d%s" % (L, "-T" if tr else ""), lb, lg, rg, mn, mx, check=check_run))
    return out


# ---- grid and line sizes ----------------------------------------------------------------------------------------------------------------------------------
UNIFORM_D = (1, 2, 15, 16, 17, 32, 33, 64, 65, 128, 129)
GRIDS = ((1, 1), (1, 37), (37, 1), (63, 2), (64, 3), (65, 2), (128, 2), (129, 3), (2, 63), (3, 64), (2, 65), (2, 128), (3, 129))


def fam_grids():
    """The cost kernels' 64-pixel tiles, the path kernels' chunks of 64 (8, 16, 32) pixels, the staged flush: every grid uniform (each disparity count at least once)
    and ragged."""
    out = []
    for k, (vw, vh) in enumerate(GRIDS):
        lb, lg, rg = textured(vw, vh, seed=100 + k)
        for j in (k, k + 5) if k < 9 else (k,):
            D = UNIFORM_D[j % len(UNIFORM_D)]
            mn = np.full((vh, vw), -(D // 3), np.int64)
            NK = 1 if D <= 64 else 2
            kern = "path<4>" if D > 128 else "uniform<%d,%s>" % (NK, "staged" if D % 16 == 0 else ("even" if D % 2 == 0 else "odd"))

            def check(p, o, D=D):
                assert p.uniform() and p.mxd == D and p.n == p.mn.size * D
            out.append(Problem("grid-%dx%d-uniform-%d" % (vw, vh, D), lb, lg, rg, mn, mn + D, check=check, kernel=kern))
        mn, mx = ragged(vw, vh, seed=k)
        out.append(Problem("grid-%dx%d-ragged" % (vw, vh), lb, lg, rg, mn, mx, check=lambda p, o: _assert(p.mn.size == 1 or not p.uniform())))
    assert {p.mxd for p in out if p.uniform() and "uniform" in p.name} >= set(UNIFORM_D)
    return out


def fam_flush():
    """One uniform problem with D a multiple of 16 on a 66 x 66 grid: the diagonal lines take every length 1 .. 66, so the staged flush of the uniform path kernel
    (32 pixels of delta bytes in LDS, written out at done & 31 == 0 and at the end of the line) ends on every value of done & 31 and a line crosses a 64-pixel chunk."""
    vw = vh = 66
    lb, lg, rg = textured(vw, vh, seed=7)
    mn = np.full((vh, vw), -5, np.int64)

    def check(p, o):
        for d in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            assert {len(line) for line in p.walk()[d]} == set(range(1, 67))
        assert p.mxd % 16 == 0 and {n & 31 for n in range(1, 67)} == set(range(32))
    return [Problem("flush-66x66-D16", lb, lg, rg, mn, mn + 16, check=check, kernel="uniform<1,staged>")]


# ---- image content --------------------------------------------------------------------------------------------------------------------------------------------
def fam_content():
    out = []
    for v in (0.0, 128.0 / 255.0, 1.0):                               # flat images: every sum ties, the first minimum decides
        for uni in (True, False):
            vw, vh = 13, 7
            lb, lg, rg = flat(vw, vh, F(v))
            if uni:
                mn = np.full((vh, vw), -2, np.int64); mx = mn + 6
            else:
                x, y = grid(vw, vh)                                   # ranges that differ from pixel to pixel and still share most disparities
                mn = -3 + (x + y) % 2; mx = mn + 6 + (x * 3 + y) % 3

            def check(p, o):
                d, c, costs, acc = o
                tied = wide = 0
                for i in np.flatnonzero(p.nd.ravel() >= 2):
                    a = acc[int(p.px["idx"][i]):int(p.px["idx"][i]) + int(p.nd.ravel()[i])]
                    wide += 1; tied += int((a == a.min()).sum() > 1)
                assert tied * 2 > wide > 0, (tied, wide)
            out.append(Problem("flat-%.3f-%s" % (v, "uniform" if uni else "ragged"), lb, lg, rg, mn, mx, check=check))
    for axis in (0, 1):                                               # a step edge 0 -> 1: the grey difference is exactly 1, the table's last entry is used
        vw, vh = 12, 10
        g = np.zeros((vh + 6, vw + 6), np.float32)
        if axis:
            g[:, 5:] = 1
        else:
            g[4:, :] = 1
        b = np.repeat((g * 255).astype(np.uint8)[..., None], 3, 2)
        mn, mx = ragged(vw, vh, lo=-3, widest=7, seed=4)

        def check(p, o):
            assert sum(1 for s in p.steps() if s[7] == 255) > 0 and max(s[7] for s in p.steps()) == 255
        out.append(Problem("step-edge-%s" % "xy"[1 - axis], b, g, np.roll(g, 1, axis), mn, mx, check=check))
    # black and white first pixels of lines: from the start value 0.5 they give index 128 (white: ROUND2INT(127.5)) and 127 (black: ROUND2INT(-127.5) = -127)
    vw, vh = 10, 8
    lb, lg, rg = textured(vw, vh, seed=5)
    lg = lg.copy(); x, y = grid(vw, vh)
    border = (x == 0) | (y == 0) | (x == vw - 1) | (y == vh - 1)
    lg[:vh, :vw][border] = ((x + y) % 2)[border].astype(np.float32)    # (the path reads the grey image at the valid-grid coordinate)
    mn, mx = ragged(vw, vh, seed=6)

    def check_first(p, o):
        firsts = {line[0][7] for lines in p.walk().values() for line in lines if line}
        assert firsts == {127, 128}, firsts
    out.append(Problem("black-and-white-line-starts", lb, lg, rg, mn, mx, check=check_first))
    # colour extremes: a centre pixel differs by 255 in every channel from all 48 neighbours of its window, the weights are at their smallest
    vw, vh = 11, 9
    lb, lg, rg = textured(vw, vh, seed=8)
    yy, xx = np.mgrid[0:vh + 6, 0:vw + 6]
    lone = (xx % 5 == 0) & (yy % 5 == 0)
    lb = np.repeat(np.where(lone, 255, 0).astype(np.uint8)[..., None], 3, 2)
    mn, mx = ragged(vw, vh, seed=7)

    def check_colour(p, o):
        hit = 0
        for r in range(vh):
            for c in range(vw):
                win = p.bgr[r:r + 7, c:c + 7].astype(int)
                diff = np.abs(win - win[3, 3])
                diff[3, 3] = 255
                hit += int((diff == 255).all())
        assert hit > 0
    out.append(Problem("colour-extremes", lb, lg, rg, mn, mx, check=check_colour))
    return out


def fam_tiny():
    """Grey values around 1e-20 and a few subnormal ones: the products of the cost sums underflow.  The score of such a window is a subnormal number over sqrt(eps), and
    whether a side keeps it or flushes it to zero the cost is 255 (ncc <= 0, or ROUND2INT(255 (1 - ncc)) with a tiny ncc): what the family pins is that the underflow
    produces no NaN and no other cost on either side, and that the path steps (grey differences of 1e-20: index 0) and the ties of an all-255 volume agree."""
    out = []
    for uni in (True, False):
        vw, vh = 12, 8
        lb, lg, rg = textured(vw, vh, seed=9)
        lg = (lg * F(1e-20)).astype(np.float32); rg = (rg * F(1e-20)).astype(np.float32)
        for img in (lg, rg):
            img[2, 3] = F(1e-40); img[5, 7] = F(1.4e-45); img[7, 11] = F(-3e-39); img[9, 4] = F(1.17549e-38)
        if uni:
            mn = np.full((vh, vw), -3, np.int64); mx = mn + 8
        else:
            mn, mx = ragged(vw, vh, seed=9)

        def check(p, o):
            tiny = np.finfo(np.float32).tiny
            for img in (p.gl, p.gr):
                assert ((img != 0) & (np.abs(img) < tiny)).sum() >= 3 and float(np.abs(img).max()) < 2e-20
            assert float(np.abs(p.gl).max()) ** 2 < tiny               # a product of two grey values is subnormal or zero
            assert (o[2] == 255).all() and p.used() == [0, 127]        # (127: the first pixel of a line, ROUND2INT(255 (0 - 0.5)) = -127)
        out.append(Problem("tiny-%s" % ("uniform" if uni else "ragged"), lb, lg, rg, mn, mx, check=check))
    return out


# ---- penalties ------------------------------------------------------------------------------------------------------------------------------------------------
def _penalty_problems(tag, P1, P2s, check=None, routes=None):
    out = []
    for uni in (True, False):
        vw, vh = 14, 9
        lb, lg, rg = textured(vw, vh, seed=11)
        if uni:
            mn = np.full((vh, vw), -3, np.int64); mx = mn + 13
        else:
            mn, mx = ragged(vw, vh, lo=-3, widest=13, seed=11)
        out.append(Problem("penalties-%s-%s" % (tag, "uniform" if uni else "ragged"), lb, lg, rg, mn, mx, P1=P1, P2s=P2s, check=check, routes=routes))
    return out


def fam_penalties():
    """What Match must compute exactly: P1 at the smallest entry of the table, P1 = 0, an entry of 0, a table that is not monotone, a largest entry of 255 (bytes) against
    256 (u16 sums) on the same problem, and the largest penalties whose eight-path sums fit 16 bits."""
    d = po.sgm_generate_p2s()
    out = _penalty_problems("P1-at-the-smallest-entry", int(d.min()), d, check=lambda p, o: _assert(p.P1 == int(p.P2s.min()) and p.P1 > 3))
    out += _penalty_problems("P1-zero", 0, d)
    z = d.copy(); z[:3] = 0; z[7] = 0

    def check_zero(p, o):
        assert {i for i in p.used() if p.P2s[i] == 0}, "a step uses an entry of 0"
    out += _penalty_problems("entry-zero", 0, z, check=check_zero)
    nm = (4 + (np.arange(256) * 37) % 57).astype(np.uint16)

    def check_nm(p, o):
        u = p.used()
        assert any(nm[a] > nm[b] for a, b in zip(u, u[1:])) and any(nm[a] < nm[b] for a, b in zip(u, u[1:]))
    out += _penalty_problems("not-monotone", 3, nm, check=check_nm)
    top = d.copy(); top[:6] = 255

    def check_top(p, o):
        assert int(p.P2s.max()) == 255 and any(p.P2s[i] == 255 for i in p.used()) and p.same_integers()
        assert int(p.tables()["u16"].max()) == 256 and not any(p.tables()["u16"][i] == 256 for i in p.used())
    out += _penalty_problems("255-against-256", 3, top, check=check_top)
    over = d.copy(); over[:6] = 256                                    # 256 where steps use it: one more than a byte holds

    def check_over(p, o):
        assert int(p.P2s.max()) == 256 and any(p.P2s[i] == 256 for i in p.used()) and list(p.tables()) == ["u16"]
    out += _penalty_problems("256-used", 3, over, check=check_over)
    full = np.full(256, MAX_P2, np.uint16)

    def check_full(p, o):
        assert 8 * (255 + int(p.P2s.max())) <= 65535 < 8 * (255 + int(p.P2s.max()) + 1) and int(o[3].max()) > 32767      # the top bit of a sum's half of its word
    out += _penalty_problems("largest", 3, full, check=check_full)
    out += _penalty_problems("largest-with-P1", MAX_P2, full, check=check_full)
    # one pixel: all eight paths start on it and pay P2; the costs whose windows leave the image are 255, their sums 8 (255 + 7936) = 65528
    lb, lg, rg = textured(1, 1, seed=13, shift=0)
    out.append(Problem("penalties-largest-one-pixel", lb, lg, rg, np.full((1, 1), -5), np.full((1, 1), 6), P2s=full, check=lambda p, o: _assert(int(o[3].max()) == 65528 and int(o[3].min()) < 65528)))
    return out


def _assert(v):
    assert v


def refused():
    """(P1, P2s, why): penalties the engine must refuse with SGMError -- it would compute them silently wrong."""
    d = po.sgm_generate_p2s()
    one = d.copy(); one[200] = MAX_P2 + 1
    low = d.copy(); low[255] = 2
    return [(int(d.min()) + 1, d, "P1 one above the smallest entry"), (40, d, "P1 inside the table's values"), (3, low, "one entry below P1"),
            (3, one, "one entry of 7937: 8 (255 + P2) = 65536"), (3, np.full(256, 65535, np.uint16), "65535 everywhere")]


# ---- grey values the lookup was not written for ------------------------------------------------------------------------------------------------------------------
def fam_grey():
    """Grey values outside [0, 1] and not finite.  The lookup is defined as min(|ROUND2INT(255 DI)|, 255), 255 for a DI that is not finite, and a score that is not
    finite costs 255 (csrc/sgm_post.h); the oracle shares both definitions, the reference has none."""
    out = []
    vw, vh = 13, 9
    lb, lg, rg = textured(vw, vh, seed=12)
    for uni in (True, False):
        if uni:
            mn = np.full((vh, vw), -3, np.int64); mx = mn + 9
        else:
            mn, mx = ragged(vw, vh, lo=-3, widest=9, seed=12)
        u = "uniform" if uni else "ragged"

        def check_over(p, o):
            raws = [s[7] for s in p.steps()]
            assert None not in raws and max(raws) > 255 and sum(1 for r in raws if r > 255) > 8
        out.append(Problem("grey-x3-" + u, lb, lg * F(3), rg * F(3), mn, mx, check=check_over))
        out.append(Problem("grey-0-255-" + u, lb, lg * F(255), rg * F(255), mn, mx, check=check_over))
        for nm, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            g = lg.copy(); g[0, 0] = v; g[0, 5] = v; g[4, 0] = v; g[vh - 1, vw - 1] = v; g[4, 6] = v; g[5, 7] = v       # on lines' first pixels and off them

            def check_nf(p, o):
                for first in (True, False):
                    assert sum(1 for lines in p.walk().values() for line in lines for k, s in enumerate(line) if s[7] is None and (k == 0) == first) > 0
                assert (o[2] != 255).any()
            out.append(Problem("grey-left-%s-%s" % (nm, u), lb, g, rg, mn, mx, check=check_nf))
        g = rg.copy(); g[6, 8] = np.nan; g[3, 2] = np.nan

        def check_right(p, o):
            assert np.isnan(p.gr).sum() == 2 and np.isfinite(p.gl).all() and (o[2] != 255).any()
        out.append(Problem("grey-right-nan-" + u, lb, lg, g, mn, mx, check=check_right))
    return out


# family -> (builder, inside the reference's domain: grey values in [0, 1], P1 <= P2, penalties within the bound)
FAMILIES = {"overlap": (fam_overlap, True), "touching": (fam_touching, True), "narrow": (fam_narrow, True), "int16": (fam_int16, True), "holes": (fam_holes, True),
            "grids": (fam_grids, True), "flush": (fam_flush, True), "content": (fam_content, True), "tiny": (fam_tiny, True), "penalties": (fam_penalties, True),
            "grey": (fam_grey, False)}
_BUILT = {}


def problems(family):
    if family not in _BUILT:
        _BUILT[family] = FAMILIES[family][0]()
        assert len({p.name for p in _BUILT[family]}) == len(_BUILT[family])
    return _BUILT[family]


def prove(p):
    """the predicates of a problem, on its inputs and on the oracle's result; -> the oracle's result per route"""
    want = {r: p.oracle(r) for r in p.tables()}
    if p.check:
        p.check(p, want[sorted(want)[0]])
    if p.same_integers():
        for a, b, nm in zip(want["byte"], want["u16"], NAMES):
            assert np.array_equal(a, b), "%s: the oracle's %s changes with an entry no step uses" % (p.name, nm)
    if p.kernel:
        assert p.path_kernel(0, sorted(want)[0]) == p.kernel, (p.name, p.path_kernel(0, sorted(want)[0]), p.kernel)
    return want


NAMES = ("disparity", "cost", "cost volume", "8-path sums")


def same(got, want, what):
    for nm, a, b in ((NAMES[2], got[2], want[2]), (NAMES[3], got[3], want[3]), (NAMES[0], got[0], want[0]), (NAMES[1], got[1], want[1])):
        assert np.array_equal(a, b), "%s: %s: %d of %d differ" % (what, nm, int((a != b).sum()), a.size)


def run(m, p, lanes, P2s, P1=None):
    m.set_sub_group_kernels(lanes)
    m.P1 = p.P1 if P1 is None else P1; m.P2s = np.ascontiguousarray(P2s, np.uint16)
    m.set_problem(p.bgr, p.gl, p.gr, p.px, p.n, p.mxd)
    m.Match()
    return m.results(volumes=True)


def check_family(m, family, mappings=MAPPINGS, order=None):
    """Every problem of the family on matcher `m`: predicates first, then every mapping x route against the oracle.  `order` permutes the problems (the device test
    interleaves sizes); -> the number of engine runs compared."""
    saved = m.P1, m.P2s
    ps = problems(family)
    runs = 0
    try:
        for i in (order if order is not None else range(len(ps))):
            p = ps[i]
            want = prove(p)
            for lanes in mappings:
                for route, table in p.tables().items():
                    same(run(m, p, lanes, table), want[route], "%s, %s lanes, %s route (%s)" % (p.name, lanes or 64, route, p.path_kernel(lanes, route)))
                    runs += 1
    finally:
        m.P1, m.P2s = saved
        m.set_sub_group_kernels(0)
    return runs


def ordinary():
    return problems("touching")[-1]


def check_refusals(m, mappings=(0, 16)):
    """Every refused penalty set raises SGMError from Match and from the resident tSGM loop, and the engine computes an ordinary problem right afterwards."""
    saved = m.P1, m.P2s
    p = ordinary()
    want = prove(p)
    lb, lg, rg = sc.stereo_pair(64, 48, 3, seed=2)
    mask = np.full((48, 64), 255, np.uint8)
    try:
        for lanes in mappings:
            same(run(m, p, lanes, p.tables()["byte"]), want["byte"], "before the refusals")
            for P1, P2s, why in refused():
                try:
                    run(m, p, lanes, P2s, P1=P1)
                except sgm.SGMError as e:
                    assert "P1" in str(e) or "65535" in str(e), str(e)
                else:
                    raise AssertionError("Match accepted %s" % why)
                same(run(m, p, lanes, p.tables()["u16"]), want["u16"], "after the refusal of %s" % why)
        for P1, P2s, why in refused()[1::2]:
            m.P1, m.P2s = P1, P2s
            try:
                m.tsgm_match(lb, lb, lg, rg, mask, mask, min_resolution=20)
            except sgm.SGMError:
                pass
            else:
                raise AssertionError("tsgm_match accepted %s" % why)
        m.P1, m.P2s = saved
        assert m.tsgm_match(lb, lb, lg, rg, mask, mask, min_resolution=20)[2] >= 1
        same(run(m, p, 0, p.tables()["byte"]), want["byte"], "after the refused loops")
    finally:
        m.P1, m.P2s = saved
        m.set_sub_group_kernels(0)
