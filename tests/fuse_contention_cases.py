"""Adversarial inputs for the depth-map fusion (csrc/pm_fuse.h through pmhip_scene_fuse), shared by the emulator suite (tests/test_emu_fuse_contention.py), the device
suite (tests/test_zz_gpu_fuse_contention.py) and the pin to the reference's own function (tests/test_ref_fuse.py).  The other fusion tests feed it noisy ground truth
seen by similar cameras, on which two seeds rarely share a neighbour cell; the scenes here are built for what those never contain: sixteen or thousands of seeds per
cell, seeds whose outcome depends on what an earlier seed of the same cell did, points of seventeen views with shuffled neighbour lists, thresholds straddled by one
ulp, views of their own sizes funnelling into each other, depths / confidences / normals that are not numbers, and kept points placed on the compaction's tile borders.

All cameras share one centre and look down +z (one looks backwards), so a pixel's ray alone decides the neighbour cell it projects to and the contention can be derived
by hand: a neighbour whose focal length is 1/r of the seed view's receives r x r seeds per cell.  Principal points are offset by .3 (.01 under the 1/64 funnel, where the
projections are 1/64 apart) so that no projection is near an x.5 rounding boundary, except where a case puts it there on purpose with a power-of-two focal length.

Every expected value comes from the sequential oracle (oracle.pyoracle.fuse_depth_maps), every comparison is exact (fuse_cases.same_cloud), and every case carries a
predicate that is asserted on the oracle's result and the inputs alone: a scene that does not do what its name claims must not pass silently."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po

F = np.float32
SMALL = (67, 37)             # odd both ways; 2479 pixels = two full compaction tiles and one of 431, not divisible by 4
THIN = ((9, 70), (70, 9))    # the narrowest scenes the engine holds; 630 pixels: less than one tile
LARGE = (131, 83)            # device only (and the emulator once, for the round count): 10 873 pixels; funnel64 packs 64 x 64 = 4096 seeds into one cell there
Z0 = 4.0
HERE = os.path.dirname(os.path.abspath(__file__))


class Case:
    """A scene with its maps and fusion options: the attributes PatchMatchHIP.scene_load reads and the lists po.fuse_depth_maps takes."""

    def __init__(self, name, sizes, K, deps, nbs, R=None, nrms=None, cnfs=None, bgrs=None, order=None, check=None, **kw):
        n = len(sizes)
        self.name, self.n_views, self.sizes = name, n, [tuple(s) for s in sizes]
        self.width, self.height = self.sizes[0]
        self.K = [np.array(k, np.float64) for k in K]
        self.R = [np.eye(3) for _ in range(n)] if R is None else [np.array(r, np.float64) for r in R]
        self.C = [np.zeros(3) for _ in range(n)]
        self.neighbors = [np.array(x, np.int32) for x in nbs]
        self.gray = [np.zeros((h, w), F) for w, h in self.sizes]          # (fusion does not read the gray images)
        self.dmin = [0.5] * n; self.dmax = [100.0] * n
        self.deps = [np.ascontiguousarray(d, F) for d in deps]
        self.nrms = [np.tile(F([0, 0, -1]), (h, w, 1)) for w, h in self.sizes] if nrms is None else [np.ascontiguousarray(x, F) for x in nrms]
        self.cnfs = [conf_pattern(w, h, v) for v, (w, h) in enumerate(self.sizes)] if cnfs is None else [np.ascontiguousarray(x, F) for x in cnfs]
        self.bgrs = [bgr_pattern(w, h, v) for v, (w, h) in enumerate(self.sizes)] if bgrs is None else bgrs
        self.order = list(order) if order is not None else po.fuse_order([len(x) for x in nbs])
        self.kw = kw
        self.check = check                                                # check(case, oracle cloud): the predicate
        for v, (w, h) in enumerate(self.sizes):
            assert self.deps[v].shape == (h, w) and self.nrms[v].shape == (h, w, 3) and self.cnfs[v].shape == (h, w)

    @property
    def mixed(self):
        return len(set(self.sizes)) > 1

    def nbs(self):
        return [list(int(b) for b in x) for x in self.neighbors]

    def fuse(self, fn=None, order=None):
        return po.fuse_depth_maps(self.deps, self.nrms, self.cnfs, self.bgrs, self.K, self.R, self.C, self.nbs(), order=self.order if order is None else order, fn=fn, **self.kw)

    def load(self, engine):
        engine.scene_load(self, n_levels=0)
        for v in range(self.n_views):
            engine.scene_set_maps(v, self.deps[v], self.nrms[v]); engine.scene_set_conf(v, self.cnfs[v]); engine.scene_set_color(v, self.bgrs[v])


def conf_pattern(w, h, v):
    ys, xs = np.mgrid[0:h, 0:w]
    return (0.2 + 0.7 * ((xs * 3 + ys * 5 + v * 7) % 17) / 17.0).astype(F)


def bgr_pattern(w, h, v):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([(xs * 7 + ys * 13 + v * 29 + k * 50) % 256 for k in range(3)], -1).astype(np.uint8)


def Kmat(f, w, h, off=0.0):
    return [[f, 0, (w - 1) // 2 + off], [0, f, (h - 1) // 2 + off], [0, 0, 1]]


def plane(w, h, z=Z0):
    return np.full((h, w), z, F)


def cell_map(case, a, b):
    """The pixel index in view b that every pixel of view a projects to (-1: nowhere), from the geometry in float64.  Only used on cases that keep every projection
    away from a rounding boundary, where it cannot disagree with the float arithmetic of the code under test."""
    (wa, ha), (wb, hb) = case.sizes[a], case.sizes[b]
    ys, xs = np.mgrid[0:ha, 0:wa].astype(np.float64)
    Ka, Kb = case.K[a], case.K[b]
    z = case.deps[a].astype(np.float64)
    cam = np.stack([(xs - Ka[0, 2]) * z / Ka[0, 0], (ys - Ka[1, 2]) * z / Ka[1, 1], z], -1)
    X = cam @ case.R[a] + case.C[a]                                       # R^T cam + C
    q = (X - case.C[b]) @ (Kb @ case.R[b]).T
    with np.errstate(all="ignore"):
        xb = np.floor(q[..., 0] / q[..., 2] + .5); yb = np.floor(q[..., 1] / q[..., 2] + .5)
        ok = (q[..., 2] > 0) & (xb >= 0) & (yb >= 0) & (xb < wb) & (yb < hb) & (case.deps[a] != 0)
    return np.where(ok, yb * wb + xb, -1).astype(np.int64).ravel()


def max_population(case, a, b):
    """The largest number of seeds of view a that share one cell of view b: they commit one per round, so fusing a takes at least this many rounds."""
    m = cell_map(case, a, b)
    return int(np.bincount(m[m >= 0]).max()) if (m >= 0).any() else 0


def views_per_point(r):
    return np.diff(r["viewStart"].astype(np.int64))


def canon(r):
    """The cloud with every NaN replaced by one NaN: the sign and payload of a NaN that an operation makes (inf - inf, 0 * inf) are the processor's choice -- x86 sets the
    sign bit, the GPU does not -- and no part of the result.  Only the hostile case produces any."""
    r = dict(r)
    for k in ("points", "weights", "normals"):
        if r[k] is not None:
            a = r[k].copy(); a[np.isnan(a)] = np.float32(np.nan); r[k] = a
    return r


def reversed_case(case):
    """The same scene with every image turned by 180 degrees (and every camera about its axis): the pixels of an image are then visited in reverse raster order."""
    S = np.diag([-1.0, -1.0, 1.0])
    K = []
    for k, (w, h) in zip(case.K, case.sizes):
        k = k.copy(); k[0, 2] = w - 1 - k[0, 2]; k[1, 2] = h - 1 - k[1, 2]; K.append(k)
    flip = lambda a: np.ascontiguousarray(a[::-1, ::-1])
    return Case(case.name + "_reversed", case.sizes, K, [flip(d) for d in case.deps], case.nbs(), R=[S @ r for r in case.R],
                nrms=[flip(n) * F([-1, -1, 1]) for n in case.nrms], cnfs=[flip(c) for c in case.cnfs], bgrs=[flip(b) for b in case.bgrs], order=case.order, **case.kw)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------
def funnel(w, h, ratio, zB=Z0, name=None):
    """Two views of the plane z = 4 from one centre; the neighbour's focal length is 1/ratio of the seed view's: ratio x ratio seeds of view 0 per cell of view 1.  The first
    seed of a cell claims it and is kept, the others find it claimed and are rolled back.  Fusing view 1 afterwards has no contention (its seeds spread out in view 0)."""
    c = Case(name or "funnel%d" % ratio, [(w, h)] * 2, [Kmat(100.0, w, h), Kmat(100.0 / ratio, w, h, .3 if ratio < 64 else .01)], [plane(w, h), plane(w, h, zB)], [[1], [0]])

    def check(c, r):
        m = cell_map(c, 0, 1)
        cells = np.unique(m[m >= 0])
        assert max_population(c, 0, 1) >= min(ratio, w) * min(ratio, h) // 2, "the funnel does not funnel"
        assert r["nDepths"] == 2 * w * h
        if zB == Z0:                                                      # one point per cell of view 1 that is hit, seeded by the first pixel that hits it
            assert r["nPoints"] == len(cells) and (views_per_point(r) == 2).all()
            first = np.array([np.flatnonzero(m == k)[0] for k in cells])
            seeds = r["projs"][r["viewStart"][:-1]].astype(np.int64)
            assert np.array_equal(np.sort(seeds[:, 1] * w + seeds[:, 0]), np.sort(first))
        else:                                                             # the neighbour's plane is behind: every seed would invalidate its cell, but single-view seeds are rolled back
            assert r["nPoints"] == 0
    c.check = check
    return c


def funnel_occluded3(w, h):
    """funnel4 with the neighbour's plane at z = 6 and a third view (1 : 1) that agrees with view 0.  In view 0 the first pixel of every cell is at z = 4, in front of the
    neighbour's plane: its point survives on the third view and zeroes the cell.  The fifteen later seeds of the cell are at z = 6 and would claim it -- they find depth 0.
    Taken in reverse raster order the last seed claims the cell first and the z = 4 seed finds it claimed: order decides."""
    base = funnel(w, h, 4)
    m = cell_map(base, 0, 1)
    d0 = plane(w, h, 6.0).ravel()
    for k in np.unique(m[m >= 0]):
        d0[np.flatnonzero(m == k)[0]] = Z0
    d0 = d0.reshape(h, w)
    c = Case("funnel_occluded3", [(w, h)] * 3, [Kmat(100.0, w, h), Kmat(25.0, w, h, .3), Kmat(100.0, w, h)], [d0, plane(w, h, 6.0), d0.copy()], [[1, 2], [0, 2], [0, 1]])

    def check(c, r):
        nv = views_per_point(r)
        fwd = np.bincount(nv, minlength=4)
        bwd = np.bincount(views_per_point(reversed_case(c).fuse()), minlength=4)
        assert fwd[3] == 0 and fwd[2] >= w * h, "in raster order no seed of view 0 may reach the zeroed cell: %s" % fwd
        assert bwd[3] >= len(np.unique(m[m >= 0])) * 3 // 4, "in reverse order the last seed of a cell claims it: %s" % bwd
        assert r["nDepths"] < 3 * w * h                                    # the zeroed cells of view 1 are not counted when view 1 is fused
    c.check = check
    return c


def rollback_then_claim(w, h):
    """Three views with focal lengths 100 / 25 / 50 and nMinViewsFuse = 3.  View 2 has no depth where the first pixel of every cell of view 1 projects to, so the first seeds of a
    cell claim it, find nothing in view 2 and are rolled back; a later seed of the same cell with a depth in view 2 then claims the freed cell and is kept."""
    K = [Kmat(100.0, w, h), Kmat(25.0, w, h, .3), Kmat(50.0, w, h, .3)]
    probe = Case("probe", [(w, h)] * 3, K, [plane(w, h)] * 3, [[1, 2], [0, 2], [0, 1]])
    m1, m2 = cell_map(probe, 0, 1), cell_map(probe, 0, 2)
    d2 = plane(w, h).ravel()
    for k in np.unique(m1[m1 >= 0]):
        p = np.flatnonzero(m1 == k)[0]
        if m2[p] >= 0:
            d2[m2[p]] = 0
    d2 = d2.reshape(h, w)
    c = Case("rollback_then_claim", [(w, h)] * 3, K, [plane(w, h), plane(w, h), d2], [[1, 2], [0, 2], [0, 1]], nMinViewsFuse=3)

    def check(c, r):
        nv = views_per_point(r)
        assert r["nPoints"] > 0 and (nv == 3).all()
        m = cell_map(c, 0, 1)
        s = r["viewStart"][:-1]
        assert (r["views"][s] == 0).all() and (r["views"][s + 1] == 1).all()
        seed = r["projs"][s].astype(np.int64); seed = seed[:, 1] * w + seed[:, 0]
        cell = r["projs"][s + 1].astype(np.int64); cell = cell[:, 1] * w + cell[:, 0]
        assert np.array_equal(m[seed], cell)
        # pixels of view 0 are claimed by seeds of view 0 only (it is fused first), so every pixel before a kept seed was a seed itself; those in the same cell were rolled back
        earlier = sum(int((m[:p] == k).sum()) for p, k in zip(seed, cell))
        assert earlier > 0, "no kept point took a cell that a rolled-back seed had projected to"
    c.check = check
    return c


def across_images(w, h, order=None):
    """Three 1 : 1 views.  Left third: all agree, so view 0 claims the pixels of view 1.  Middle third: view 1 lies behind (z = 6), views 0 and 2 agree, so the kept point zeroes
    the pixel of view 1.  Right third: view 0 has no depth and view 1 seeds its own points with view 2.  With view 1 fused first (a custom order) its middle third is counted
    before it is zeroed."""
    a, b = w // 3, 2 * w // 3
    d0 = plane(w, h); d0[:, b:] = 0
    d1 = plane(w, h); d1[:, a:b] = 6.0
    c = Case("across_images" + ("" if order is None else "_" + "".join(map(str, order))), [(w, h)] * 3, [Kmat(100.0, w, h)] * 3, [d0, d1, plane(w, h)], [[1, 2], [0, 2], [0, 1]], order=order)

    def check(c, r):
        s = r["viewStart"][:-1]
        first, x = r["views"][s], r["projs"][s][:, 0]
        mid = (b - a) * h
        nv = views_per_point(r)
        # left: views 0, 1, 2; middle: 0 and 2 (view 1's pixel is zeroed, never a point); right: 1 and 2 (seeded by view 1 whatever the order)
        assert r["nPoints"] == w * h and ((nv == 3) == (x < a)).all() and ((first == 1) == (x >= b)).all() and (r["views"][s + 1][(x >= a) & (x < b)] == 2).all()
        if c.order[0] == 0:      # view 1 is fused after view 0 zeroed its middle third: those depths are not counted, and its only seeds are the right third
            assert r["nDepths"] == int((d0 != 0).sum()) + w * h - mid + w * h
            assert (first[-(w - b) * h:] == 1).all() and (first[:-(w - b) * h] == 0).all()
        else:                    # view 1 is fused first: all its depths are counted, its middle seeds are rolled back and zeroed later by view 0
            assert c.order[0] == 1 and r["nDepths"] == int((d0 != 0).sum()) + 2 * w * h
            assert (first[-mid:] == 0).all() and (nv[-mid:] == 2).all(), "the seeds of view 0 are the pixels view 1 did not claim"
    c.check = check
    return c


def seventeen(w, h, lists="asc", nMin=2, holes=True):
    """17 views, 1 : 1, all agreeing, each with the 16 others as neighbours in ascending, descending or shuffled order; view 8 is fused first, so the insertion sort of a point's
    views inserts on both sides of the seed view.  View v has no depth where (x + 3 y) % 19 == v + 1: pixels of residue 0 and 18 give points of 17 views, the others of 16."""
    n = 17
    ys, xs = np.mgrid[0:h, 0:w]
    deps = []
    for v in range(n):
        d = plane(w, h)
        if holes:
            d[(xs + 3 * ys) % 19 == v + 1] = 0
        deps.append(d)
    rng = np.random.RandomState(17)
    nbs = []
    for v in range(n):
        o = [b for b in range(n) if b != v]
        nbs.append(o if lists == "asc" else o[::-1] if lists == "desc" else list(rng.permutation(o)))
    order = [8, 16, 3, 0] + [v for v in range(n) if v not in (8, 16, 3, 0)]
    c = Case("seventeen_%s_%d%s" % (lists, nMin, "" if holes else "_full"), [(w, h)] * n, [Kmat(100.0, w, h)] * n, deps, nbs, order=order, nMinViewsFuse=nMin)

    def check(c, r):
        nv = views_per_point(r)
        assert nv.max() == 17 and (nv == 17).sum() >= w * h // 19, "no points of 17 views"
        assert nv.min() >= min(nMin, 17)
        if nMin > 16:
            assert (nv == 17).all()
        elif holes:
            assert (nv == 16).sum() > w * h // 2
        else:
            assert r["nPoints"] == w * h
        for i in np.flatnonzero(nv == 17)[:50]:
            assert np.array_equal(r["views"][r["viewStart"][i]:r["viewStart"][i + 1]], np.arange(17)), "views not strictly ascending"
        bad = [i for i in range(r["nPoints"]) if np.any(np.diff(r["views"][r["viewStart"][i]:r["viewStart"][i + 1]].astype(np.int64)) <= 0)]
        assert not bad
    c.check = check
    return c


def eighteen(w, h):
    """A view with 17 neighbours.  The reference fuses any number (its view lists are dynamic arrays) and so does the oracle; the engine holds 16 per view and refuses the
    seventeenth when the view is set (pmhip_scene_set_view: PMHIP_E_ARG) -- it never truncates the list silently."""
    n = 18
    nbs = [[b for b in range(n) if b != v][:17 if v == 0 else 16] for v in range(n)]
    c = Case("eighteen", [(w, h)] * n, [Kmat(100.0, w, h)] * n, [plane(w, h) for _ in range(n)], nbs)
    def check(c, r):
        assert r["nPoints"] == w * h and (views_per_point(r) == 18).all(), "points of 18 views expected"
    c.check = check
    return c


def _cosf(x):
    libm = C.CDLL("libm.so.6"); libm.cosf.restype = C.c_float; libm.cosf.argtypes = [C.c_float]
    return F(libm.cosf(float(x)))


def ties(w, h):
    """Pairs of scenes on the two sides of a threshold, one ulp apart: -> [(name, this side, that side)].  Each pair must give different clouds in the oracle."""
    out = []
    two = lambda name, **kw: Case(name, [(w, h)] * 2, kw.pop("K", [Kmat(100.0, w, h)] * 2), kw.pop("deps", [plane(w, h), plane(w, h)]), [[1], []], **kw)     # (view 1 is a neighbour only: the test runs one way)
    # IsDepthSimilar: |q2 - depthB| / q2 < 0.01 with q2 = 4 exactly
    th = F(0.01); dB = F(Z0 * 1.01)
    sim = lambda d: F(abs(F(Z0) - d)) / F(Z0) < th
    while sim(dB):
        dB = np.nextafter(dB, F(np.inf))
    while not sim(dB):
        dB = np.nextafter(dB, F(0))
    out.append(("depth", two("tie_depth_in", deps=[plane(w, h), plane(w, h, dB)]), two("tie_depth_out", deps=[plane(w, h), plane(w, h, np.nextafter(dB, F(np.inf)))])))
    # the normal test: dot > cos(25 deg); with the seed normal (0, 0, -1) the dot product is -nBz exactly
    ne = _cosf(F(25.0) * (F(3.14159265358979323846) / F(180)))
    def nrm(z):
        n = np.tile(F([np.sqrt(max(0.0, 1.0 - float(z) ** 2)), 0, -z]), (h, w, 1)); return [np.tile(F([0, 0, -1]), (h, w, 1)), n]
    out.append(("normal", two("tie_normal_in", nrms=nrm(np.nextafter(ne, F(1)))), two("tie_normal_out", nrms=nrm(ne))))
    # Conf2Weight: max(1 - conf, 0.03)
    cf = F(0.97)
    while F(1) - cf > F(0.03):
        cf = np.nextafter(cf, F(1))
    cn = lambda v: [np.full((h, w), v, F), np.full((h, w), 0.5, F)]
    out.append(("conf", two("tie_conf_above", cnfs=cn(np.nextafter(cf, F(0)))), two("tie_conf_clamped", cnfs=cn(cf))))
    assert F(1) - np.nextafter(cf, F(0)) > F(0.03) >= F(1) - cf
    # Round2Int at x.5 on the two borders: focal length 64 and depth 4 keep every product exact, so q0 / q2 of column j is j - cxA + cxB exactly
    cxA, cy = float(w // 2), float(h // 2)
    KA = [[64.0, 0, cxA], [0, 64.0, cy], [0, 0, 1]]
    def KB(q0_border, j):       # the principal point of view 1 that puts 4 * (the projection of column j) at q0_border
        return [[64.0, 0, (float(q0_border) - 4.0 * (j - cxA)) / 4.0], [0, 64.0, cy], [0, 0, 1]]
    qL = F(-2.0)                # column 0 at -0.5: Round2Int gives 0, inside; one ulp below gives -1
    out.append(("round_left", two("tie_left_in", K=[KA, KB(qL, 0)]), two("tie_left_out", K=[KA, KB(np.nextafter(qL, F(-np.inf)), 0)])))
    qR = F(4.0 * (w - 1) + 2.0)  # column w-1 at w - 0.5: Round2Int gives w, outside; one ulp below gives w - 1
    out.append(("round_right", two("tie_right_in", K=[KA, KB(np.nextafter(qR, F(0)), w - 1)]), two("tie_right_out", K=[KA, KB(qR, w - 1)])))
    return out


def check_tie(name, a, b, ra, rb):
    if name == "conf":
        assert ra["nPoints"] == rb["nPoints"] > 0 and not np.array_equal(ra["weights"], rb["weights"])
    elif name in ("depth", "normal"):
        assert ra["nPoints"] == a.width * a.height and rb["nPoints"] == 0
    else:                         # the border column of view 0 finds its partner in view 1 on one side of the tie only
        col = 0 if name == "round_left" else a.width - 1
        seeds = lambda r: r["projs"][r["viewStart"][:-1]][r["views"][r["viewStart"][:-1]] == 0]
        assert (seeds(ra)[:, 0] == col).sum() == a.height and (seeds(rb)[:, 0] == col).sum() == 0


def mixed_funnel(order):
    """Views of their own sizes over the same field of view: 67 x 37 (f = 100), 17 x 9 (f = 25, a quarter the size) and 84 x 46 (f = 125).  The small view is the target of a
    16 : 1 funnel when view 0 is fused first and the seed image when it is."""
    sizes = [SMALL, (17, 9), (84, 46)]
    K = [Kmat(100.0, *sizes[0]), Kmat(25.0, 17, 9, .3), Kmat(125.0, 84, 46, .3)]
    c = Case("mixed_funnel_" + "".join(map(str, order)), sizes, K, [plane(w, h) for w, h in sizes], [[1, 2], [0, 2], [0, 1]], order=order)

    def check(c, r):
        assert c.mixed and r["nPoints"] > 17 * 9 // 2 and views_per_point(r).max() == 3
        first = c.order[0]
        if first == 0:
            assert max_population(c, 0, 1) >= 12 and max_population(c, 2, 1) >= 16
        else:
            assert r["views"][r["viewStart"][0]] == 0 and (r["views"][r["viewStart"][:-1] + 1] == 1).sum() >= 17 * 9 // 2    # points seeded by the small view hold a view-0 pixel
    c.check = check
    return c


def hostile(w, h):
    """An agreeing 1 : 1 scene of three views and a fourth that looks backwards (every point is behind it: q2 <= 0), sprinkled with what a damaged .dmap can hold.  Seeds
    (view 0, fused first) and neighbour values (view 1) get depths of NaN, +-inf, negative, 1e-30 (the weight overflows: 1 / confidence = 0 and 0 * inf), 3e38 (the point
    overflows: inf and inf * 0 in the projection), a denormal; at one pixel all three views hold 1e-18, whose weights are finite and whose colour sum is not.  Confidences of 1,
    1.5, -1 and NaN; normals that are zero or NaN (neither can pass the normal test, so a kept normal of length 0 -- the nv == 0 branch -- cannot be reached from the maps).  Pixel 0 and the last pixel are among the positions.
    Expected values are the oracle's as built on x86, which tests/test_ref_fuse.py shows to be the reference's own: there a conversion of NaN or of a value outside int gives
    INT_MIN -- outside every image, 0 as a colour.  (NaNs are compared as NaN, not by sign and payload: see canon.)"""
    n = 4
    P = w * h
    bad = [np.nan, np.inf, -np.inf, -4.0, 1e-30, 3e38, 1e-45, 1e-18]
    deps = [plane(w, h) for _ in range(n)]
    cnfs = [conf_pattern(w, h, v) for v in range(n)]
    nrms = [np.tile(F([0, 0, -1]), (h, w, 1)) for _ in range(n)]
    at = lambda k: (0 if k == 0 else P - 1 if k == 1 else (k * 97 + 13) % (P - 2) + 1)
    k = 0
    for v in (0, 1):                                   # as a seed's depth and as the value a seed finds in its neighbour; the first and the last pixel get NaN and inf
        for b in bad:
            deps[v].ravel()[at(k)] = b; k += 1
    for b in (1e-30, 1e-18, np.nan, 3e38):             # in all three views at once: the seed claims its neighbours and the point is kept
        p = at(k); k += 1
        for v in range(3):
            deps[v].ravel()[p] = b
    for v in (0, 1):
        for b in (1.0, 1.5, -1.0, np.nan):
            cnfs[v].ravel()[at(k)] = b; k += 1
    for v in (0, 1):
        for b in (0.0, np.nan):
            nrms[v].reshape(-1, 3)[at(k)] = b; k += 1
    p = at(k); k += 1
    for v in range(3):
        nrms[v].reshape(-1, 3)[p] = 0.0                # every view's normal is zero
    R = [np.eye(3)] * 3 + [np.diag([-1.0, 1.0, -1.0])]
    nbs = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    c = Case("hostile", [(w, h)] * n, [Kmat(100.0, w, h)] * n, deps, nbs, R=R, nrms=nrms, cnfs=cnfs)

    def check(c, r):
        assert len({at(i) for i in range(k)}) == k, "two hostile values share a pixel"
        assert np.isnan(deps[0].ravel()[0]) and np.isinf(deps[0].ravel()[P - 1])
        assert r["nPoints"] > P * 9 // 10 and views_per_point(r).max() == 3 and not (r["views"] == 3).any()     # nothing ever joins the view that looks away
        assert np.isnan(r["points"]).any() and np.isinf(r["weights"]).any(), "no overflowing weight was kept"
        assert r["nDepths"] > 3 * P
    c.check = check
    return c


def compaction(w, h):
    """Two 1 : 1 views; view 0 has depths only where a point is to be kept, so the records of view 0 are exactly the chosen pixels and those of view 1 are empty: no kept
    point at all, only pixel 0, only the last pixel (in the last, partial tile), one on each side of the first tile border (1023 and 1024), every pixel."""
    P = w * h
    sets = [("empty", []), ("first", [0]), ("last", [P - 1]), ("all", range(P))] + ([("tile_border", [1023, 1024])] if P > 1024 else [])
    out = []
    for name, keep in sets:
        keep = np.array(list(keep), np.int64)
        d0 = np.zeros(P, F); d0[keep] = Z0
        c = Case("compaction_" + name, [(w, h)] * 2, [Kmat(100.0, w, h)] * 2, [d0.reshape(h, w), plane(w, h)], [[1], [0]], order=[0, 1])

        def check(c, r, keep=keep):
            s = r["projs"][r["viewStart"][:-1]].astype(np.int64)
            assert r["nPoints"] == len(keep) and np.array_equal(s[:, 1] * w + s[:, 0], keep) and r["nDepths"] == len(keep) + P
        c.check = check
        out.append(c)
    return out


def uniform_cases(w, h):
    """Every uniform-size case at w x h."""
    cs = [funnel(w, h, 4), funnel(w, h, 64), funnel(w, h, 4, zB=6.0, name="funnel_occluded"), funnel_occluded3(w, h), rollback_then_claim(w, h),
          across_images(w, h), across_images(w, h, order=[1, 0, 2])]
    cs += [seventeen(w, h, l, m) for l in ("asc", "desc", "shuffled") for m in (2, 17, 40)] + [seventeen(w, h, "shuffled", 2, holes=False)]
    for _, a, b in ties(w, h):
        cs += [a, b]
    return cs + [hostile(w, h)] + compaction(w, h)


def mixed_cases():
    return [mixed_funnel([0, 1, 2]), mixed_funnel([1, 0, 2])]


def all_cases(sizes=(SMALL,) + THIN):
    return {"%s@%dx%d" % (c.name, w, h): c for w, h in sizes for c in uniform_cases(w, h)} | {c.name: c for c in mixed_cases()}


# ---- the host emulation of the device algorithm (tests/cpp/fuse_emul.cpp) -----------------------------------------------------------------------------------------
def emulator(src=None, tag=""):
    src = src or os.path.join(HERE, "cpp", "fuse_emul.cpp")
    out = os.path.join(HERE, "cpp", "build", "libfuse_emul%s.so" % tag)
    hdr = os.path.join(HERE, "..", "openmvs_amd", "csrc", "pm_fuse.h")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(out):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out, src])
    lib = C.CDLL(out)
    lib.emu_fuse_depth_maps.restype = C.c_int
    return lib


def emulate(lib, case, mode):
    """-> (cloud, rounds, seeds) of the emulator under thread order `mode` (0 ascending, 1 descending, 2 random in every phase)."""
    old = os.environ.get("EMU_FUSE_ORDER")
    os.environ["EMU_FUSE_ORDER"] = str(mode)
    try:
        r = case.fuse(fn=lib.emu_fuse_depth_maps)
    finally:
        if old is None:
            del os.environ["EMU_FUSE_ORDER"]
        else:
            os.environ["EMU_FUSE_ORDER"] = old
    rounds, seeds = C.c_uint64(), C.c_uint64()
    lib.emu_fuse_stats(C.byref(rounds), C.byref(seeds))
    return r, int(rounds.value), int(seeds.value)
