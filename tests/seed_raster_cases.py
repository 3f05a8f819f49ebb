"""The cases of the seed rasteriser (csrc/seed_raster.hip, include/pmhip_seed.h), shared by tests/test_emu_seed_raster.py (the wave64 emulator, CPU suite) and
tests/test_zz_gpu_seed_raster.py (the device).  Every comparison is on uint32 views, bit for bit.  The expectation is the literal sequential walk -- `views._raster_face`
over the faces in the order given (a later face overwrites), or the 2x2 loop over the vertices -- and, where oracle/_ref is built, `pyref.ref_raster_faces`, the
reference's own compiled rasteriser.  Expectations are computed once per case and shared (read only)."""
import functools
import os

import numpy as np

from openmvs_amd import densify, optdense, views
from openmvs_amd.patchmatch import SEED_FACES, SEED_POINTS
from oracle import pyref

f32 = np.float32
INT_MAX = 0x7FFFFFFF
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %s: %r != %r" % (what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


class Case:
    def __init__(self, name, w, h, proj, z, normals, faces, mode=SEED_FACES):
        self.name, self.w, self.h, self.mode = name, int(w), int(h), mode
        self.proj = np.ascontiguousarray(proj, f32).reshape(-1, 2); self.z = np.ascontiguousarray(z, f32).ravel()
        self.normals = np.ascontiguousarray(normals, f32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        self._want = None

    def want(self):
        """(depth, normal) of the sequential walk; cross-checked once against the reference's compiled rasteriser where it is built."""
        if self._want is None:
            self._want = walk_faces(self) if self.mode == SEED_FACES else walk_points(self)
            if self.mode == SEED_FACES and pyref.fuse_available():
                rd, rn = pyref.ref_raster_faces(self.w, self.h, self.proj, self.z, self.normals, self.faces)
                same_bits(self._want[0], rd, self.name + ": the walk against ref_raster_faces, depth"); same_bits(self._want[1], rn, self.name + ": the walk against ref_raster_faces, normals")
        return self._want


def walk_faces(c, faces=None):
    d = np.zeros((c.h, c.w), f32); n = np.zeros((c.h, c.w, 3), f32)
    with np.errstate(all="ignore"):
        for fa in (c.faces if faces is None else faces):
            views._raster_face(c.proj[fa], c.z[fa], c.normals[fa], d, n)
    return d, n


def walk_points(c):
    d = np.zeros((c.h, c.w), f32); n = np.zeros((c.h, c.w, 3), f32)
    for (x, y), zz, nn in zip(np.floor(c.proj).astype(np.int64), c.z, c.normals):
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            if 0 <= x + dx < c.w and 0 <= y + dy < c.h:
                d[y + dy, x + dx] = zz; n[y + dy, x + dx] = nn
    return d, n


def coverage(c):
    """How many faces cover each pixel, from the host walk of every face on its own."""
    cnt = np.zeros((c.h, c.w), np.int64)
    for fa in c.faces:
        d = np.zeros((c.h, c.w), f32)
        views._raster_face(c.proj[fa], c.z[fa], None, d, None)
        cnt += d > 0
    return cnt


def run_case(engine, c):
    """With normals and depth only: the same depths, and both equal the walk."""
    wd, wn = c.want()
    d, n = engine.seed_raster(c.mode, c.w, c.h, c.proj, c.z, c.normals, c.faces)
    same_bits(d, wd, c.name + ": depth"); same_bits(n, wn, c.name + ": normals")
    d2, n2 = engine.seed_raster(c.mode, c.w, c.h, c.proj, c.z, None, c.faces)
    assert n2 is None
    same_bits(d2, wd, c.name + ": depth only")
    return d, n


def front_facing(proj, tri):
    """Wound front-facing for EdgeFunction (back faces are culled), as tests/test_ref_fuse.py does."""
    out = []
    for f in np.asarray(tri, np.uint32):
        a, b, c = proj[f].astype(np.float64)
        out.append(f if (c[0] - a[0]) * (b[1] - a[1]) - (c[1] - a[1]) * (b[0] - a[0]) > 0 else f[[0, 2, 1]])
    return np.array(out, np.uint32).reshape(-1, 3)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


# ---- FACES: seeded random Delaunay meshes overhanging the image ------------------------------------------------------------------------------------------
def delaunay_case(w, h, nv, seed):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    proj = (rng.random((nv, 2)) * [w + 10, h + 10] - 5).astype(f32)
    z = (rng.random(nv) * 3 + 2).astype(f32)
    tri = Delaunay(proj.astype(np.float64)).simplices if nv > 3 else np.array([[0, 1, 2]])
    return Case("delaunay_%dx%d_%dv" % (w, h, nv), w, h, proj, z, unit_normals(rng, nv), front_facing(proj, tri))


DELAUNAY_CASES = [delaunay_case(w, h, nv, 100 * w + nv) for w, h in ((1, 1), (2, 2), (7, 5), (64, 48), (131, 67)) for nv in (3, 4, 30, 400)]
DELAUNAY_IDS = [c.name for c in DELAUNAY_CASES]


# ---- FACES: an integer grid, cells split along diagonals that alternate from row to row --------------------------------------------------------------------
def grid_mesh(nx=5, ny=5, step=3, soup=False):
    """Vertices on pixel centres.  Shared vertices, or (`soup`) every face with vertices of its own at one depth per face, so that the depth map names the winner."""
    w, h = (nx - 1) * step + 1, (ny - 1) * step + 1
    rng = np.random.default_rng(7)
    P = np.array([(i * step, j * step) for j in range(ny) for i in range(nx)], f32)
    Z = (rng.random(len(P)) * 2 + 3).astype(f32)
    N = unit_normals(rng, len(P))
    tri = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            tri += [(a, b, d), (a, d, c)] if j % 2 == 0 else [(a, b, c), (b, d, c)]
    F = front_facing(P, tri)
    if not soup:
        return Case("grid", w, h, P, Z, N, F)
    P2 = P[F.ravel()]; Z2 = np.repeat((2 + 0.125 * np.arange(len(F))).astype(f32), 3); N2 = N[F.ravel()]
    return Case("grid_soup", w, h, P2, Z2, N2, np.arange(3 * len(F), dtype=np.uint32).reshape(-1, 3))


def grid_case(engine):
    for soup in (False, True):
        c = grid_mesh(soup=soup)
        cnt = coverage(c)
        assert (cnt == 2).any() and (cnt >= 6).any() and (cnt == 1).any() and cnt.min() >= 1, "edge pixels under 2 faces, interior vertex pixels under 6 or more"
        run_case(engine, c)
        rng = np.random.default_rng(11)
        maps = {}
        for name, order in (("given", np.arange(len(c.faces))), ("reversed", np.arange(len(c.faces))[::-1]), ("shuffled", rng.permutation(len(c.faces)))):
            o = Case(c.name + "_" + name, c.w, c.h, c.proj, c.z, c.normals, c.faces[order])
            maps[name] = run_case(engine, o)[0]
        if soup:                                                                 # one depth per face: the map names the winner, and the winner follows the order
            assert (bits(maps["given"]) != bits(maps["reversed"])).any() and (bits(maps["given"]) != bits(maps["shuffled"])).any()
            assert ((bits(maps["given"]) != bits(maps["reversed"])) <= (cnt >= 2)).all()


# ---- FACES: the box rules on their boundaries -----------------------------------------------------------------------------------------------------------------
def box_rule_cases():
    w, h = 9, 7
    up = lambda v: np.nextafter(f32(v), f32(np.inf)); dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    tris = {
        "vertex_at_w_minus_1": [(w - 1, 1), (w - 1, 5), (4, 3)],
        "all_x_at_w_minus_1_or_beyond": [(w - 1, 1), (w + 3, 3), (w - 1, 5)],
        "min_x_one_ulp_beyond_w_minus_1": [(up(w - 1), 1), (w + 3, 3), (up(w - 1), 5)],
        "max_x_minus_zero": [(-0.0, 1), (-4, 3), (-0.0, 5)],
        "max_x_one_ulp_below_zero": [(dn(0), 1), (-4, 3), (dn(0), 5)],
        "max_y_minus_zero": [(1, -0.0), (5, -0.0), (3, -4)],
        "max_y_one_ulp_below_zero": [(1, dn(0)), (5, dn(0)), (3, -4)],
        "min_y_at_h_minus_1": [(1, h - 1), (3, h + 3), (5, h - 1)],
        "min_y_one_ulp_beyond_h_minus_1": [(1, up(h - 1)), (3, h + 3), (5, up(h - 1))],
        "outside_left": [(-9, 1), (-3, 1), (-6, 5)], "outside_right": [(w + 2, 1), (w + 8, 1), (w + 5, 5)],
        "outside_above": [(1, -9), (5, -9), (3, -3)], "outside_below": [(1, h + 2), (5, h + 2), (3, h + 8)],
        "box_of_one_pixel": [(0, 0), (-0.9, 0), (0, -0.9)],
        "box_of_one_pixel_inside": [(4, 3), (4, 3), (4, 3)],                     # (a point: area 0, nothing drawn)
        "whole_image_and_more": [(-20, -20), (40, -20), (-20, 40)],
    }
    out = []
    rng = np.random.default_rng(3)
    for name, t in tris.items():
        P = np.array(t, f32)
        out.append(Case("box_" + name, w, h, P, [2.5, 3.0, 4.0], unit_normals(rng, 3), front_facing(P, [[0, 1, 2]])))
    return out


BOX_CASES = box_rule_cases()
BOX_IDS = [c.name for c in BOX_CASES]
BOX_DRAWS = {"box_vertex_at_w_minus_1": True, "box_all_x_at_w_minus_1_or_beyond": True, "box_min_x_one_ulp_beyond_w_minus_1": False, "box_max_x_minus_zero": True,
             "box_max_x_one_ulp_below_zero": False, "box_max_y_minus_zero": True, "box_max_y_one_ulp_below_zero": False, "box_min_y_at_h_minus_1": True,
             "box_min_y_one_ulp_beyond_h_minus_1": False, "box_outside_left": False, "box_outside_right": False, "box_outside_above": False, "box_outside_below": False,
             "box_box_of_one_pixel": True, "box_box_of_one_pixel_inside": False, "box_whole_image_and_more": True}


def box_case(engine, c):
    d, _ = run_case(engine, c)
    assert bool(d.any()) == BOX_DRAWS[c.name], c.name
    if c.name == "box_box_of_one_pixel":
        assert (d > 0).sum() == 1 and d[0, 0] > 0
    if c.name == "box_whole_image_and_more":
        assert (d > 0).all()


def culled_case(engine):
    """Back-facing and collinear faces are skipped; a mesh with every winding reversed gives all-zero maps."""
    c = next(k for k in DELAUNAY_CASES if k.name == "delaunay_64x48_30v")
    back = Case(c.name + "_reversed_winding", c.w, c.h, c.proj, c.z, c.normals, c.faces[:, [0, 2, 1]])
    d, n = run_case(engine, back)
    assert not d.any() and not n.any() and c.want()[0].any()
    P = np.array([(1, 1), (4, 2.5), (7, 4), (1, 5)], f32)                        # 0, 1, 2 collinear; (0, 2, 3) and its reverse
    col = Case("collinear_and_back", 9, 7, P, [2, 3, 4, 5], unit_normals(np.random.default_rng(5), 4), [[0, 1, 2], [2, 1, 0], [0, 2, 3], [0, 3, 2]])
    d, _ = run_case(engine, col)
    only = Case("the_one_front_face", 9, 7, P, col.z, col.normals, front_facing(P, [[0, 2, 3]]))
    same_bits(d, only.want()[0], "only the front-facing, non-degenerate face is drawn"); assert d.any()


# ---- FACES: the two routes -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corners_case():
    """Four faces through the image corners that cover everything (as bAddCorners leaves them), plus 400 tiny faces."""
    w, h = 96, 64
    rng = np.random.default_rng(21)
    P = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (40.3, 30.6)]
    tri = [(0, 1, 4), (1, 3, 4), (3, 2, 4), (2, 0, 4)]
    for _ in range(400):
        x, y = rng.random(2) * [w + 4, h + 4] - 2
        k = len(P)
        P += [(x, y), (x + rng.random() * 3 + 0.2, y + rng.random()), (x + rng.random(), y + rng.random() * 3 + 0.2)]
        tri.append((k, k + 1, k + 2))
    P = np.array(P, f32)
    return Case("corners_and_400_tiny", w, h, P, (rng.random(len(P)) * 3 + 2).astype(f32), unit_normals(rng, len(P)), front_facing(P, tri))


def routes_case(engine):
    c = corners_case()
    default = engine.seed_stats()["box_pixels"]
    assert default == 64
    try:
        got = {}
        for box in (1, -1, INT_MAX):
            engine.seed_set_tuning(box)
            got[box] = run_case(engine, c)
            st = engine.seed_stats()
            assert st["box_pixels"] == (default if box < 0 else box)
            drawn = len(c.faces)                                                 # (every face of this case is front-facing and touches the image or lies just outside)
            assert (st["large_faces"] == 0) if box == INT_MAX else (4 <= st["large_faces"] <= drawn), st
            if box == 1:
                assert st["large_faces"] > 300                                   # every drawn face has a box of more than one pixel
        assert (got[1][0] > 0).all()
        engine.seed_set_tuning(0)
        assert engine.seed_stats()["box_pixels"] == INT_MAX                      # 0 keeps the value
        # one face whose clipped box holds exactly boxPixels, boxPixels - 1 and boxPixels + 1 pixels (default 64): 8 x 8, 9 x 7, 13 x 5
        engine.seed_set_tuning(-1)
        for (bw, bh), large in (((8, 8), 0), ((9, 7), 0), ((13, 5), 1)):
            P = np.array([(2, 3), (2 + bw - 1, 3), (2, 3 + bh - 1)], f32)
            one = Case("box_%dx%d" % (bw, bh), 20, 16, P, [2, 3, 4], unit_normals(np.random.default_rng(1), 3), front_facing(P, [[0, 1, 2]]))
            d, _ = run_case(engine, one)
            assert d.any() and engine.seed_stats()["large_faces"] == large, (bw, bh, engine.seed_stats())
    finally:
        engine.seed_set_tuning(-1)


def zero_normal_case(engine):
    """Vertex normals that sum to zero at a pixel give a zero normal there (cv::normalize of a zero vector), not a NaN."""
    P = np.array([(2, 1), (10, 1), (6, 9)], f32)
    c = Case("normals_cancel", 13, 11, P, [3, 3, 3], [(1, 0, 0), (-1, 0, 0), (0, 0, 0)], front_facing(P, [[0, 1, 2]]))
    d, n = run_case(engine, c)
    assert (d[:, 6] > 0).sum() >= 5 and not n[:, 6][d[:, 6] > 0].any() and n[d > 0].any()    # the median x = 6: pb0 == pb1
    z = Case("normals_all_zero", 13, 11, P, [3, 4, 5], np.zeros((3, 3), f32), c.faces)
    d, n = run_case(engine, z)
    assert d.any() and not n.any() and not np.isnan(n).any()


# ---- POINTS ----------------------------------------------------------------------------------------------------------------------------------------------------
def points_cases():
    w, h = 9, 7
    rng = np.random.default_rng(9)
    mk = lambda name, P, ww=w, hh=h: Case("points_" + name, ww, hh, np.array(P, f32), (np.arange(len(P)) + 2).astype(f32), unit_normals(rng, len(P)), np.zeros((0, 3)), SEED_POINTS)
    out = [mk("same_pixel", [(3.2, 2.7), (3.9, 2.1)]),
           mk("overlapping_blocks", [(3.5, 2.5), (4.5, 3.5), (4.2, 2.9), (3.1, 3.3)]),
           mk("floor_minus_1", [(-0.5, 2.5), (3.5, -0.25), (-0.5, -0.5)]),
           mk("floor_w_minus_1", [(w - 1, 2.0), (2.0, h - 1), (w - 0.5, h - 0.5)]),
           mk("outside", [(-1.5, 2), (w, 2), (2, -1.01), (2, h), (-300.0, 1e6)]),
           mk("one_pixel_image", [(-1, -1), (0, 0), (-0.5, 0.5)], 1, 1),
           mk("minus_zero", [(-0.0, -0.0)])]
    P = rng.random((700, 2)) * [w * 4 + 6, h * 4 + 6] - 3
    out.append(mk("700_random", P, w * 4, h * 4))
    return out


POINTS_CASES = points_cases()
POINTS_IDS = [c.name for c in POINTS_CASES]


def points_case(engine, c):
    d, n = run_case(engine, c)
    if c.name == "points_same_pixel":
        assert d[2, 3] == 3 and d[3, 4] == 3 and (d > 0).sum() == 4              # the later index wins
    if c.name == "points_floor_minus_1":
        assert d[2, 0] == 2 and d[3, 0] == 2 and d[0, 3] == 3 and d[0, 4] == 3 and d[0, 0] == 4 and (d > 0).sum() == 5
    if c.name == "points_floor_w_minus_1":
        assert d[2, 8] == 2 and d[3, 8] == 2 and d[6, 2] == 3 and d[6, 3] == 3 and d[6, 8] == 4 and (d > 0).sum() == 5
    if c.name == "points_outside":
        assert not d.any() and not n.any()
    if c.name == "points_overlapping_blocks":
        assert d[3, 4] == 5 and d[3, 5] == 4 and d[4, 4] == 5 and d[4, 5] == 3


def empty_case(engine):
    """No vertex, or no face in FACES mode: all-zero maps and no error."""
    z3 = np.zeros((0, 3), f32)
    for mode in (SEED_POINTS, SEED_FACES):
        d, n = engine.seed_raster(mode, 5, 4, np.zeros((0, 2), f32), np.zeros(0, f32), z3, None)
        assert d.shape == (4, 5) and not d.any() and n.shape == (4, 5, 3) and not n.any()
    d, n = engine.seed_raster(SEED_FACES, 5, 4, [(1, 1), (3, 1), (1, 3)], [2, 2, 2], np.ones((3, 3), f32), None)
    assert not d.any() and not n.any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def refusal_cases(engine, Error):
    """Every refusal of include/pmhip_seed.h, each followed by a call that succeeds on the same engine."""
    import pytest
    c = next(k for k in DELAUNAY_CASES if k.name == "delaunay_7x5_30v")
    ok = lambda: run_case(engine, c)
    ok()

    def bad(match, mode=SEED_FACES, w=c.w, h=c.h, proj=c.proj, z=c.z, faces=c.faces):
        for m in ([mode] if mode is not None else [SEED_FACES, SEED_POINTS]):
            with pytest.raises(Error, match=match):
                engine.seed_raster(m, w, h, proj, z, c.normals, faces)
        ok()
    edit = lambda a, i, v: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    bad("not finite", None, proj=edit(c.proj, (4, 0), np.nan))
    bad("not finite", None, proj=edit(c.proj, (4, 1), np.inf))
    bad("not finite", None, proj=edit(c.proj, (29, 0), -np.inf))
    bad("not finite", None, z=edit(c.z, 7, np.nan))
    bad("not finite", None, z=edit(c.z, 7, np.inf))
    bad("vertex 7 has depth", None, z=edit(c.z, 7, 0.0))
    bad("vertex 7 has depth", None, z=edit(c.z, 7, -1.5))
    bad("outside the range of int", None, proj=edit(c.proj, (2, 0), 2147483648.0))
    bad("outside the range of int", None, proj=edit(c.proj, (2, 1), -2147483904.0))
    bad("face 3 names vertex 30 of 30", faces=edit(c.faces, (3, 1), 30))
    bad("a map of 0 x 5", None, w=0)
    bad("a map of 7 x 0", None, h=0)
    bad("a map of -2 x 5", None, w=-2)
    bad("more than INT_MAX pixels", None, w=65536, h=32768)
    bad("neither points", mode=2)
    # a NULL array with a non-zero count, through the C ABI itself
    lib, h_ = engine._lib, engine._h
    d = np.zeros((c.h, c.w), f32)
    assert lib.pmhip_seed_raster(h_, SEED_FACES, c.w, c.h, None, c.z, None, len(c.z), c.faces, len(c.faces), d, None) == -1 and b"no projections or depths" in lib.pmhip_last_error(h_)
    assert lib.pmhip_seed_raster(h_, SEED_FACES, c.w, c.h, c.proj, None, None, len(c.z), c.faces, len(c.faces), d, None) == -1
    assert lib.pmhip_seed_raster(h_, SEED_FACES, c.w, c.h, c.proj, c.z, None, len(c.z), None, len(c.faces), d, None) == -1 and b"no indices" in lib.pmhip_last_error(h_)
    assert lib.pmhip_seed_raster(h_, SEED_FACES, c.w, c.h, c.proj, c.z, None, len(c.z), c.faces, len(c.faces), None, None) == -1 and b"no depth map" in lib.pmhip_last_error(h_)
    assert not d.any(), "nothing was written"
    ok()
    # the largest coordinates that are taken: the floors and ceils still fit an int
    far = Case("far", 5, 4, [(2147483520.0, 1), (-2147483648.0, 1), (2, 2147483520.0)], [2, 2, 2], np.ones((3, 3), f32), [[0, 1, 2], [0, 2, 1]])
    for mode in (SEED_FACES, SEED_POINTS):
        engine.seed_raster(mode, far.w, far.h, far.proj, far.z, far.normals, far.faces)


# ---- the scene route ---------------------------------------------------------------------------------------------------------------------------------------------
def scene_view_case(engine):
    """`scene_seed_view` + `scene_get_maps` against `scene_set_maps` with the host maps + `scene_get_maps`: a view of the scene's size and one of its own size, both
    modes, with and without normals (without: the resident normal map stays, as with a NULL normal map)."""
    from openmvs_amd import synth
    sc = synth.make_scene(3, 40, 32, n_src=2)
    engine.scene_load(sc, n_levels=0)
    own = np.zeros((23, 31), f32)                                                # view 2 carries its own size, 31 x 23
    engine.scene_set_view_sized(2, own, sc.K[2], sc.R[2], sc.C[2], float(sc.dmin[2]), float(sc.dmax[2]), sc.neighbors[2])
    rng = np.random.default_rng(4)
    for view, (w, h) in ((0, (40, 32)), (2, (31, 23))):
        assert engine.view_size(view) == (w, h)
        base = delaunay_case(w, h, 60, 77 + view)
        for mode in (SEED_FACES, SEED_POINTS):
            c = Case("%s_view%d_mode%d" % (base.name, view, mode), w, h, base.proj, base.z, base.normals, base.faces, mode)
            wd, wn = c.want()
            marker = rng.random((h, w, 3)).astype(f32)
            for with_normals in (True, False):
                engine.scene_set_maps(view, np.full((h, w), 9, f32), marker)
                engine.scene_seed_view(view, mode, c.proj, c.z, c.normals if with_normals else None, c.faces)
                got = engine.scene_get_maps(view)
                engine.scene_set_maps(view, np.full((h, w), 9, f32), marker)
                engine.scene_set_maps(view, wd, wn if with_normals else None)
                want = engine.scene_get_maps(view)
                for g, x, what in zip(got, want, ("depth", "normal", "confidence")):
                    same_bits(g, x, "%s, normals %s: %s" % (c.name, with_normals, what))
                same_bits(got[0], wd, c.name); same_bits(got[1], wn if with_normals else marker, c.name + ": normal map")
    import pytest
    from openmvs_amd.patchmatch import PatchMatchError
    with pytest.raises(PatchMatchError, match="view 3 of 3"):
        engine.scene_seed_view(3, SEED_POINTS, base.proj, base.z, None, None)
    with pytest.raises(PatchMatchError, match="not finite"):
        engine.scene_seed_view(0, SEED_POINTS, np.full((1, 2), np.nan, f32), [1.0], None, None)
    same_bits(engine.scene_get_maps(2)[0], want[0], "a refused call writes nothing")


def _opt(level, min_resolution, sparse):
    opt = optdense.defaults()
    opt.nResolutionLevel = level; opt.nMinResolution = min_resolution; opt.nNumViews = 3; opt.nEstimateNormals = 2; opt.nSpeckleSize = 20
    opt.bInitSparse = 1 if sparse else 0
    return opt


@functools.lru_cache(maxsize=None)
def host_scene(level, min_resolution, sparse):
    """The host route's SceneViews (the Python face walk at full working resolution for bInitSparse = 0), computed once and shared (read only)."""
    return densify.load_scene(SCENE, opt=_opt(level, min_resolution, sparse))


def scene_routes_agree(new_engine, level, min_resolution, size, sparse, light=False):
    """`load_scene` + `compute_depth_maps` with `seed_on_device` off and on: no init maps are made, the meshes rasterise to the host route's init maps, and the
    estimated depth, normal and confidence maps are the same bits.  `light` (the emulator): no sub-resolution level, one sweep, no geometric round."""
    host = host_scene(level, min_resolution, sparse)
    assert (host.width, host.height) == size and not host.seed_mesh and len(host.ids) >= 3
    opt = _opt(level, min_resolution, sparse)
    dev = densify.load_scene(SCENE, opt=opt, seed_on_device=True)
    assert not dev.init_depth and not dev.init_normal and sorted(dev.seed_mesh) == dev.ids == host.ids
    assert dev.dmin == host.dmin and dev.dmax == host.dmax
    opt.nSubResolutionLevels = 0 if light else 1; opt.nEstimationGeometricIters = 0 if light else 1; opt.nEstimationIters = 1 if light else 2
    maps = {}
    for name, sv in (("device", dev), ("host", host)):
        e = new_engine()
        try:
            e.scene_load(sv, n_levels=int(opt.nSubResolutionLevels))
            if name == "device":
                for v in sv.ids:                                                 # the seed itself: what scene_set_maps would have uploaded
                    mode, proj, z, normals, faces = sv.seed_mesh[v]
                    assert mode == (SEED_POINTS if sparse else SEED_FACES) and len(z) > 100
                    e.scene_seed_view(v, mode, proj, z, normals, faces)
                    d, n, _ = e.scene_get_maps(v)
                    same_bits(d, host.init_depth[v], "seed depth of view %d" % v); same_bits(n, host.init_normal[v], "seed normals of view %d" % v)
                    assert (d > 0).mean() > (0.001 if sparse else 0.3)
            densify.compute_depth_maps(e, sv.ids, opt.params(3), n_optimize=0, init_depth=sv.init_depth, init_normal=sv.init_normal, scene=sv, seed_mesh=sv.seed_mesh)
            maps[name] = {v: e.scene_get_maps(v) for v in sv.ids}
        finally:
            e.close()
    for v in host.ids:
        for g, x, what in zip(maps["device"][v], maps["host"][v], ("depth", "normal", "confidence")):
            same_bits(g, x, "view %d: %s" % (v, what))
        assert (maps["host"][v][0] > 0).mean() > 0.3


def dense_reconstruction_routes_agree(new_engine, tmp_path, level, min_resolution, light=False):
    """`dense_reconstruction` with the same seed by both routes: the archives are the same bytes."""
    out = {}
    for on in (False, True):
        opt = _opt(level, min_resolution, True)
        if light:
            opt.nSubResolutionLevels = 0; opt.nEstimationIters = 1; opt.nEstimationGeometricIters = 0
        e = new_engine()
        try:
            out[on] = str(tmp_path / ("device.mvs" if on else "host.mvs"))
            sv, cloud = densify.dense_reconstruction(e, SCENE, out[on], opt, seed=3, seed_on_device=on)
            assert bool(sv.seed_mesh) == on and bool(sv.init_depth) != on
            if on:
                assert e.seed_stats()["mesh_bytes"] > 0
        finally:
            e.close()
    with open(out[True], "rb") as a, open(out[False], "rb") as b:
        assert a.read() == b.read()


def full_hd_case(engine):
    """The device only: the test scene's points of image 0 scaled to 1920 x 1080, FACES, against the reference's compiled rasteriser."""
    from openmvs_amd import mvsi
    w, h = 1920, 1080
    sc = mvsi.load(SCENE)
    cams = views.Cameras(sc, [(w, h)] * len(sc.images))
    sel = views.select_views(sc, cams, 0, views.DenseOptions())
    proj, z, vz, normals, faces, _, _ = views.point_mesh(sc, cams, 0, sel[1], views.DenseOptions())
    assert len(z) > 1000 and len(faces) > 2000
    rd, rn = pyref.ref_raster_faces(w, h, proj, vz, normals, faces.astype(np.uint32))
    d, n = engine.seed_raster(SEED_FACES, w, h, proj, vz, normals, faces)
    assert (rd > 0).mean() > 0.3
    same_bits(d, rd, "1920 x 1080: depth"); same_bits(n, rn, "1920 x 1080: normals")
    assert engine.seed_stats()["large_faces"] > 1000
