"""CPU tests of pmhip_scene_cloud_finish (csrc/pm_cloud.hip) under the wave64 emulator: the ROI crop against a literal RFOREACH + RemoveAt
loop, EstimatePointColors bit for bit, the k-nearest-neighbour sets against cKDTree, the PCA normals against numpy, and the Python driver."""
import os

import numpy as np
import pytest

from openmvs_amd import patchmatch, synth
from tests import cloud_cases as cc
from tests import emu

F = np.float32


@pytest.fixture(scope="module")
def lib():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as path:
        yield path


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(5, 160, 120, n_src=4)


def _engine(sc, colors=True):
    e = patchmatch.PatchMatchHIP(0)
    e.scene_load(sc, n_levels=0)
    if colors:
        for v in range(sc.n_views):
            e.scene_set_color(v, sc.bgr[v])
    return e


def _same(got, want, what):
    assert got["nPoints"] == want["nPoints"], what
    for k in ("points", "viewStart", "views", "weights", "projs", "colors", "normals"):
        if want.get(k) is None:
            assert got.get(k) is None, (what, k)
            continue
        assert np.array_equal(got[k], want[k]), (what, k)


def _obb(sc, pts, shrink, angle=0.3):
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F)
    pos = np.median(pts, axis=0).astype(F)
    local = (pts - pos) @ rot.T
    ext = (np.abs(local).max(axis=0) * shrink).astype(F)
    return rot, pos, ext


# ---- crop --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border,shrink", [(0.0, 0.6), (1.2, 0.5), (-0.05, 0.5), (0.0, 1e-6), (0.0, 2.0)])
def test_crop_matches_swap_remove_order(lib, scene, border, shrink):
    sc = scene
    e = _engine(sc)
    cl = cc.random_cloud(sc, 20000, seed=3)
    # a cloud with colours and normals already made: fuse them through set + finish, then crop
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"], cl["weights"])
    full = e.scene_cloud_finish(estimate_colors=True, estimate_normals=True)
    rot, pos, ext = _obb(sc, cl["points"], shrink)
    r2, p2, e2 = cc.obb_enlarged(rot, pos, ext, border)
    inside = cc.obb_inside(full["points"], r2, p2, e2)
    want = cc.crop_reference(full, inside)
    got = e.scene_cloud_finish(crop_obb=(rot, pos, ext), border_roi=border)
    _same(got, want, "crop border=%g shrink=%g" % (border, shrink))
    if shrink <= 1e-6:
        assert got["nPoints"] <= 1
    if shrink >= 2.0 and border == 0:
        assert got["nPoints"] == full["nPoints"]
    assert 0 <= got["nPoints"] <= full["nPoints"]
    e.close()


def test_crop_then_estimates_see_the_permuted_order(lib, scene):
    sc = scene
    e = _engine(sc)
    cl = cc.random_cloud(sc, 6000, seed=4)
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"], cl["weights"])
    rot, pos, ext = _obb(sc, cl["points"], 0.5)
    got = e.scene_cloud_finish(crop_obb=(rot, pos, ext), estimate_colors=True, estimate_normals=True)
    want = cc.crop_reference(dict(cl, projs=np.zeros((len(cl["views"]), 2), np.uint16)), cc.obb_inside(cl["points"], rot, pos, ext))
    for k in ("points", "viewStart", "views", "weights"):
        assert np.array_equal(got[k], want[k]), k
    Ps = [cc.compose_P(sc.K[i], sc.R[i], sc.C[i]) for i in range(sc.n_views)]
    assert np.array_equal(got["colors"], cc.colors_reference(want, Ps, list(sc.bgr)))
    e.close()


# ---- colours ----------------------------------------------------------------------------------------------------------------------------
def test_colors_bit_exact(lib, scene):
    sc = scene
    e = _engine(sc)
    cl = cc.random_cloud(sc, 30000, seed=5, max_views=5)
    # points near the image borders (white) and duplicated view depths (first view wins)
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"], cl["weights"])
    got = e.scene_cloud_finish(estimate_colors=True)
    Ps = [cc.compose_P(sc.K[i], sc.R[i], sc.C[i]) for i in range(sc.n_views)]
    want = cc.colors_reference(cl, Ps, list(sc.bgr))
    assert got["colors"] is not None and got["normals"] is None
    assert np.array_equal(got["colors"], want)
    white = (want == 255).all(axis=1).mean()
    assert 0 < white < 0.5
    e.close()


def test_colors_first_view_wins_ties_and_outside_is_white(lib, scene):
    sc = scene
    e = _engine(sc)
    # view 2 is a copy of view 1's camera with another image: equal PointDepth, the first listed view must win
    e.scene_set_view(2, sc.gray[1], sc.K[1], sc.R[1], sc.C[1], float(sc.dmin[1]), float(sc.dmax[1]), sc.neighbors[1])
    e.scene_set_color(2, np.full_like(sc.bgr[1], 7))
    cl = cc.random_cloud(sc, 3000, seed=6)
    n = cl["nPoints"]
    vs = np.arange(n + 1, dtype=np.uint32) * 2
    views = np.tile(np.array([1, 2], np.uint32), n)
    pts = cl["points"].copy()
    pts[:50] += F(1e4)                                                   # far away: projects outside -> white
    e.scene_cloud_set(pts, vs, views)
    got = e.scene_cloud_finish(estimate_colors=True)
    Ps = [cc.compose_P(sc.K[i], sc.R[i], sc.C[i]) for i in range(sc.n_views)]
    Ps[2] = Ps[1]
    imgs = list(sc.bgr); imgs[2] = np.full_like(sc.bgr[1], 7)
    want = cc.colors_reference(dict(points=pts, viewStart=vs, views=views), Ps, imgs)
    assert np.array_equal(got["colors"], want)
    assert not (want[50:] == 7).all(axis=1).any()                        # never the second, tied view
    e.close()


def test_colors_without_images_is_an_error(lib, scene):
    sc = scene
    e = _engine(sc, colors=False)
    cl = cc.random_cloud(sc, 500, seed=7)
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"])
    with pytest.raises(patchmatch.PatchMatchError):
        e.scene_cloud_finish(estimate_colors=True)
    e.close()


def test_no_cloud_is_a_state_error(lib, scene):
    e = _engine(scene, colors=False)
    with pytest.raises(patchmatch.PatchMatchError):
        e.scene_cloud_finish(estimate_normals=True)
    e.close()


# ---- neighbours --------------------------------------------------------------------------------------------------------------------------
def _check_knn(e, pts, queries, k=16):
    got = e.scene_cloud_knn(queries, k)
    want, d = cc.knn_reference(pts, queries, k)
    want = cc.knn_tie_order(pts, queries, want)
    distinct = d[:, k - 1] < d[:, k] if d.shape[1] > k else np.ones(len(queries), bool)
    assert distinct.mean() > 0.5
    assert np.array_equal(got[distinct], want[distinct])
    return got


def test_knn_equals_kdtree(lib, scene):
    sc = scene
    e = _engine(sc, colors=False)
    cl = cc.random_cloud(sc, 50000, seed=8)
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"])
    q = np.random.default_rng(0).choice(cl["nPoints"], 4000, replace=False).astype(np.uint32)
    got = _check_knn(e, cl["points"], q)
    assert (got[:, 0] == q).mean() > 0.99                                # the point itself is its own nearest neighbour
    e.close()


def test_knn_duplicates_and_ties_follow_the_index_rule(lib, scene):
    sc = scene
    e = _engine(sc, colors=False)
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.25)
    pts = np.concatenate([g, g[::7], g[::11]]).astype(F)                 # a lattice (equal distances everywhere) with exact duplicates
    perm = rng.permutation(len(pts)); pts = pts[perm]
    n = len(pts)
    e.scene_cloud_set(pts, np.arange(n + 1, dtype=np.uint32), np.zeros(n, np.uint32))
    q = np.arange(n, dtype=np.uint32)
    got = e.scene_cloud_knn(q, 16)
    X = pts.astype(np.float64)
    for r in range(n):
        d = ((X - X[r]) ** 2).sum(axis=1)
        d = ((X[:, 0] - X[r, 0]) ** 2 + (X[:, 1] - X[r, 1]) ** 2) + (X[:, 2] - X[r, 2]) ** 2
        want = np.lexsort((np.arange(n), d))[:16]
        assert np.array_equal(got[r], want), r
    e.close()


def test_knn_density_contrast(lib, scene):
    """Two clusters whose densities differ 1000:1 (the grid's cell edge fits one of them only): still exact."""
    sc = scene
    e = _engine(sc, colors=False)
    rng = np.random.default_rng(10)
    dense = rng.uniform(0, 0.1, (15000, 3)); sparse = rng.uniform(0, 1, (1500, 3)) + np.array([2.0, 0, 0]) * 1.0
    pts = np.concatenate([dense, sparse * 10 ** (1 / 3) / 1.0]).astype(F)
    pts = pts[rng.permutation(len(pts))]
    n = len(pts)
    e.scene_cloud_set(pts, np.arange(n + 1, dtype=np.uint32), np.zeros(n, np.uint32))
    q = rng.choice(n, 3000, replace=False).astype(np.uint32)
    _check_knn(e, pts, q)
    small = e.scene_cloud_knn(np.arange(5, dtype=np.uint32), 16)[:, :16]
    assert small.shape == (5, 16)
    e.close()


def test_knn_small_cloud_uses_all_points(lib, scene):
    e = _engine(scene, colors=False)
    pts = np.random.default_rng(11).normal(size=(5, 3)).astype(F)
    e.scene_cloud_set(pts, np.arange(6, dtype=np.uint32), np.zeros(5, np.uint32))
    got = e.scene_cloud_knn(np.arange(5, dtype=np.uint32), 16)
    assert (got[:, 5:] == 0xFFFFFFFF).all()
    for r in range(5):
        assert sorted(got[r, :5]) == list(range(5)) and got[r, 0] == r
    out = e.scene_cloud_finish(estimate_normals=True)
    assert np.allclose(np.linalg.norm(out["normals"], axis=1), 1, atol=1e-6)
    e.close()


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def _check_normals(e, sc, cl, k=16):
    got = e.scene_cloud_finish(estimate_normals=True, n_neighbors=k)
    n = got["nPoints"]
    q = np.arange(n)
    nb = e.scene_cloud_knn(q.astype(np.uint32), k)
    first = got["views"][got["viewStart"][:-1]]
    cf = sc.C[first].astype(F)
    ref, lam = cc.pca_normals(got["points"], nb.astype(np.int64), cf)
    ref, _ = cc.orient(ref, got["points"], cf)
    _, dot = cc.orient(got["normals"], got["points"], cf)
    assert (dot >= 0).all()                                              # the orientation rule holds everywhere
    ok = (lam[:, 1] - lam[:, 0]) > 1e-3 * lam[:, 2]
    ang = cc.angle(got["normals"], ref)
    assert ok.mean() > 0.9
    assert ang[ok].max() < 1e-5, ang[ok].max()
    return got


def test_normals_match_numpy_pca(lib, scene):
    sc = scene
    e = _engine(sc, colors=False)
    cl = cc.random_cloud(sc, 20000, seed=12, jitter=1e-3)
    e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"])
    _check_normals(e, sc, cl)
    e.close()


def test_normals_of_planes_and_spheres(lib, scene):
    sc = scene
    e = _engine(sc, colors=False)
    rng = np.random.default_rng(13)
    # a tilted plane in front of camera 0, then a sphere: the analytic normal (towards camera 0 on the plane)
    C0 = sc.C[0]; fwd = sc.R[0][2]
    nrm = fwd + np.array([0.2, -0.1, 0.05]); nrm /= np.linalg.norm(nrm)
    u = np.cross(nrm, [0, 0, 1.0]); u /= np.linalg.norm(u); v = np.cross(nrm, u)
    centre = C0 + fwd * 5
    ab = rng.uniform(-1, 1, (8000, 2))
    plane = (centre + ab[:, :1] * u + ab[:, 1:] * v).astype(F)
    n = len(plane)
    e.scene_cloud_set(plane, np.arange(n + 1, dtype=np.uint32), np.zeros(n, np.uint32))
    got = e.scene_cloud_finish(estimate_normals=True)["normals"].astype(np.float64)
    want = -nrm if np.dot(nrm, C0 - centre) < 0 else nrm
    assert cc.angle(got, np.broadcast_to(want, got.shape)).max() < 1e-3           # (the float positions of the plane's points are its only noise)
    d = rng.normal(size=(12000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = (centre + d * 0.5).astype(F)
    n = len(sphere)
    e.scene_cloud_set(sphere, np.arange(n + 1, dtype=np.uint32), np.zeros(n, np.uint32))
    got = e.scene_cloud_finish(estimate_normals=True)["normals"].astype(np.float64)
    radial = sphere.astype(np.float64) - centre; radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    ang = np.degrees(cc.angle(got * np.sign(np.einsum("ij,ij->i", got, radial))[:, None], radial))
    assert np.median(ang) < 1.0 and np.percentile(ang, 99) < 3.0
    e.close()


# ---- the Python driver -----------------------------------------------------------------------------------------------------------------
def test_finish_leaves_modes_0_and_2_unchanged(lib, scene):
    from openmvs_amd import densify, optdense
    sc = scene
    e = _engine(sc)
    cl = cc.random_cloud(sc, 3000, seed=14)
    for colors, normals in ((0, 0), (2, 2), (0, 2)):
        e.scene_cloud_set(cl["points"], cl["viewStart"], cl["views"], cl["weights"])
        before = e.scene_cloud_get()
        opt = optdense.defaults(); opt.nEstimateColors = colors; opt.nEstimateNormals = normals
        after = densify.finish_point_cloud(e, None, opt, cloud=before)
        _same(after, before, "modes %d/%d" % (colors, normals))
    e.close()


_REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


def _recon_opt(colors, normals):
    from openmvs_amd import optdense
    opt = optdense.defaults()
    opt.nResolutionLevel = 3; opt.nMinResolution = 40; opt.nNumViews = 8; opt.nSpeckleSize = 20; opt.nEstimationGeometricIters = 1
    opt.nEstimateColors = colors; opt.nEstimateNormals = normals
    return opt


def test_dense_reconstruction_modes_1_and_crop(lib, tmp_path):
    """densify.dense_reconstruction on the pipeline-test scene with --estimate-colors 1 --estimate-normals 1: the saved _dense.mvs carries colours and PCA normals
    that the archive reader loads back; with an OBB on the archive and crop_to_roi, exactly the points roi_contains keeps remain, in the swap-remove order."""
    from openmvs_amd import densify, mvsi
    opt = _recon_opt(1, 1)
    e = patchmatch.PatchMatchHIP(0)
    out = str(tmp_path / "scene_dense.mvs")
    sv, cloud = densify.dense_reconstruction(e, _REAL, out, opt, seed=3)
    assert cloud["nPoints"] > 100 and cloud["colors"] is not None and cloud["normals"] is not None
    assert np.allclose(np.linalg.norm(cloud["normals"], axis=1), 1, atol=1e-5)
    back = mvsi.load(out)
    assert np.array_equal(back.vertices, cloud["points"]) and np.array_equal(back.vertices_normal, cloud["normals"]) and np.array_equal(back.vertices_color, cloud["colors"])
    # the same run without the finishing modes: the fused cloud itself, before colours / normals
    sv0, plain = densify.dense_reconstruction(e, _REAL, None, _recon_opt(0, 0), seed=3)
    assert plain["colors"] is None and plain["normals"] is None and np.array_equal(plain["points"], cloud["points"])
    # a bounded archive: crop_to_roi keeps exactly what roi_contains keeps, in the order of RemovePointsOutside
    sc = mvsi.load(_REAL)
    pts = plain["points"]
    rot = np.eye(3); lo = np.percentile(pts, 20, axis=0); hi = np.percentile(pts, 80, axis=0)
    sc.obb_rot, sc.obb_min, sc.obb_max = rot, lo.astype(np.float64), hi.astype(np.float64)
    base = os.path.dirname(_REAL)
    for im in sc.images:                                                 # (the copy lives elsewhere: absolute image paths)
        im.name = os.path.join(base, im.name)
    bounded = str(tmp_path / "bounded.mvs")
    mvsi.save(bounded, sc)
    sc2 = mvsi.load(bounded)
    assert sc2.is_bounded()
    _, cropped = densify.dense_reconstruction(e, bounded, None, _recon_opt(0, 0), seed=3, crop_to_roi=True)
    keep = sc2.roi_contains(pts)
    want = cc.crop_reference(plain, keep)
    assert 0 < cropped["nPoints"] < plain["nPoints"] and cropped["nPoints"] == int(keep.sum())
    for k in ("points", "viewStart", "views", "weights", "projs"):
        assert np.array_equal(cropped[k], want[k]), k
    e.close()


def test_cloud_params_layout():
    import ctypes as C
    assert C.sizeof(patchmatch.PMHipCloudParams) == 4 + 15 * 4 + 4 + 3 * 4 and patchmatch.PMHIP_ABI_VERSION == 7
