"""CPU tests of pmhip_scene_cloud_filter (csrc/pm_cloud_filter.hip) under the wave64 emulator: the visibility vote of Scene::PointCloudFilter against the sum
over all points per cone (tests/cloud_filter_cases.py, float32 step by step), the removal against the literal RFOREACH + RemoveAt loop, RemoveMinViews, the
independence of the result from the angular bins, the ABI and the archive driver."""
import ctypes as C
import os

import numpy as np
import pytest

from openmvs_amd import patchmatch, synth
from tests import cloud_cases as cc
from tests import cloud_filter_cases as fc
from tests import emu

F = np.float32


@pytest.fixture(scope="module")
def lib():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as path:
        yield path


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(5, 160, 120, n_src=4)


@pytest.fixture(scope="module")
def floaters(scene):
    """8000 surface points, 8 % of them moved along their first view's ray, with colours and normals."""
    cl = cc.random_cloud(scene, 8000, seed=21)
    cl, _ = fc.move_along_first_ray(cl, scene.C, 0.08, seed=1)
    return fc.with_attributes(cl, seed=2)


def _engine(sc=None):
    e = patchmatch.PatchMatchHIP(0)
    if sc is not None:
        e.scene_load(sc, n_levels=0)
    return e


def _load(e, cl, attrs=True, n_cams=0):
    e.scene_cloud_load(cl["points"], cl["viewStart"], cl["views"], cl["weights"], cl.get("colors") if attrs else None, cl.get("normals") if attrs else None, n_cams=n_cams)


def _same(got, want, what):
    assert got["nPoints"] == want["nPoints"], what
    for k in ("points", "viewStart", "views", "weights", "colors", "normals"):
        if want.get(k) is None:
            assert got.get(k) is None, (what, k)
            continue
        assert np.array_equal(got[k], want[k]), (what, k)


def _check_cones(got, K, widths):
    """The constants the engine used against double precision, to 1 ulp."""
    ang, c2 = fc.cone_constants(K, widths)
    assert np.array_equal(got["cones"][:, 0], ang)
    assert (np.abs(got["cones"][:, 1].astype(np.float64) - c2) <= np.spacing(c2.astype(F)).astype(np.float64)).all()


# ---- exact on whole clouds ---------------------------------------------------------------------------------------------------------------
def test_input_has_floaters_on_both_sides(lib, scene, floaters):
    """Conditions on the test's own input, from the restatement alone."""
    e = _engine(scene); _load(e, floaters)
    cos_sq = e.scene_cloud_filter(th_remove=-1)["cones"][:, 1]
    e.close()
    vis = fc.visibility_reference(floaters, scene.C, cos_sq)
    n = floaters["nPoints"]
    print("\n%d cones, %d non-zero (%d negative, min %d; %d positive, max %d), %d removed at -1" %
          (len(floaters["views"]), (vis != 0).sum(), (vis < 0).sum(), vis.min(), (vis > 0).sum(), vis.max(), (vis <= -1).sum()))
    assert (vis != 0).mean() >= 0.05 and (vis < 0).mean() >= 0.01 and (vis > 0).mean() >= 0.01
    assert 0.02 <= (vis <= -1).mean() <= 0.30


_VOTES = {}


@pytest.mark.parametrize("th_remove", [-1, -4, 0])
@pytest.mark.parametrize("min_views", [0, 2])
@pytest.mark.parametrize("attrs", [True, False])
def test_filter_is_exact_on_a_whole_cloud(lib, scene, floaters, th_remove, min_views, attrs):
    sc = scene
    e = _engine(sc); _load(e, floaters, attrs)
    got = e.scene_cloud_filter(th_remove=th_remove, min_views=min_views)
    e.close()
    _check_cones(got, sc.K, [160] * 5)
    cl = floaters if attrs else dict(floaters, colors=None, normals=None)
    base = fc.remove_min_views(cl, min_views) if min_views else cl
    key = (min_views, got["cones"][:, 1].tobytes())                                            # (the vote depends on neither the threshold nor the attributes)
    if key not in _VOTES:
        _VOTES[key] = fc.visibility_reference(base, sc.C, got["cones"][:, 1])
    vis = _VOTES[key]
    want = cc.crop_reference(base, vis > th_remove)
    assert np.array_equal(got["visibility"], vis)
    _same(got, want, "th %d min_views %d" % (th_remove, min_views))
    assert 0 < got["nPoints"] < floaters["nPoints"]
    assert set(got["times"]) == {"binning", "cones", "removal"} and got["times"]["cones"] > 0


def test_a_point_behind_a_view_it_lists_and_far_outside_its_image(lib, scene, floaters):
    """View lists are the caller's: points behind a camera they list, beside it at right angles, and at its very centre vote and are voted on like any other."""
    sc = scene
    cl = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in floaters.items()}
    fwd = sc.R[0][2]; side = sc.R[0][0]
    pts = cl["points"]
    first = cl["views"][cl["viewStart"][:-1].astype(np.int64)]
    idx = np.nonzero(first == 0)[0][:40]
    assert len(idx) == 40
    pts[idx[:10]] = (sc.C[0] - fwd * np.linspace(2, 6, 10)[:, None]).astype(F)                 # on the optical axis, behind: a chain that occludes itself
    pts[idx[10:20]] = (sc.C[0] + side * np.linspace(2, 6, 10)[:, None]).astype(F)              # at right angles to it
    pts[idx[20:30]] = (sc.C[0] - fwd * 3 + side * np.linspace(-3, 3, 10)[:, None]).astype(F)   # behind, across cube faces
    pts[idx[30]] = sc.C[0].astype(F)                                                          # the camera centre itself: distance 0
    e = _engine(sc); _load(e, cl)
    got = e.scene_cloud_filter(th_remove=-1)
    e.close()
    want, vis = fc.filter_reference(cl, sc.C, got["cones"][:, 1], -1)
    assert (vis[idx[:20]] != 0).sum() >= 10                                                    # the chains do vote on each other
    assert np.array_equal(got["visibility"], vis)
    _same(got, want, "behind")


def test_nothing_removed_everything_removed_and_empty(lib, scene):
    sc = scene
    clean = fc.with_attributes(cc.random_cloud(sc, 3000, seed=22), seed=3)
    e = _engine(sc); _load(e, clean)
    got = e.scene_cloud_filter(th_remove=-1)
    vis = fc.visibility_reference(clean, sc.C, got["cones"][:, 1])
    assert np.array_equal(got["visibility"], vis) and (vis > -1).all()                        # an undisturbed surface: nothing to remove
    _same(got, clean, "nothing removed")
    _load(e, clean)
    got = e.scene_cloud_filter(th_remove=10 ** 6)
    assert got["nPoints"] == 0 and len(got["views"]) == 0 and np.array_equal(got["viewStart"], [0]) and np.array_equal(got["visibility"], vis)
    got = e.scene_cloud_filter(th_remove=-1, min_views=2)                                      # the empty cloud: a no-op
    assert got["nPoints"] == 0 and got["visibility"] is None
    e.scene_cloud_load(np.zeros((0, 3), F), np.zeros(1, np.uint32), np.zeros(0, np.uint32))
    assert e.scene_cloud_filter(th_remove=-1)["nPoints"] == 0
    e.close()


# ---- the accelerator never shows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scaled", "shifted", "narrow", "wide", "very_wide"])
def test_result_does_not_depend_on_the_bins(lib, scene, case):
    sc = scene
    cl = cc.random_cloud(sc, 6000, seed=23)
    cl, _ = fc.move_along_first_ray(cl, sc.C, 0.10, seed=4)
    ang, _ = fc.cone_constants(sc.K, [160] * 5)
    Cc = np.asarray(sc.C, np.float64).copy()
    if case == "scaled":
        cl["points"] = (cl["points"].astype(np.float64) * 1000).astype(F); Cc = Cc * 1000
    elif case == "shifted":
        off = np.array([5000.0, -3000.0, 2000.0])
        cl["points"] = (cl["points"].astype(np.float64) + off).astype(F); Cc = Cc + off
    else:
        ang = (ang * F({"narrow": 0.25, "wide": 4.0, "very_wide": 40.0}[case])).astype(F)
    e = _engine()
    _load(e, cl, n_cams=5)
    got = e.scene_cloud_filter(th_remove=-1, cam_C=Cc, cam_angle=ang)
    e.close()
    assert np.array_equal(got["cones"][:, 0], ang)
    c2 = np.cos(ang.astype(np.float64)) ** 2
    assert (np.abs(got["cones"][:, 1].astype(np.float64) - c2) <= np.spacing(c2.astype(F)).astype(np.float64)).all()
    want, vis = fc.filter_reference(cl, Cc, got["cones"][:, 1], -1)
    print("\n%s: %d non-zero, %d removed" % (case, (vis != 0).sum(), (vis <= -1).sum()))
    if case != "shifted":                                                                       # (far from the origin float32 leaves the rays too coarse to tell)
        assert (vis != 0).sum() >= 10                                                           # a condition on the input: the case decides something
    assert np.array_equal(got["visibility"], vis)
    _same(got, want, case)


def test_a_view_listed_twice_votes_twice(lib, scene):
    sc = scene
    cl = cc.random_cloud(sc, 1500, seed=24, max_views=1)
    cl, _ = fc.move_along_first_ray(cl, sc.C, 0.10, seed=5)
    n = cl["nPoints"]
    cl["viewStart"] = (np.arange(n + 1) * 2).astype(np.uint32); cl["views"] = np.repeat(cl["views"], 2); cl["weights"] = np.repeat(cl["weights"], 2)
    e = _engine(sc); _load(e, cl)
    got = e.scene_cloud_filter(th_remove=-1)
    e.close()
    want, vis = fc.filter_reference(cl, sc.C, got["cones"][:, 1], -1)
    assert (vis != 0).sum() >= 20 and np.array_equal(got["visibility"], vis)
    _same(got, want, "twice")


# ---- RemoveMinViews, ABI, arguments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_views", [1, 2, 3, 9])
def test_min_views_alone_is_remove_min_views(lib, scene, floaters, min_views):
    e = _engine(scene); _load(e, floaters)
    got = e.scene_cloud_filter(min_views=min_views)
    e.close()
    want = fc.remove_min_views(floaters, min_views)
    assert got["visibility"] is None and got["cones"] is None
    _same(got, want, "min_views %d" % min_views)
    assert (want["nPoints"] == floaters["nPoints"]) == (min_views == 1) and (want["nPoints"] == 0) == (min_views == 9)


def test_abi_and_bad_arguments(lib, scene, floaters):
    assert C.sizeof(patchmatch.PMHipCloudFilterParams) == 4 * 4 + 2 * C.sizeof(C.c_void_p) and patchmatch.PMHIP_ABI_VERSION == 7
    assert patchmatch.load_library().pmhip_abi_version() == 7
    e = _engine()
    with pytest.raises(patchmatch.PatchMatchError):
        e.scene_cloud_filter(th_remove=-1)                                                     # no cloud
    with pytest.raises(patchmatch.PatchMatchError):
        _load(e, floaters)                                                                     # no scene and no camera count
    with pytest.raises(patchmatch.PatchMatchError):
        _load(e, floaters, n_cams=3)                                                           # a view index outside the cameras
    _load(e, floaters, n_cams=5)
    with pytest.raises(patchmatch.PatchMatchError):
        e.scene_cloud_filter(th_remove=-1)                                                     # no scene and no cameras
    with pytest.raises(patchmatch.PatchMatchError):
        e.scene_cloud_filter(th_remove=-1, cam_C=scene.C[:3], cam_angle=np.full(3, 0.005, F))   # a point lists a view outside the cameras
    with pytest.raises(ValueError):
        e.scene_cloud_filter(th_remove=-1, cam_C=scene.C)
    lib_ = e._lib
    assert lib_.pmhip_scene_cloud_filter(e._h, None, None, None) != 0
    prm = patchmatch.PMHipCloudFilterParams(); prm.bVisibility = 1; prm.nCams = 5
    prm.camAngle = np.zeros(5, F).ctypes.data_as(C.POINTER(C.c_float))
    assert lib_.pmhip_scene_cloud_filter(e._h, C.byref(prm), None, None) != 0                  # camAngle without camC
    buf = np.zeros(3, np.int32)
    assert lib_.pmhip_scene_cloud_visibility(e._h, buf.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint64(3)) != 0   # not the size of the last vote
    got = e.scene_cloud_filter(th_remove=-1, cam_C=scene.C, cam_angle=np.full(5, 0.005, F))    # and the engine still works
    assert 0 < got["nPoints"] < floaters["nPoints"]
    e.close()


# ---- the archive driver ------------------------------------------------------------------------------------------------------------------
_REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.mark.parametrize("with_normals", [True, False])
def test_filter_point_cloud_on_an_archive(lib, tmp_path, monkeypatch, with_normals):
    """densify.filter_point_cloud on an archive written by save_dense_scene: the archive read back equals the restatement; no image is opened, no scene loaded."""
    from openmvs_amd import densify, mvsi
    src = mvsi.load(_REAL)
    rng = np.random.default_rng(30)
    rep = 3
    pts = np.repeat(src.vertices, rep, axis=0).astype(np.float64)
    scale = np.linalg.norm(np.ptp(src.vertices, axis=0))
    pts = (pts + rng.normal(0, 2e-3 * scale, pts.shape)).astype(F)
    cnt = np.repeat(np.diff(src.vertex_view_start), rep)
    vs = np.zeros(len(pts) + 1, np.uint32); vs[1:] = np.cumsum(cnt)
    gather = np.concatenate([np.arange(src.vertex_view_start[i // rep], src.vertex_view_start[i // rep + 1]) for i in range(len(pts))])
    cloud = dict(nPoints=len(pts), points=pts, viewStart=vs, views=src.vertex_views["image_id"][gather].astype(np.uint32),
                 weights=rng.uniform(0.1, 2, len(gather)).astype(F))
    Cc, ang = densify.archive_cones(src)
    cloud, _ = fc.move_along_first_ray(cloud, Cc, 0.08, seed=6)
    cloud = fc.with_attributes(cloud, seed=7)
    if not with_normals:
        cloud["normals"] = None
    dense = str(tmp_path / "scene_dense.mvs"); out = str(tmp_path / "scene_dense_filtered.mvs")
    densify.save_dense_scene(_REAL, dense, cloud)

    def no_images(*a, **k):
        raise AssertionError("filter_point_cloud must not open an image")
    from PIL import Image
    monkeypatch.setattr(Image, "open", no_images)
    monkeypatch.setattr(densify, "load_scene", no_images)
    e = _engine()
    got = densify.filter_point_cloud(e, dense, out, th_remove=-1, min_views=2)
    e.close()
    widths = [src.camera(i)[3] for i in range(len(src.images))]
    a2, c2 = fc.cone_constants([src.camera(i)[0] for i in range(len(src.images))], widths)
    assert np.array_equal(got["cones"][:, 0], a2) and np.array_equal(ang, a2)
    want, vis = fc.filter_reference(cloud, Cc, got["cones"][:, 1], -1, 2)
    assert (vis < 0).sum() >= 20 and 0 < want["nPoints"] < cloud["nPoints"]
    assert np.array_equal(got["visibility"], vis)
    back = mvsi.load(out)
    assert np.array_equal(back.vertices, want["points"]) and np.array_equal(back.vertex_view_start, want["viewStart"].astype(np.int64))
    assert np.array_equal(back.vertex_views["image_id"], want["views"]) and np.array_equal(back.vertex_views["confidence"], want["weights"])
    assert np.array_equal(back.vertices_color, want["colors"])
    if with_normals:
        assert np.array_equal(back.vertices_normal, want["normals"])
    else:
        assert len(back.vertices_normal) == 0
    assert len(back.images) == len(src.images)


def test_sampled_restatement_equals_the_full_one(lib, scene, floaters):
    """The cone pre-selection of cloud_filter_cases.visibility_sampled (what the device tests use on clouds too large for the full sum) loses nothing."""
    ang, c2 = fc.cone_constants(scene.K, [160] * 5)
    cos_sq = c2.astype(F)
    tg = np.arange(0, floaters["nPoints"], 3)
    full = fc.visibility_reference(floaters, scene.C, cos_sq, targets=tg)
    assert (full != 0).sum() >= 100
    assert np.array_equal(fc.visibility_sampled(floaters, scene.C, ang, cos_sq, tg), full)


@pytest.mark.parametrize("angle", [0.0004, 0.005, 0.03])
def test_all_directions_around_a_camera(lib, angle):
    """Points all around one camera -- uniformly, and crowded along the edges and into the corners of the cube map the bins live on -- with a second point on
    nearly the same ray for most of them: every face, edge and corner takes part, for a cone far below, at and above the rounding slack of the float test."""
    rng = np.random.default_rng(40)
    d = rng.normal(size=(1500, 3))
    edge = np.stack([np.ones(800), 1 + rng.normal(0, 3 * angle, 800), rng.uniform(-1.2, 1.2, 800)], 1)
    corner = 1 + rng.normal(0, 3 * angle, (500, 3))
    d = np.concatenate([d, edge, corner])
    d = np.stack([d[i, rng.permutation(3)] for i in range(len(d))])
    d *= rng.choice([-1.0, 1.0], d.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Cc = np.array([[0.3, -0.2, 0.1]])
    near = Cc + d * rng.uniform(1, 2, (len(d), 1))
    # the partner: farther along a ray that is off by up to two cone angles
    off = rng.normal(size=d.shape); off -= (off * d).sum(1, keepdims=True) * d; off /= np.linalg.norm(off, axis=1, keepdims=True)
    d2 = d + off * rng.uniform(0, 2 * angle, (len(d), 1)); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    far = Cc + d2 * rng.uniform(2.2, 3, (len(d), 1))
    pts = np.concatenate([near, far[: len(d) * 3 // 4]]).astype(F)
    n = len(pts)
    cl = dict(nPoints=n, points=pts, viewStart=np.arange(n + 1, dtype=np.uint32), views=np.zeros(n, np.uint32), weights=np.ones(n, F))
    e = _engine()
    _load(e, cl, attrs=False, n_cams=1)
    got = e.scene_cloud_filter(th_remove=-1, cam_C=Cc, cam_angle=np.array([angle], F))
    e.close()
    want, vis = fc.filter_reference(cl, Cc, got["cones"][:, 1], -1)
    print("\nangle %g: %d non-zero of %d, %.0f candidates per cone" % (angle, (vis != 0).sum(), n, got["n_candidates"] / got["n_cones"]))
    assert (vis != 0).sum() >= 500                                                             # a condition on the input
    assert np.array_equal(got["visibility"], vis)
    _same(got, want, "all directions")


def test_dense_reconstruction_filter_point_cloud(lib, tmp_path):
    """densify.dense_reconstruction(filter_point_cloud=-1): the fused cloud of the pipeline-test scene filtered with the archive's cameras; off by default."""
    import time
    from openmvs_amd import densify, mvsi, optdense
    opt = optdense.defaults()
    opt.nResolutionLevel = 3; opt.nMinResolution = 40; opt.nNumViews = 8; opt.nSpeckleSize = 20; opt.nEstimationGeometricIters = 1
    opt.nEstimateColors = 1; opt.nEstimateNormals = 1
    e = patchmatch.PatchMatchHIP(0)
    _, plain = densify.dense_reconstruction(e, _REAL, None, opt, seed=3)
    out = str(tmp_path / "scene_dense.mvs")
    _, got = densify.dense_reconstruction(e, _REAL, out, opt, seed=3, filter_point_cloud=-1)
    e.close()
    assert "visibility" not in plain and plain["nPoints"] > 100
    Cc, ang = densify.archive_cones(mvsi.load(_REAL))
    assert np.array_equal(got["cones"][:, 0], ang)
    want, vis = fc.filter_reference(plain, Cc, got["cones"][:, 1], -1)
    print("\n%d fused points, %d votes non-zero, %d kept" % (plain["nPoints"], (vis != 0).sum(), want["nPoints"]))
    assert np.array_equal(got["visibility"], vis)
    _same(got, want, "dense_reconstruction")
    back = mvsi.load(out)
    assert np.array_equal(back.vertices, want["points"]) and np.array_equal(back.vertices_color, want["colors"]) and np.array_equal(back.vertices_normal, want["normals"])
