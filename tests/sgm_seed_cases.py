"""The SGM side of the device seed (include/sgmhip_seed.h; `sgm_pipeline.match_pair(seed_mesh=...)`), shared by tests/test_emu_seed_raster.py and
tests/test_zz_gpu_seed_raster.py: on tests/data/scene the seed rasterised from its mesh and converted on the device equals the host seed through Depth2DisparityMap,
and `match_pair` gives the same disparity and cost whichever route makes the seed -- for tSGM and for plain SGM (min_resolution = 0), on both rectification routes."""
import functools

import numpy as np

from openmvs_amd import rectify, sgm_pipeline, tsgm, views
from tests import sgm_rectify_cases as rc


@functools.lru_cache(maxsize=None)
def scene_pair(level, A=0, B=2):
    """Pair (A, B) of the test scene at `level`, with the counted builders of image A's seed: mesh(w, h) -> (proj, z, faces) with corners, seed(w, h) -> the depth
    map the host rasterises from it (`views.triangulate_points_depth_map`; computed once per size)."""
    scn, cams, bgr, seen = rc.load_scene(level)
    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    X = scn.vertices[seen[A] & seen[B]]
    avg = views.select_neighbor_views(scn, cams, A)[3]
    pts = np.nonzero(seen[A])[0]
    calls = dict(mesh=0, seed=0)

    def KP(w, h):
        K, R, C, _, _ = scn.camera(A, (w, h))
        return K, K @ np.hstack([R, -(R @ C)[:, None]])

    @functools.lru_cache(maxsize=None)
    def host_mesh(w, h):
        proj, _, vert, faces = views.triangulate_points(*KP(w, h), scn.vertices[pts], w, h, avg)
        return proj, np.ascontiguousarray(vert[:, 2]), faces

    @functools.lru_cache(maxsize=None)
    def host_seed(w, h):
        return views.triangulate_points_depth_map(*KP(w, h), scn.vertices[pts], w, h, avg_depth=avg)[0]

    def mesh(w, h):
        calls["mesh"] += 1
        return host_mesh(w, h)

    def seed(w, h):
        calls["seed"] += 1
        return host_seed(w, h)
    return dict(args=(bgr[A], cam(A), bgr[B], cam(B), X), bgr=bgr, ids=(A, B), mesh=mesh, seed=seed, calls=calls)


def seed_steps_case(m, Error, level, min_resolution):
    """`seed_raster` + `seed_disparity` against `Depth2DisparityMap` of the host seed (with corners), at the size the loop's coarsest level asks for; the refusals."""
    import pytest
    p = scene_pair(level)
    bgrA, camA, bgrB, camB, X = p["args"]
    size = (bgrA.shape[1], bgrA.shape[0])
    r = rectify.stereo_rectify_geometry(size, *camA, (bgrB.shape[1], bgrB.shape[0]), *camB, sgm_pipeline.world_to_image3(*camA, X), sgm_pipeline.world_to_image3(*camB, X))
    f = 1 << tsgm.compute_scale(r["size"][0], r["size"][1], min_resolution)
    w, h = r["size"][0] // f * f, r["size"][1] // f * f
    s = 0.5 / f
    sw, sh = sgm_pipeline.compute_resize(size, s)
    H2, Q2 = rectify.scale_stereo_rectification(r["H1"], r["Q"], s)
    hw, hh = sgm_pipeline.compute_resize((w // f, h // f), 0.5)
    grid = (hw - 2 * tsgm.HW, hh - 2 * tsgm.HW)
    proj, z, faces = p["mesh"](sw, sh)
    depth = p["seed"](sw, sh)
    assert len(z) > 100 and len(faces) > 200 and (depth > 0).all()              # with corners the faces cover the image
    m.seed_clear()
    with pytest.raises(Error, match="no seed is resident"):
        m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid)
    got = m.seed_raster(sw, sh, proj, z, faces)
    assert np.array_equal(got.view(np.uint32), depth.view(np.uint32)), "the seed depth map"
    want = m.Depth2DisparityMap(depth, np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid)
    disp = m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid)
    assert disp.dtype == np.int16 and np.array_equal(disp, want) and (want != 32767).any()
    assert m.seed_raster(sw, sh, proj, z, faces, download=False) is None and m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid, download=False) is None
    # refusals: the reason is reported, the seed held before stays, and the next call succeeds
    for bad_proj, bad_z, bad_faces, bad_w, match in ((np.where(np.arange(len(z))[:, None] == 3, np.nan, proj), z, faces, sw, "not finite"),
                                                     (np.where(np.arange(len(z))[:, None] == 3, np.inf, proj), z, faces, sw, "not finite"),
                                                     (proj, np.where(np.arange(len(z)) == 5, 0, z), faces, sw, "vertex 5 has depth"),
                                                     (proj, np.where(np.arange(len(z)) == 5, -2, z), faces, sw, "vertex 5 has depth"),
                                                     (proj, z, np.where(np.arange(len(faces))[:, None] == 1, len(z), faces), sw, "face 1 names vertex"),
                                                     (proj, z, faces, 0, "a map of 0 x")):
        with pytest.raises(Error, match=match):
            m.seed_raster(bad_w, sh, bad_proj, bad_z, bad_faces)
        assert np.array_equal(m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid), want)
    with pytest.raises(Error, match="width or height"):
        m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, (0, 4))
    empty = m.seed_raster(5, 4, np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros((0, 3), np.uint32))
    assert empty.shape == (4, 5) and not empty.any()
    m.seed_clear()
    with pytest.raises(Error, match="no seed is resident"):
        m.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, grid)


def match_pair_seed_routes_agree(m, Error, level, min_resolution):
    """`match_pair` with the seed made on the device (seed_mesh) and on the host (seed_depth), on the device-rectified and the host-rectified route."""
    import pytest
    p = scene_pair(level)
    calls = p["calls"]
    kw = dict(min_resolution=min_resolution, seed_depth=p["seed"], seed_mesh=p["mesh"])
    be = sgm_pipeline.DeviceBackend(m, None)
    assert be.seed_on_device and sgm_pipeline.seeds_on_device(be)
    be.scene_set_images(p["bgr"])
    try:
        m.seed_clear()
        with pytest.raises(Error, match="no seed disparity is resident"):        # a missing seed
            be.rectify_pair(0, 2, np.eye(3), np.eye(3), (64, 48), sgm_pipeline._srgb_table()); m.tsgm_match_rectified(min_resolution=min_resolution, seeded=True)
        before = dict(calls)
        dev = sgm_pipeline.match_pair(be, *p["args"], image_ids=p["ids"], **kw)
        assert calls["mesh"] == before["mesh"] + 1 and calls["seed"] == before["seed"], "the device route takes the mesh and never the map"
        with pytest.raises(Error, match="the first level's seed grid"):          # a wrongly sized seed
            m.seed_disparity(np.eye(3), np.eye(4), 1, (7, 5)); m.tsgm_match_rectified(min_resolution=min_resolution, seeded=True)
        before = dict(calls)
        host_seed = sgm_pipeline.match_pair(sgm_pipeline.DeviceBackend(m, None, seed_on_device=False), *p["args"], image_ids=p["ids"], **kw)
        assert calls["seed"] == before["seed"] + 1 and calls["mesh"] == before["mesh"]
        no_ids = sgm_pipeline.match_pair(be, *p["args"], **kw) if min_resolution else None      # no resident pair: the host route, whatever the backend can do (once: tSGM)
    finally:
        be.scene_clear()
    host_rect = sgm_pipeline.match_pair(sgm_pipeline.DeviceBackend(m, None, rectify_on_device=False), *p["args"], **kw)
    unseeded = sgm_pipeline.match_pair(sgm_pipeline.DeviceBackend(m, None, rectify_on_device=False), *p["args"], min_resolution=min_resolution) if min_resolution else None
    assert dev["seeded"] and (dev["disparity"] != 32767).mean() > 0.3
    for name, other in (("host seed, device-rectified", host_seed), ("host seed, no indices", no_ids), ("host seed, host-rectified", host_rect)):
        if other is None:
            continue
        for k in ("disparity", "cost", "H", "Q"):
            assert np.array_equal(dev[k], other[k]), "%s: %s" % (name, k)
        assert other["seeded"] and dev["image_size"] == other["image_size"]
    if unseeded is not None:
        assert not unseeded["seeded"] and not np.array_equal(unseeded["disparity"], dev["disparity"]), "the seed reaches the loop"
