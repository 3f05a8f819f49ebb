"""Depth maps through the SGM path (`DensifyPointCloud --fusion-mode -1/-2`): for a reference image and each of its best neighbours
`SemiGlobalMatcher::Match(scene, idxImage, numNeighbors, minResolution)` (reference `libs/MVS/SemiGlobalMatcher.cpp:529-736`) -- rectify the pair,
run the tSGM loop, keep the disparity data -- then `SemiGlobalMatcher::Fuse` (`:738-859`): project every pair's disparities into the reference
image and fuse the pair depth maps per pixel.  Orchestration only: the steps are `rectify.py`, `tsgm.py` and the calls of include/sgmhip.h
behind the backend object (see tsgm.py)."""
from __future__ import annotations

import numpy as np

from . import rectify, tsgm


_SRGB = None


def _srgb_table():
    """g_ptrsRGB82RGBf (libs/Common/Types.inl:1595-1607): sRGB2RGB(i / 255.f) in float, with the C library's powf as the reference uses."""
    global _SRGB
    if _SRGB is None:
        import ctypes, ctypes.util
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.powf.restype = ctypes.c_float; libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
        f = np.float32
        t = np.zeros(256, f)
        for i in range(256):
            x = f(i) / f(255)
            t[i] = x * (f(1) / f(12.92)) if x <= f(0.04045) else f(libm.powf(f((x + f(0.055)) * (f(1) / f(1.055))), f(2.4)))
        _SRGB = t
    return _SRGB


def to_gray_linear(bgr):
    """`imageColor.toGray(imageGray, COLOR_BGR2GRAY, bNormalize = true, bSRGB = true)` of the SGM path (libs/MVS/SemiGlobalMatcher.cpp:579-582;
    TImage::toGray, libs/Common/Types.inl:2377-2425): every 8-bit channel through the sRGB -> linear table, then 0.114 B + 0.587 G + 0.299 R."""
    f = np.float32
    t = _srgb_table()
    return (f(0.114) * t[bgr[..., 0]] + f(0.587) * t[bgr[..., 1]]) + f(0.299) * t[bgr[..., 2]]


def world_to_image3(K, R, C, X):
    """Camera::TransformPointW2I3 (libs/MVS/Camera.h:396-399): (x, y, depth) as float32."""
    cx = (np.asarray(X, np.float64) - C) @ R.T
    return np.stack([K[0, 2] + K[0, 0] * cx[:, 0] / cx[:, 2], K[1, 2] + K[1, 1] * cx[:, 1] / cx[:, 2], cx[:, 2]], 1).astype(np.float32)


def compute_resize(size, scale):
    """Image8U::computeResize(size, scale) (libs/Common/Types.inl:2446-2449): cvRound of the scaled extents."""
    return int(np.rint(size[0] * scale)), int(np.rint(size[1] * scale))


def rectifies_on_device(be):
    """The backend keeps the scene's images resident and rectifies pairs itself (`SemiGlobalMatcherHIP.scene_set_images` / `rectify_pair` /
    `tsgm_match_rectified`), and was not told to leave that to the host (`DeviceBackend(..., rectify_on_device=False)`)."""
    return all(hasattr(be, n) for n in ("scene_set_images", "rectify_pair", "tsgm_match_rectified")) and bool(getattr(be, "rectify_on_device", True))


def seeds_on_device(be):
    """The backend rasterises the seed from its mesh, converts it and hands it to the loop on the device (`SemiGlobalMatcherHIP.seed_raster` / `seed_disparity` /
    `tsgm_match_rectified(seeded=True)`), and was not told to leave that to the host (`DeviceBackend(..., seed_on_device=False)`)."""
    return rectifies_on_device(be) and all(hasattr(be, n) for n in ("seed_raster", "seed_disparity")) and bool(getattr(be, "seed_on_device", False))


def match_pair(be, bgrA, camA, bgrB, camB, shared_points, min_resolution=320, subpixel_steps=4, seed_depth=None, image_ids=None, seed_mesh=None):
    """One pair of `Match(scene, ...)`: cam = (K, R, C).  Returns the `.dimap` content: dict(disparity, cost, H, Q, image_size, subpixel_steps)
    or None if the pair cannot be rectified.

    seed_depth: callable (w, h) -> depth map of image A at that size, the rough estimate from the sparse points that the reference makes with
    `TriangulatePoints2DepthMap(..., bAddCorners = true)` (SemiGlobalMatcher.cpp:608-618; `views.triangulate_points_depth_map` or
    `mvsf_triangulate_depth_map`); it becomes the first level's initial disparities through Depth2DisparityMap (`:619-625`).  Without it the
    first level searches the default range around zero.

    seed_mesh: callable (w, h) -> (proj, z, faces), the mesh that depth map is rasterised from (`views.triangulate_points` with corners: z the depth of every
    vertex).  With it, a resident pair (`image_ids`) and a backend that seeds on the device (`seeds_on_device`) the seed is rasterised, converted and consumed there
    and no map crosses to the host; otherwise `seed_depth` is used as before.  Both routes give the same result.

    image_ids: (a, b), the slots of the two images in the backend's resident scene (`be.scene_set_images`).  With them and a backend that
    rectifies (`rectifies_on_device`) the pair is warped, converted to gray and matched on the device and no image travels; otherwise the host
    warps (`rectify.stereo_rectify_images`) and the six images are uploaded for the loop.  Both routes give the same result."""
    p1 = world_to_image3(*camA, shared_points); p2 = world_to_image3(*camB, shared_points)
    on_device = image_ids is not None and rectifies_on_device(be)
    if on_device:
        r = rectify.stereo_rectify_geometry((bgrA.shape[1], bgrA.shape[0]), *camA, (bgrB.shape[1], bgrB.shape[0]), *camB, p1, p2)
    else:
        r = rectify.stereo_rectify_images(bgrA, *camA, bgrB, *camB, p1, p2)
    if r is None:
        return None
    H = r["H1"] if on_device else r["H"]
    k = tsgm.compute_scale(r["size"][0], r["size"][1], min_resolution)
    f = 1 << k
    w, h = r["size"][0] // f * f, r["size"][1] // f * f           # the loop's 8-bit resampler wants multiples of 2^levels: crop right / bottom
    init = None
    seeded = on_device and seed_mesh is not None and seeds_on_device(be)
    if seeded:
        s = 0.5 / f
        sw, sh = compute_resize((bgrA.shape[1], bgrA.shape[0]), s)
        be.seed_raster(sw, sh, *seed_mesh(sw, sh), download=False)
        H2, Q2 = rectify.scale_stereo_rectification(H, r["Q"], s)
        hw, hh = compute_resize((w // f, h // f), 0.5)
        be.seed_disparity(np.linalg.inv(H2), np.linalg.inv(Q2), 1, (hw - 2 * tsgm.HW, hh - 2 * tsgm.HW), download=False)
    elif seed_depth is not None:
        s = 0.5 / f                                               # scale * 0.5
        depth = seed_depth(*compute_resize((bgrA.shape[1], bgrA.shape[0]), s))
        H2, Q2 = rectify.scale_stereo_rectification(H, r["Q"], s)
        hw, hh = compute_resize((w // f, h // f), 0.5)
        init = be.Depth2DisparityMap(depth, np.linalg.inv(H2), np.linalg.inv(Q2), 1, (hw - 2 * tsgm.HW, hh - 2 * tsgm.HW))
    if on_device:                                                 # sgmhip_rectify_pair + sgmhip_tsgm_match_rectified: the crop leaves the pixel coordinates as they are
        be.rectify_pair(image_ids[0], image_ids[1], np.linalg.inv(r["H1"]), np.linalg.inv(r["H2"]), (w, h), _srgb_table())
        if seeded:
            disp, cost, _ = be.tsgm_match_rectified(min_resolution=min_resolution, subpixel_steps=subpixel_steps, seeded=True)
        else:
            disp, cost, _ = be.tsgm_match_rectified(min_resolution=min_resolution, init_left_disparity=init, subpixel_steps=subpixel_steps)
        return dict(disparity=disp, cost=cost, H=H, Q=r["Q"], image_size=(bgrA.shape[1], bgrA.shape[0]), subpixel_steps=subpixel_steps, seeded=seeded or init is not None)
    lb, rb = r["rect1"][:h, :w].copy(), r["rect2"][:h, :w].copy()
    args = (lb, to_gray_linear(lb), rb, to_gray_linear(rb), r["mask1"][:h, :w].copy(), r["mask2"][:h, :w].copy())
    if hasattr(be, "tsgm_match"):                                 # the device runs the whole loop in one resident call (sgmhip_tsgm_match)
        disp, cost, _ = be.tsgm_match(args[0], args[2], args[1], args[3], args[4], args[5], min_resolution=min_resolution, init_left_disparity=init,
                                      subpixel_steps=subpixel_steps)
    else:
        disp, cost, _ = tsgm.tsgm_match(be, *args, min_resolution=min_resolution, init_left_disparity=init, subpixel_steps=subpixel_steps)
    return dict(disparity=disp, cost=cost, H=H, Q=r["Q"], image_size=(bgrA.shape[1], bgrA.shape[0]), subpixel_steps=subpixel_steps, seeded=init is not None)


def fuse_pairs(be, pairs, min_views=2):
    """`SemiGlobalMatcher::Fuse` for pairs that all have the reference image on the left: ProjectDisparity2DepthMap per pair, then the per-pixel
    cluster fusion.  -> (depth map, confidence map) of the reference image."""
    if hasattr(be, "fuse_disparities") and pairs:                 # the device does it in one resident call (sgmhip_fuse_disparities)
        dep, cf, _ = be.fuse_disparities(pairs, pairs[0]["image_size"], min_views)
        return dep, cf
    deps, rgs, cfs = [], [], []
    for p in pairs:
        ok, dep, rg, cf = be.ProjectDisparity2DepthMap(p["disparity"], p["cost"], p["Q"], p["subpixel_steps"], p["image_size"])
        if ok:
            deps.append(dep); rgs.append(rg); cfs.append(cf)
    if not deps:
        w, h = pairs[0]["image_size"] if pairs else (0, 0)
        return np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    return be.FusePairs(deps, rgs, cfs, min_views)


# ---- scene level: `DensifyPointCloud --fusion-mode -1` (disparity maps of every pair) and `-2` (fuse them into depth maps) ------------------------------------------

def _matx(a, b):
    """cv::Matx product: c(i, j) = sum_k a(i, k) b(k, j), accumulated left to right from 0 in double."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    c = np.zeros((a.shape[0], b.shape[1]))
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            s = 0.0
            for k in range(a.shape[1]):
                s += a[i, k] * b[k, j]
            c[i, j] = s
    return c


def swapped_pair_q(Q, cam_left, cam_right):
    """`SemiGlobalMatcher::Fuse` when only the pair (right, left) is on disk (libs/MVS/SemiGlobalMatcher.cpp:767-777): that file's Q puts a disparity of the rectified RIGHT
    image into the right camera's image space; `P * invK * Q` carries it on into the LEFT image -- P = K_left [R | -R C] with (R, C) the pose of the left camera relative to
    the right one (ComputeRelativePose, libs/Common/Util.inl:39-42), invK = the right camera's inverse intrinsics (Camera::InvK)."""
    (Kl, Rl, Cl), (Kr, Rr, Cr) = [tuple(np.asarray(x, np.float64) for x in cam) for cam in (cam_left, cam_right)]
    poseR = _matx(Rl, Rr.T)
    poseC = _matx(Rr, (Cl - Cr)[:, None])[:, 0]
    M = _matx(Kl, poseR)
    P = np.eye(4); P[:3, :3] = M; P[:3, 3] = _matx(M, (-poseC)[:, None])[:, 0]          # AssembleProjectionMatrix (libs/MVS/Camera.cpp:173-180)
    invK = np.eye(4)
    invK[0, 0] = 1.0 / Kr[0, 0]; invK[1, 1] = 1.0 / Kr[1, 1]; invK[0, 2] = -Kr[0, 2] * invK[0, 0]; invK[1, 2] = -Kr[1, 2] * invK[1, 1]   # Camera::InvK, libs/MVS/Camera.h:175-188
    return _matx(_matx(P, invK), Q)


def pair_file_name(a: int, b: int) -> str:
    return "%04u_%04u.dimap" % (a, b)


def _listed(neighbors, n_views, f_min_score_ratio, f_min_score):
    """The neighbours `Match` / `Fuse` walk (:532-540, :742-759): best first, cut at numNeighbors and at the score threshold."""
    if not len(neighbors):
        return []
    f_min = max(np.float32(neighbors[0]["score"]) * np.float32(f_min_score_ratio), np.float32(f_min_score))
    out = []
    for k, nb in enumerate(neighbors):
        if (n_views and k >= n_views) or nb["score"] < f_min:
            break
        out.append(int(nb["ID"]))
    return out


def match_scene(be, sc, cams, bgr, neighbors, out_dir, n_views=0, f_min_score_ratio=0.03, f_min_score=2.0, min_resolution=320, subpixel_steps=4, avg_depth=None):
    """`SemiGlobalMatcher::Match(scene, idxImage, numNeighbors, minResolution)` for every image (DenseReconstruction with nFusionMode == -1, SceneDensify.cpp:2046-2048):
    each image against its listed neighbours -- a pair whose disparity file exists already, in either order, is skipped (:543-545) -- rectified, matched through the tSGM
    loop seeded from the image's sparse points (`match_pair`), written as `<left>_<right>.dimap`.
    sc: mvsi.Scene; cams: views.Cameras; bgr: the colour images; neighbors: {image: its whole scored list (Image::neighbors)}; avg_depth: {image: Image::avgDepth} for the
    seed's corner points.  The seed's mesh (`views.triangulate_points`) is built once per (image, size) and reused for all of that image's pairs; a backend that
    seeds on the device (`seeds_on_device`) gets the mesh, any other the depth map rasterised from it on the host.  Returns the pairs written."""
    import os
    from . import dmap, views
    os.makedirs(out_dir, exist_ok=True)
    own = np.repeat(np.arange(len(sc.vertices)), np.diff(sc.vertex_view_start)); ids = sc.vertex_views["image_id"]
    seen = {}

    def sees(i):
        if i not in seen:
            s = np.zeros(len(sc.vertices), bool); s[own[ids == i]] = True; seen[i] = s
        return seen[i]

    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    listed = {i: _listed(neighbors[i], n_views, f_min_score_ratio, f_min_score) for i in sorted(neighbors)}
    resident = False                                             # the images this run touches are in the backend's scene (uploaded before the first pair, once)
    done = []
    meshes, depths = {}, {}                                      # (image, w, h) -> the seed's mesh / the depth map rasterised from it on the host
    for i in sorted(neighbors):
        meshes.clear(); depths.clear()                           # (an image's pairs follow one another)
        for j in listed[i]:
            if os.path.exists(os.path.join(out_dir, pair_file_name(i, j))) or os.path.exists(os.path.join(out_dir, pair_file_name(j, i))):
                continue
            if not resident and rectifies_on_device(be):
                used = set(listed) | {j_ for js in listed.values() for j_ in js}
                be.scene_set_images([bgr[v] if v in used else None for v in range(max(used) + 1)])
                resident = True
            pts = np.nonzero(sees(i))[0]

            def mesh(w, h, i=i, pts=pts):
                if (i, w, h) not in meshes:
                    K, R, C, _, _ = sc.camera(i, (w, h))
                    P = K @ np.hstack([R, -(R @ C)[:, None]])
                    proj, _, vert, faces = views.triangulate_points(K, P, sc.vertices[pts], w, h, None if avg_depth is None else avg_depth[i])
                    meshes[(i, w, h)] = (proj, np.ascontiguousarray(vert[:, 2]), faces)
                return meshes[(i, w, h)]

            def seed(w, h, i=i):
                if (i, w, h) not in depths:
                    proj, z, faces = mesh(w, h)
                    depths[(i, w, h)] = views.raster_faces_depth_map(proj, z, faces, w, h)
                return depths[(i, w, h)]

            with_seed = avg_depth is not None and len(pts) >= 3
            p = match_pair(be, bgr[i], cam(i), bgr[j], cam(j), sc.vertices[sees(i) & sees(j)], min_resolution=min_resolution, subpixel_steps=subpixel_steps,
                           seed_depth=seed if with_seed else None, image_ids=(i, j) if resident else None, seed_mesh=mesh if with_seed else None)
            if p is None:
                continue                                         # the pair cannot be rectified (:566-567)
            dmap.save_dimap(os.path.join(out_dir, pair_file_name(i, j)), p["image_size"], p["H"], p["Q"], p["subpixel_steps"], p["disparity"], p["cost"])
            done.append((i, j))
    if resident:
        be.scene_clear()
    return done


def _fuse_image(be, cams, sizes, neighbors, pair_dir, i, n_views=0, f_min_score_ratio=0.03, f_min_score=2.0, min_views=2):
    """`SemiGlobalMatcher::Fuse` for image i: (depth, conf), or None when none of its listed pairs has a disparity file."""
    import os
    from . import dmap
    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    pairs = []
    for j in _listed(neighbors[i], n_views, f_min_score_ratio, f_min_score):
        direct, swapped = os.path.join(pair_dir, pair_file_name(i, j)), os.path.join(pair_dir, pair_file_name(j, i))
        if os.path.exists(direct):
            g = dmap.load_dimap(direct)
        elif os.path.exists(swapped):
            g = dmap.load_dimap(swapped)
            g["Q"] = swapped_pair_q(g["Q"], cam(i), cam(j))
        else:
            continue                                         # "no disparity-data file found for image pair"
        pairs.append(dict(disparity=g["disparity"], cost=g["cost"], Q=g["Q"], subpixel_steps=g["subpixel_steps"], image_size=tuple(sizes[i])))
    return fuse_pairs(be, pairs, min_views) if pairs else None


def fuse_scene(be, cams, sizes, neighbors, pair_dir, n_views=0, f_min_score_ratio=0.03, f_min_score=2.0, min_views=2, estimate_normals=True):
    """`SemiGlobalMatcher::Fuse` for every image (DenseReconstruction with nFusionMode == -2, SceneDensify.cpp:2049-2057): the disparity files of the image's listed
    neighbours -- stored as (image, neighbour), or as (neighbour, image) with Q carried over (`swapped_pair_q`) -- projected into the image and fused per pixel; normals from
    the depths (`views.estimate_normal_map`) when `estimate_normals` (nEstimateNormals == 2).  sizes: {image: (w, h)}.
    Returns {image: (depth, normal or None, conf)}; the depth range of such a map is (ZEROTOLERANCE, FLT_MAX), :2056."""
    from . import views
    out = {}
    for i in sorted(neighbors):
        fused = _fuse_image(be, cams, sizes, neighbors, pair_dir, i, n_views, f_min_score_ratio, f_min_score, min_views)
        if fused is None:
            w, h = sizes[i]
            out[i] = (np.zeros((h, w), np.float32), None, np.zeros((h, w), np.float32))
            continue
        depth, conf = fused
        out[i] = (depth, views.estimate_normal_map(cams.K[i], depth) if estimate_normals else None, conf)
    return out


class DeviceBackend:
    """The device behind `match_pair` / `fuse_pairs`: `sgm.SemiGlobalMatcherHIP` has every step of the interface (and the resident loop and fusion, `tsgm_match`,
    `fuse_disparities`) except the float area resampler of the image pyramid, which the PatchMatch library provides (`PatchMatchHIP.resize`).
    rectify_on_device: keep the scene's images resident and rectify every pair on the device (`match_scene`, `match_pair`); False leaves the warps and the gray
    conversion to the host and uploads each pair's images for the loop -- the same results, for A/B runs and tests.
    seed_on_device: the loop's seed is rasterised from its mesh, converted to disparities and consumed on the device (`seeds_on_device`; it needs the resident pair, so
    it follows `rectify_on_device`); False rasterises on the host and uploads the disparities -- the same bits."""

    def __init__(self, matcher, engine, rectify_on_device=True, seed_on_device=True):
        self.m, self.e, self.rectify_on_device, self.seed_on_device = matcher, engine, bool(rectify_on_device), bool(seed_on_device)

    def resize_area_f32(self, img, f):
        return self.e.resize(0, img, f)

    def __getattr__(self, name):
        return getattr(self.m, name)


def to_the_cloud(be, sv, cams, sizes, neighbors, out_dir, opt, mvs_in, mvs_out, crop_to_roi=False, border_roi=0.0, **listing):
    """What `Scene::ComputeDepthMaps` and `DenseReconstruction` do in mode -2 after `SemiGlobalMatcher::Fuse` (SceneDensify.cpp:2053-2117, :1955, :1690-1737), on the
    backend's PatchMatch engine `be.e`, loaded here with the scene `sv` (`densify.load_scene`).  Per image, in order: Fuse (`fuse_pairs`; an image without a pair file holds
    all-zero maps), depth and confidence installed in the resident scene with the range (ZEROTOLERANCE, FLT_MAX) of :2056, EstimateNormalMap on the device
    (`scene_estimate_normals`), RemoveSmallSegments and GapInterpolation per nOptimize, `depthNNNN.dmap` written from the resident maps.  Then the cross-view filter (nOptimize
    & ADJUST_FILTER; the filtered maps are written again), FuseDepthMaps, the crop / colours / normals block and the dense archive at `mvs_out`, with the arguments
    `densify.dense_reconstruction` derives from `opt`.  Depth and confidence travel through the host between the two libraries.  Returns the cloud."""
    from . import densify, mvsi
    engine = be.e
    n_optimize, th = int(opt.nOptimize), float(opt.fDepthDiffThreshold)
    engine.scene_load(sv, n_levels=int(opt.nSubResolutionLevels))
    ids = sorted(neighbors)
    d_min, d_max = 1e-4, float(np.finfo(np.float32).max)              # ZEROTOLERANCE<float>() = FZERO_TOLERANCE (libs/Common/Types.h:579), FLT_MAX
    for i in ids:
        fused = _fuse_image(be, cams, sizes, neighbors, out_dir, i, min_views=2, **listing)
        w, h = sizes[i]
        depth, conf = fused if fused is not None else (np.zeros((h, w), np.float32), np.zeros((h, w), np.float32))
        sv.dmin[i], sv.dmax[i] = d_min, d_max
        engine.scene_set_view(i, None, sv.K[i], sv.R[i], sv.C[i], d_min, d_max, sv.neighbors[i])      # the image neighbours, as the filter and the fusion read them
        engine.scene_set_maps(i, depth, None)
        engine.scene_set_conf(i, conf)
        engine.scene_estimate_normals([i])
        if n_optimize & densify.REMOVE_SPECKLES:
            engine.scene_remove_small_segments([i], int(opt.nSpeckleSize), th)
        if n_optimize & densify.FILL_GAPS:
            engine.scene_gap_interpolation([i], int(opt.nIpolGapSize), th)
        densify.save_depth_maps(engine, sv, [i], out_dir, sv.names)
    if n_optimize & densify.ADJUST_FILTER and ids:
        engine.scene_filter(ids, bool(opt.bFilterAdjust), int(opt.nMinViewsFilter), int(opt.nMinViewsFilterAdjust), th, commit=True)
        densify.save_depth_maps(engine, sv, ids, out_dir, sv.names)
    cloud = densify.fuse_depth_maps(engine, sv, opt, bgr=sv.bgr)
    cloud = densify.finish_point_cloud(engine, (sv, mvsi.load(mvs_in) if crop_to_roi else None), opt, crop_to_roi, border_roi, cloud=cloud)
    densify.save_dense_scene(mvs_in, mvs_out, cloud, sv)
    return cloud


def dense_reconstruction(be, mvs_in, out_dir, fusion_mode, opt=None, image_loader=None, min_resolution=320, mvs_out=None, crop_to_roi=False, border_roi=0.0, seed=0):
    """The SGM modes of `Scene::DenseReconstruction` (libs/MVS/SceneDensify.cpp:1655-1750, :2042-2058): `fusion_mode` -1 writes the disparity files of every image's
    pairs into `out_dir`; -2 fuses the files found there into depth maps and writes `depthNNNN.dmap` (depth, normals when nEstimateNormals == 2, confidence; depth range
    (ZEROTOLERANCE, FLT_MAX) as at :2056).  be: a backend (`DeviceBackend(SemiGlobalMatcherHIP(dev), PatchMatchHIP(dev))`); opt: an `optdense.OptDense` (nNumViews,
    view-score cuts, resolution level); image_loader as in `densify.load_scene`.
    Without `mvs_out` mode -2 stops at the depth maps, which a later `--fusion-mode 0` run fuses into the cloud.  Returns the pairs written (-1) or
    {image: (depth, normal, conf)} (-2).
    `mvs_out` (mode -2 only): the reference's mode -2 through to the cloud (`to_the_cloud` below), the dense archive written there; `crop_to_roi` / `border_roi` as in
    `densify.dense_reconstruction`, and `seed` for the same signature (nothing on this route draws a random number).  Returns the cloud dict of
    `densify.dense_reconstruction`."""
    import os
    from . import densify, dmap, mvsi, optdense, views
    if fusion_mode not in (-1, -2):
        raise ValueError("the SGM path is fusion modes -1 and -2")
    opt = opt or optdense.defaults()
    if mvs_out is not None:
        if fusion_mode != -2:
            raise ValueError("mvs_out: only fusion mode -2 goes on to the cloud (-1 writes the pairs' disparity files)")
        if int(opt.nEstimateNormals) != 2:
            # FuseDepthMaps(pointcloud, nEstimateColors == 2, nEstimateNormals == 2), SceneDensify.cpp:1443-1444,1553: without normal maps the reference fuses with a constant normal
            raise ValueError("mvs_out with nEstimateNormals = %d: the reference then fuses the depth maps without normal maps (bNormalMap == false), "
                             "a fusion mode this engine does not have; set nEstimateNormals = 2" % int(opt.nEstimateNormals))
        if getattr(be, "e", None) is None:
            raise ValueError("mvs_out needs the backend's PatchMatch engine (DeviceBackend.e): the filters and the fusion run there")
    sv = densify.load_scene(mvs_in, opt=opt, image_loader=image_loader)
    sc = mvsi.load(mvs_in)
    cams = views.Cameras(sc, sv.sizes[:len(sc.images)])          # every image at its own size; the slots behind them are PatchMatch's resampled neighbour copies
    nbs = {i: sv.all_view_scores[i] for i in sv.ids if len(sv.all_view_scores.get(i, ()))}
    args = dict(n_views=int(opt.nNumViews), f_min_score_ratio=float(opt.fViewMinScoreRatio), f_min_score=float(opt.fViewMinScore))
    if fusion_mode == -1:
        return match_scene(be, sc, cams, sv.bgr, nbs, out_dir, min_resolution=min_resolution, avg_depth=sv.avg_depth, **args)
    sizes = {i: tuple(sv.sizes[i]) for i in nbs}
    if mvs_out is not None:
        return to_the_cloud(be, sv, cams, sizes, nbs, out_dir, opt, mvs_in, mvs_out, crop_to_roi, border_roi, **args)
    fused = fuse_scene(be, cams, sizes, nbs, out_dir, min_views=2, estimate_normals=int(opt.nEstimateNormals) == 2, **args)
    for i, (depth, normal, conf) in fused.items():
        ids = [i] + [int(v) for v in sv.neighbors[i]]
        dmap.save(os.path.join(out_dir, dmap.depth_file_name(i)), sv.names[i], ids, sizes[i], sv.K[i], sv.R[i], sv.C[i], 1e-4, float(np.finfo(np.float32).max),      # ZEROTOLERANCE<float>() = FZERO_TOLERANCE (libs/Common/Types.h:579), FLT_MAX
                  depth, normal, conf)
    return fused
