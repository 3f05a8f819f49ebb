"""Host-side mirror of Scene::ComputeDepthMaps (libs/MVS/SceneDensify.cpp:1754-1982) for the HBM-resident engine:
photometric pass, geometric-consistency rounds, per-map post-filters after the last round (nOptimize bits REMOVE_SPECKLES
and FILL_GAPS, :1884-1886,1919-1920,2069-2093), cross-view filter (ADJUST_FILTER, :1955-1980), optional `.dmap` output
(:2095-2117).  Everything between the image upload and the final download stays on the device."""
from __future__ import annotations

import os

import numpy as np

from . import dmap as _dmap

REMOVE_SPECKLES, FILL_GAPS, ADJUST_FILTER = 1, 2, 4   # OPTDENSE::DepthFlags, libs/MVS/DepthMap.h:87-92
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")   # what `--export-depth-maps-name` may name besides .dmap and .pfm: the image writer fails on anything else


def compute_depth_maps(engine, view_ids, params, n_optimize: int = 7, b_filter_adjust: bool = True,
                       n_speckle_size: int = 100, n_ipol_gap_size: int = 7, f_depth_diff_threshold: float = 0.01,
                       n_min_views_filter: int = 2, n_min_views_filter_adjust: int = 1, init_depth=None, init_normal=None, scene=None, dmap_dir=None, image_names=None,
                       export=None, seed_mesh=None):
    """Runs the reference's dense schedule for `view_ids` on a loaded scene (engine.scene_load / scene_set_view).
    `init_depth` / `init_normal` (dicts view id -> map) seed the photometric pass like `InitViews(..., loadDepthMaps=0)` does
    (SceneDensify.cpp:418-460); views without an entry start from random planes.
    `seed_mesh` (dict view id -> (mode, proj, z, normals, faces), `SceneViews.seed_mesh`): the same maps rasterised on the device from the view's point mesh
    (`engine.scene_seed_view`) where `scene_set_maps` would upload them; a view listed here does not read `init_depth`.
    `scene`: the `SceneViews` the engine was loaded from, needed when it holds resampled copies of neighbours (`alias_of`, ViewData::ScaleImage): at every round
    boundary a copy is handed the depth map of the image it stands for, at that image's size and camera (the neighbour's saved .dmap, SceneDensify.cpp:378-393), and
    before the cross-view filter the reference views get their image neighbours back (FilterDepthMap reads arrDepthData[ID], :1049-1299).
    `dmap_dir` (needs `scene`): the reference's file-based checkpoint contract (SceneDensify.cpp:2010-2029,1943-1950).  A view whose `depthNNNN.dmap` is already there
    is NOT estimated in the photometric pass: its depth, normal and confidence maps are read back and the schedule carries on from them (every view takes part in the geometric
    rounds again, as there); every map is written when it has been estimated -- after the photometric pass, after each geometric round (the reference's .geo.dmap + rename)
    and after the filters -- each file atomically (.tmp + rename, DepthData::Save).
    `export`: called as export(stage, ids) where the reference writes its verbose per-view files: "raw" before the per-map filters (SceneDensify.cpp:2075-2076), "" after
    them (EVT_SAVEDEPTHMAP, :2099-2110; after every estimation, as there) and "filtered" after the cross-view filter (:2201-2206).  Returns the views whose maps were
    resumed from files."""
    ids = list(view_ids)
    if dmap_dir is not None and scene is None:
        raise ValueError("dmap_dir needs the scene (cameras, neighbours and depth ranges go into the files)")
    G = int(params.nEstimationGeometricIters)
    alias_of = dict(getattr(scene, "alias_of", None) or {})

    def hand_depths_to_copies():
        for a, j in alias_of.items():
            engine.scene_set_source_depth(a, engine.scene_get_maps(j)[0], scene.K[j], scene.R[j], scene.C[j])

    def image_neighbours():
        for v in ids:
            if alias_of and not np.array_equal(scene.estimate_neighbors[v], scene.neighbors[v]):
                engine.scene_set_view(v, None, scene.K[v], scene.R[v], scene.C[v], float(scene.dmin[v]), float(scene.dmax[v]), scene.neighbors[v])

    def post():
        if export is not None:
            export("raw", ids)
        if n_optimize & REMOVE_SPECKLES:
            engine.scene_remove_small_segments(ids, n_speckle_size, f_depth_diff_threshold)
        if n_optimize & FILL_GAPS:
            engine.scene_gap_interpolation(ids, n_ipol_gap_size, f_depth_diff_threshold)

    def save(which):
        if export is not None and which:
            export("filtered" if which is filtered else "", which)
        if dmap_dir is not None and which:
            save_depth_maps(engine, scene, which, dmap_dir, image_names)

    engine.Init(False)
    resumed = []
    filtered = list(ids)                                       # (its own list object: how `save` knows the call after the cross-view filter)
    for v in ids:
        engine.scene_reset_view(v)
        done = os.path.join(dmap_dir, _dmap.depth_file_name(int(v))) if dmap_dir is not None else None
        if done is not None and os.path.exists(done):          # depthmapComputed (SceneDensify.cpp:2010): loaded instead of estimated
            f = _dmap.load(done)
            want = tuple(scene.sizes[v])[::-1] if getattr(scene, "sizes", None) else (scene.height, scene.width)
            if f["depth_map"].shape != want or f.get("confidence_map") is None:
                raise ValueError("%s does not hold the maps of view %d (%s, expected %s with a confidence map)" % (done, v, f["depth_map"].shape, want))
            normal = f.get("normal_map")
            # a depth map stored without normals gets them from its depths (EstimateNormalMap, SceneDensify.cpp:411-414): on the device when the engine's class has
            # the method (a stand-in that answers every name through __getattr__ does not), else on the host -- the same bits
            on_device = normal is None and callable(getattr(type(engine), "scene_estimate_normals", None))
            if normal is None and not on_device:
                from . import views as _views
                normal = _views.estimate_normal_map(scene.K[v], f["depth_map"])
            engine.scene_set_maps(v, f["depth_map"], normal)
            if on_device:
                engine.scene_estimate_normals([v])
            engine.scene_set_conf(v, f["confidence_map"])
            resumed.append(v)
        elif seed_mesh is not None and v in seed_mesh:
            mode, proj, z, normals, faces = seed_mesh[v]
            engine.scene_seed_view(v, mode, proj, z, normals, faces)
        elif init_depth is not None and v in init_depth:
            engine.scene_set_maps(v, init_depth[v], None if init_normal is None else init_normal.get(v))
    todo = [v for v in ids if v not in resumed]
    if todo:
        engine.scene_estimate(todo, -1, params)
    if G == 0:
        post()
    save(ids if (G == 0 and n_optimize & (REMOVE_SPECKLES | FILL_GAPS)) else todo)
    for g in range(G):
        engine.scene_commit_round()
        hand_depths_to_copies()
        engine.Init(True)
        engine.scene_estimate(ids, g, params)
        if g + 1 == G:
            post()
        save(ids)
    image_neighbours()
    if n_optimize & ADJUST_FILTER:
        engine.scene_filter(ids, b_filter_adjust, n_min_views_filter, n_min_views_filter_adjust, f_depth_diff_threshold, commit=True)
        save(filtered)
    return resumed


def save_depth_maps(engine, scene, view_ids, out_dir: str, image_names=None):
    """DepthData::Save for every view: depthNNNN.dmap next to each other (ComposeDepthFilePath, DepthMap.h:72)."""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for v in view_ids:
        d, n, c = engine.scene_get_maps(v)
        ids = [int(v)] + [int(i) for i in scene.neighbors[v]]
        name = image_names[v] if image_names else "images/%05d.jpg" % v
        p = os.path.join(out_dir, _dmap.depth_file_name(int(v)))
        size = tuple(scene.sizes[v]) if getattr(scene, "sizes", None) else (scene.width, scene.height)
        _dmap.save(p, name, ids, size, scene.K[v], scene.R[v], scene.C[v], float(scene.dmin[v]), float(scene.dmax[v]), d, n, c)
        paths.append(p)
    return paths


def export_view_files(engine, scene, ids, out_dir: str, level: int = 3, tag: str = "", image_saver=None) -> list:
    """What the reference writes per view at verbosity `level` (EVT_SAVEDEPTHMAP, SceneDensify.cpp:2099-2110), made on the engine from the resident maps and named by
    ComposeDepthFilePath (DepthMap.h:72): at level > 2 `depth%04u.png` (DepthMap2Image), `.conf.png` (ExportConfidenceMap; not written without a positive confidence)
    and `.ply` (ExportPointCloud with normals; not written without a valid depth), at level > 4 also `.normal.png` and `.conf.pfm`.  `tag`: "raw" writes only
    `depth%04u.raw.png`, and only at level > 3 (:2075-2076); "filtered" only `.filtered.png` and `.filtered.ply` (:2201-2206).  `scene` names nothing here: the file
    number is the view's index.  `image_saver(path, array)`: how an (h, w[, 3]) uint8 image becomes a file (default `mapexport.save_image`, PIL).  Returns the files."""
    from . import mapexport, plyio
    save = image_saver or mapexport.save_image
    out = []
    if level <= 2 or (tag == "raw" and level <= 3):
        return out
    os.makedirs(out_dir, exist_ok=True)
    for v in ids:
        base = os.path.join(out_dir, "depth%04u." % int(v) + (tag + "." if tag else ""))
        save(base + "png", engine.scene_depth_image(v)[0]); out.append(base + "png")
        if tag == "raw":
            continue
        if tag == "":
            conf = engine.scene_conf_image(v)
            if conf is not None:
                save(base + "conf.png", conf[0]); out.append(base + "conf.png")
        if plyio.save_view_cloud(base + "ply", engine.scene_view_cloud(v, True), True):
            out.append(base + "ply")
        if tag == "" and level > 4:
            save(base + "normal.png", engine.scene_normal_image(v)); out.append(base + "normal.png")
            mapexport.save_pfm(base + "conf.pfm", engine.scene_get_maps(v)[2]); out.append(base + "conf.pfm")
    return out


# ---- scene front end: *.mvs + images -> engine scene -----------------------------------------------------------------------------

class SceneViews:
    """What `Scene::ComputeDepthMaps` has in hand after its preparation steps (libs/MVS/SceneDensify.cpp:1772-1870) for a scene:
    gray images, pixel cameras, neighbour lists, depth ranges and the sparse initial maps.  Same
    attribute names as `synth.Scene`, so `PatchMatchHIP.scene_load` takes either."""

    def __init__(self):
        self.width = self.height = 0
        self.gray = []; self.K = []; self.R = []; self.C = []
        self.dmin = []; self.dmax = []; self.neighbors = []; self.view_scores = []
        self.init_depth = {}; self.init_normal = {}
        self.seed_mesh = {}                         # load_scene(seed_on_device=True): image -> (mode, proj, z, normals, faces), the mesh `scene_seed_view` makes the init maps from
        self.names = []; self.ids = []          # ids: images that passed view selection, in scene order
        self.masks = {}; self.mask_option = False   # ignore masks by image index (1 = process, 0 = ignore); mask_option: OPTDENSE::nIgnoreMaskLabel >= 0
        self.sizes = []                             # (w, h) of every slot: images of another size than the scene's carry their own (pmhip_scene_set_view_sized)
        self.estimate_neighbors = None              # per slot: the slots the ESTIMATION reads (a resampled copy where ViewData::ScaleImage applies); None = `neighbors`
        self.alias_of = {}                          # extra source-only slot -> the image it is a resampled copy of
        self.bgr = []                               # the colour images at the working resolution (B, G, R), for the fused cloud's colours
        self.all_view_scores = {}                   # image -> its WHOLE scored neighbour list (Image::neighbors: fusion order, and what a dense archive stores)
        self.avg_depth = {}                         # image -> average depth of its sparse points (Image::avgDepth)
        self.valid = []                             # per image: it has a pose (Image::IsValid); empty: all have
        self.stored = {}                            # slot -> key of the engine's image store that holds its images (load_scene(..., engine=...): `gray` / `bgr` are None there)

    @property
    def n_views(self):
        return len(self.gray)


def _area_tab(ssize: int, dsize: int, scale: float | None = None):
    """OpenCV's computeResizeAreaTab (imgproc/src/resize.cpp) for one axis: for every destination cell the source cells it covers and their float weights, in order.
    Returns (di, si, alpha) arrays; scale = ssize / dsize in double, the partial cells at both ends weighted by their covered fraction of the cell width."""
    import math
    import numpy as np
    if scale is None:
        scale = ssize / dsize
    di, si, al = [], [], []
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            di.append(dx); si.append(sx1 - 1); al.append(np.float32((sx1 - fsx1) / cell))
        for sx in range(sx1, sx2):
            di.append(dx); si.append(sx); al.append(np.float32(1.0 / cell))
        if fsx2 - sx2 > 1e-3:
            di.append(dx); si.append(sx2); al.append(np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell))
    return np.asarray(di, np.int64), np.asarray(si, np.int64), np.asarray(al, np.float32)


def _accumulate_in_order(dst_n, di, vals):
    """out[di[k]] += vals[k] in k order, in float32 (entries of one destination cell are consecutive: the j-th entries of all cells are added together, j = 0, 1, ...)."""
    import numpy as np
    out = np.zeros((dst_n,) + vals.shape[1:], np.float32)
    first = np.r_[True, di[1:] != di[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(di)), 0))
    rank = np.arange(len(di)) - start
    for j in range(int(rank.max()) + 1 if len(di) else 0):
        m = rank == j
        out[di[m]] = out[di[m]] + vals[m]
    return out


def _resize_area_u8(img, w: int, h: int):
    """cv::resize(img, Size(w, h), 0, 0, INTER_AREA) of an 8-bit image that shrinks on both axes (Image::ResizeImage, libs/MVS/Image.cpp:139-155, reached by
    --max-resolution / nResolutionLevel).  Factor 2 (the default halving, nResolutionLevel = 1): OpenCV's ResizeAreaFastVec for integer pixels, (a + b + c + d + 2) >> 2
    -- round half UP, in integers.  Other exact integer factors (the two axes may have different ones): the integer box sum times the float 1 / (fx fy), saturate_cast = round to nearest-even.  Any other factor: its general area path
    (computeResizeAreaTab + ResizeArea_Invoker, imgproc/src/resize.cpp, restated here -- OpenCV is not vendored with the reference, so this is unpinned): per source
    row the x cells weighted in float and accumulated in table order, the rows then weighted and accumulated in float per destination row, saturate_cast<uchar> = round to
    nearest-even."""
    import numpy as np
    H, W = img.shape[:2]
    if w > W or h > H:
        raise NotImplementedError("image resize %dx%d -> %dx%d: INTER_AREA is implemented for shrinking only (OpenCV enlarges with the bilinear path)" % (W, H, w, h))
    if W % w == 0 and H % h == 0:          # OpenCV's `is_area_fast`: both factors are integers (they may differ)
        fx, fy = W // w, H // h
        s = img.reshape(h, fy, w, fx, -1).astype(np.int64).sum(axis=(1, 3))
        if fx == 2 and fy == 2:
            out = ((s + 2) >> 2).astype(np.uint8)
        else:
            out = np.rint(s.astype(np.float32) * np.float32(1.0 / (fx * fy))).astype(np.uint8)
        return out if img.ndim == 3 else out[..., 0]
    src = img.reshape(H, W, -1).astype(np.float32)
    xdi, xsi, xal = _area_tab(W, w)
    ydi, ysi, yal = _area_tab(H, h)
    # every source row that takes part: buf[dx] = sum over its x cells, in table order
    rows = np.unique(ysi)
    buf = {}
    for sy in rows:
        buf[int(sy)] = _accumulate_in_order(w, xdi, src[sy][xsi] * xal[:, None])
    # destination rows: sum[dx] = beta_0 * buf_0, then += beta_k * buf_k in table order
    vals = np.stack([yal[k] * buf[int(ysi[k])] for k in range(len(ydi))])
    out = _accumulate_in_order(h, ydi, vals)
    out = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out if img.ndim == 3 else out[..., 0]


# ---- DepthData::ViewData::ScaleImage: a neighbour whose footprint differs by 15 % or more is resampled (libs/MVS/DepthMap.h:193-204) -----------------------------

def need_scale_image(scale) -> bool:
    """`NeedScaleImage`: ABS(scale - 1.f) >= 0.15f, in float."""
    import numpy as np
    return bool(np.abs(np.float32(scale) - np.float32(1)) >= np.float32(0.15))


def _resize_area_f32(img, w: int, h: int, scale: float):
    """cv::resize(img, Size(), 1/scale, 1/scale, INTER_AREA) of a float image that shrinks (`scale` = OpenCV's scale_x = scale_y > 1, (w, h) = the destination size it derived).
    An integer `scale`: the "area fast" path -- full f x f blocks are ((a+b)+(c+d))*0.25 for f = 2, else the row-major running sum times 1/f^2; blocks cut by the right /
    bottom border average what is there (the statement of oracle/pm_oracle.cpp's resizeArea, which the estimator's pyramid uses).  Any other factor: the general path
    (computeResizeAreaTab + ResizeArea_Invoker) in float, as `_resize_area_u8` without the final rounding.  OpenCV is not vendored with the reference: unpinned."""
    import numpy as np
    H, W = img.shape
    src = np.ascontiguousarray(img, np.float32)
    f = int(np.rint(scale))
    if abs(scale - f) < np.finfo(np.float64).eps:
        out = np.zeros((h, w), np.float32)
        fw, fh = min(w, W // f), min(h, H // f)                                # destination cells whose block is complete
        if fw and fh:
            blk = src[:fh * f, :fw * f].reshape(fh, f, fw, f)
            if f == 2:
                full = ((blk[:, 0, :, 0] + blk[:, 0, :, 1]) + (blk[:, 1, :, 0] + blk[:, 1, :, 1])) * np.float32(0.25)
            else:
                acc = np.zeros((fh, fw), np.float32)
                for j in range(f):
                    for i in range(f):
                        acc = acc + blk[:, j, :, i]
                full = acc * np.float32(1.0 / (f * f))
            out[:fh, :fw] = full
        for y in range(h):                                                     # cells cut by the border (sizes not divisible by f)
            for x in range(w):
                if y < fh and x < fw:
                    continue
                blk = src[y * f:min(y * f + f, H), x * f:min(x * f + f, W)]
                if blk.size:
                    acc = np.float32(0)
                    for v in blk.reshape(-1):
                        acc = np.float32(acc + v)
                    out[y, x] = acc / np.float32(blk.size)
        return out
    xdi, xsi, xal = _area_tab(W, w, scale)
    ydi, ysi, yal = _area_tab(H, h, scale)
    buf = {int(sy): _accumulate_in_order(w, xdi, src[sy][xsi] * xal) for sy in np.unique(ysi)}
    vals = np.stack([yal[k] * buf[int(ysi[k])] for k in range(len(ydi))])
    return _accumulate_in_order(h, ydi, vals)


def _cubic_coeffs(x):
    """interpolateCubic (imgproc/src/resize.cpp), A = -0.75, in float."""
    import numpy as np
    f = np.float32
    A = f(-0.75)
    x = x.astype(np.float32)
    c0 = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    c2 = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    c3 = f(1) - c0 - c1 - c2
    return c0, c1, c2, c3


def _resize_cubic_f32(img, w: int, h: int, scale: float):
    """cv::resize(img, Size(), 1/scale, 1/scale, INTER_CUBIC) of a float image (`scale` = OpenCV's scale_x = scale_y < 1 when enlarging): resizeGeneric_ with
    HResizeCubic / VResizeCubic in their scalar form -- source position (d + 0.5) * scale - 0.5 in float, four taps around its floor with interpolateCubic's weights,
    taps outside the image clamped to the border, rows first, then columns, each as ((t0*c0 + t1*c1) + t2*c2) + t3*c3 in float.  OpenCV's own SIMD column pass fuses and
    reorders these products depending on how it was built, so the last bit of this resampling is not defined by the reference either: unpinned."""
    import numpy as np
    H, W = img.shape
    src = np.ascontiguousarray(img, np.float32)

    def taps(n_dst, n_src):
        fx = ((np.arange(n_dst) + 0.5) * scale - 0.5).astype(np.float32)
        sx = np.floor(fx).astype(np.int64)
        fx = fx - sx.astype(np.float32)
        idx = np.clip(sx[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
        return idx, _cubic_coeffs(fx)

    xi, (a0, a1, a2, a3) = taps(w, W)
    rows = ((src[:, xi[:, 0]] * a0 + src[:, xi[:, 1]] * a1) + src[:, xi[:, 2]] * a2) + src[:, xi[:, 3]] * a3          # [H, w]
    yi, (b0, b1, b2, b3) = taps(h, H)
    return (((rows[yi[:, 0]] * b0[:, None] + rows[yi[:, 1]] * b1[:, None]) + rows[yi[:, 2]] * b2[:, None]) + rows[yi[:, 3]] * b3[:, None]).astype(np.float32)


def scale_image(gray, scale):
    """`DepthData::ViewData::ScaleImage` (libs/MVS/DepthMap.h:198-204): None if the scale is within 15 % of 1, else cv::resize(image, Size(), scale, scale,
    scale > 1 ? INTER_CUBIC : INTER_AREA) -- destination size saturate_cast<int>(size * scale) (round half to even)."""
    import numpy as np
    if not need_scale_image(scale):
        return None
    s = float(np.float32(scale))
    H, W = gray.shape
    w, h = int(np.rint(W * s)), int(np.rint(H * s))
    if w < 1 or h < 1:
        raise ValueError("scale %g leaves no image" % s)
    return _resize_cubic_f32(gray, w, h, 1.0 / s) if s > 1 else _resize_area_f32(gray, w, h, 1.0 / s)


def load_scene(mvs_path: str, opt=None, image_loader=None, view_neighbors_file=None, ignore_mask_label=None, mask_path=None, mask_loader=None, engine=None,
               mesh=None, mesh_engine=None, seed_on_device=False):
    """Reads an MVSI scene and its images and runs view selection + depth initialisation for every valid image.

    `opt`: a `views.DenseOptions` or the whole option table (`optdense.OptDense`, e.g. from `optdense.load(<--dense-config-file>)`).
    `view_neighbors_file`: `DensifyPointCloud --view-neighbors-file` (Scene::LoadViewNeighbors, applied right after the scene is loaded,
    apps/DensifyPointCloud/DensifyPointCloud.cpp:342-343): the listed neighbours replace view selection for those images.
    `ignore_mask_label` (`--ignore-mask-label`; default: the option table's nIgnoreMaskLabel, else off) >= 0: every image's segmentation mask is looked up like
    `DepthEstimator::ImportIgnoreMask` does (the scene's mask name, else <image>.mask.png; `mask_path` = `--mask-path`), read by `mask_loader(path) -> (h,w) labels`
    (default PIL), brought to the working resolution with INTER_NEAREST, and lands in `SceneViews.masks[i]` (1 = process, 0 = ignore) for `scene_set_mask`; an image
    whose mask cannot be read has none, as there (a warning in the reference), but `SceneViews.mask_option` tells the engine that the option is on (SceneDensify.cpp:661).
    `image_loader(path) -> (h,w,3) uint8 RGB` defaults to PIL.
    `engine` (a `PatchMatchHIP`): the images are prepared on the device.  Every decoded image goes straight to the engine's image store (`image_prepare`, key = its
    slot; one decoded image in host memory at a time), every resampled copy is made there (`image_scale`); `SceneViews.gray[i]` / `.bgr[i]` are None and
    `SceneViews.stored` = {slot: key} tells `PatchMatchHIP.scene_load` where the images are.  Sizes, view selection, seed maps and masks are the same (they never
    read pixels), and so are the images, bit for bit.
    `mesh` (`DensifyPointCloud --mesh-file`: a PLY file name, or (vertices, faces)): when no image of the scene carries neighbours, the sparse cloud is replaced by the
    mesh's vertices with the images that see them (`views.sample_mesh_with_visibility`, Scene::ComputeDepthMaps, SceneDensify.cpp:1757-1760) before view selection;
    with `mesh_engine` (a `PatchMatchHIP`) the renders and the visibility test run on the device (`mesh_visibility`) and the mesh is released afterwards.  A scene with
    neighbours ignores the mesh, as there.
    `seed_on_device`: no `init_depth` / `init_normal` maps are made; `SceneViews.seed_mesh[i]` = (mode, proj, z, normals, faces) holds the point mesh
    (`views.point_mesh`) from which `compute_depth_maps(..., seed_mesh=...)` has the engine rasterise the same maps (`scene_seed_view`).  The 5x5 splat of
    `nMinViewsTrustPoint < 2` stays on the host route.  Returns a `SceneViews`."""
    import numpy as np
    from . import mvsi, views
    opt = opt or views.DenseOptions()
    if ignore_mask_label is None:
        ignore_mask_label = int(getattr(opt, "nIgnoreMaskLabel", -1))
    if hasattr(opt, "dense_options"):
        opt = opt.dense_options()
    sc = mvsi.load(mvs_path)
    if view_neighbors_file:
        mvsi.load_view_neighbors(sc, view_neighbors_file)
    base = os.path.dirname(os.path.abspath(mvs_path))
    if image_loader is None:
        def image_loader(p):
            from PIL import Image
            with Image.open(p) as im:
                return np.asarray(im.convert("RGB"))
    sv = SceneViews()
    rgbs, sizes, decoded = [], [], []
    for im in sc.images:
        p = im.name if os.path.isabs(im.name) else os.path.join(base, im.name)
        rgb = image_loader(p)
        H, W = rgb.shape[:2]
        decoded.append((W, H))
        res, _ = views.compute_max_resolution(W, H, opt.nResolutionLevel, opt.nMinResolution, opt.nMaxResolution)
        w, h = views.resized_size(W, H, res)
        if engine is not None:
            engine.image_prepare(len(sizes), rgb, w, h, channel_order=1); sv.stored[len(sizes)] = len(sizes)
            rgb = None
        elif (w, h) != (W, H):
            rgb = _resize_area_u8(rgb, w, h)
        rgbs.append(rgb); sizes.append((w, h))
    sv.width, sv.height = max(set(sizes), key=lambda wh: (sizes.count(wh), -sizes.index(wh)))     # the scene's size: the most frequent one; the other images carry their own
    sv.sizes = list(sizes)
    if ignore_mask_label >= 0:
        sv.mask_option = True
        if mask_loader is None:
            def mask_loader(p):
                from PIL import Image
                with Image.open(p) as im:
                    return np.asarray(im)
        for i, im in enumerate(sc.images):
            name = views.mask_file_name(im.name, im.mask_name, mask_path)
            p = name if os.path.isabs(name) else os.path.join(base, name)
            if mask_path and not os.path.exists(p):
                raise FileNotFoundError("Mask image %s not found" % p)          # DensifyPointCloud.cpp:315-318
            try:
                labels = mask_loader(p)
            except (OSError, ValueError):
                continue                                                         # "warning: can not load the segmentation mask": the image is estimated unmasked
            sv.masks[i] = views.import_ignore_mask(labels, sizes[i], ignore_mask_label)
    if mesh is not None and not any(len(im.view_scores) for im in sc.images):
        replace_cloud_by_mesh(sc, mesh, decoded, mesh_engine)
    cams = views.Cameras(sc, sizes)
    for i, im in enumerate(sc.images):
        sv.gray.append(None if rgbs[i] is None else views.to_gray(rgbs[i])); sv.names.append(im.name)
        sv.bgr.append(None if rgbs[i] is None else np.ascontiguousarray(rgbs[i][..., ::-1]))
        sv.K.append(cams.K[i]); sv.R.append(cams.R[i]); sv.C.append(cams.C[i]); sv.valid.append(bool(im.is_valid()))
        whole = []
        sel = views.select_views(sc, cams, i, opt, all_neighbors=whole) if im.is_valid() else None
        if whole:
            sv.all_view_scores[i] = whole[0]
        if sel is None:
            sv.neighbors.append(np.zeros(0, np.int32)); sv.view_scores.append(None); sv.dmin.append(0.1); sv.dmax.append(100.0)
            continue
        nb, points, sv.avg_depth[i] = sel
        sv.ids.append(i); sv.neighbors.append(nb["ID"].astype(np.int32)); sv.view_scores.append(nb)
        if seed_on_device and opt.nMinViewsTrustPoint >= 2:
            proj, _, vz, normals, faces, dmin, dmax = views.point_mesh(sc, cams, i, points, opt)
            sv.seed_mesh[i] = (1 if not opt.bInitSparse else 0, proj, vz, normals, faces)          # PMHIP_SEED_FACES / PMHIP_SEED_POINTS
        else:
            d, n, dmin, dmax = views.init_depth_map(sc, cams, i, points, opt)
            sv.init_depth[i] = d; sv.init_normal[i] = n
        sv.dmin.append(dmin); sv.dmax.append(dmax)
    # InitViews, SceneDensify.cpp:333-352: a neighbour whose footprint differs by 15 % or more enters the estimation as a RESAMPLED image with the camera of that size
    # (ViewData::ScaleImage).  Each (image, scale) pair becomes an extra source-only slot behind the images; the reference view's estimation list points at it, while
    # `neighbors` keeps the image itself -- whose own depth map, at its own size and camera, is what the geometric rounds, the cross-view filter and the fusion read
    # (cameraDepthMap, :378-393; FilterDepthMap / FuseDepthMaps go through arrDepthData[ID]).
    n_img = len(sc.images)
    sv.estimate_neighbors = [nb.copy() for nb in sv.neighbors]
    made = {}
    for i in sv.ids:
        for k, v in enumerate(sv.view_scores[i]):
            j, scale = int(v["ID"]), np.float32(v["scale"])
            if not need_scale_image(scale):
                continue
            key = (j, float(scale))
            if key not in made:
                if engine is not None:
                    img, size = None, engine.image_scale(len(sv.gray), sv.stored[j], scale); sv.stored[len(sv.gray)] = len(sv.gray)
                else:
                    img = scale_image(sv.gray[j], scale); size = (img.shape[1], img.shape[0])
                Kj, Rj, Cj, w, h = sc.camera(j, size)          # Image::GetCamera(platforms, image.size())
                made[key] = len(sv.gray)
                sv.alias_of[made[key]] = j
                sv.gray.append(img); sv.K.append(Kj); sv.R.append(Rj); sv.C.append(Cj); sv.sizes.append((w, h)); sv.names.append(sv.names[j])
                sv.dmin.append(sv.dmin[j]); sv.dmax.append(sv.dmax[j]); sv.neighbors.append(np.zeros(0, np.int32)); sv.estimate_neighbors.append(np.zeros(0, np.int32))
                sv.view_scores.append(None)
            sv.estimate_neighbors[i][k] = made[key]
    assert len(sv.gray) == n_img + len(sv.alias_of)
    return sv


def replace_cloud_by_mesh(sc, mesh, image_sizes, engine=None, max_resolution: int = 320):
    """`Scene::SampleMeshWithVisibility` on an `mvsi.Scene`, in place: vertices and view lists become those of `views.sample_mesh_with_visibility`; normals, colours
    and confidences of the cloud it replaces go (pointcloud.Release()).  `mesh`: a PLY file name or (vertices, faces); `image_sizes`: the images' own (width, height);
    `engine`: a `PatchMatchHIP` that renders and tests on the device (the mesh is released afterwards), None: the host twin."""
    import numpy as np
    from . import meshio, mvsi, views
    V, F = meshio.load_ply(mesh) if isinstance(mesh, (str, os.PathLike)) else mesh
    sc.sizes = list(image_sizes)
    vis = None
    if engine is not None:
        def vis(cams):
            engine.mesh_set(V, F)
            try:
                return engine.mesh_visibility([c[0] for c in cams], [c[1] for c in cams], [c[2] for c in cams], [c[3:] for c in cams], len(V))
            finally:
                engine.mesh_release()
    pts, start, ids = views.sample_mesh_with_visibility(sc, V, F, max_resolution, visibility=vis)
    sc.vertices, sc.vertex_view_start = pts, start
    sc.vertex_views = np.zeros(len(ids), mvsi.VIEW_DTYPE)
    sc.vertex_views["image_id"] = ids
    sc.vertices_normal = np.zeros((0, 3), np.float32); sc.vertices_color = np.zeros((0, 3), np.uint8)
    return sc


def export_mesh_depth_maps(scene, mesh, base_name: str, engine=None, image_saver=None) -> list:
    """`Scene::ExportMeshToDepthMaps(baseName)` (libs/MVS/Scene.cpp:680-736; `DensifyPointCloud --export-depth-maps-name` with `--mesh-file`): the mesh rendered into
    every valid image at the working resolution -- `scene` is a `SceneViews` (`load_scene`), whose sizes and cameras come from the option table as there -- and one file
    per image, named insertBeforeFileExt(base_name, "%04u" % ID).  `.dmap`: depth and normals (vertex normals as `Mesh::ComputeNormalVertices` makes them), IDs = the
    image then its neighbours (`Image::neighbors`, the whole scored list), dMin 0.001, dMax FLT_MAX, no confidence; `.pfm`: depth only, as `TImage::Save` writes it
    (little-endian, rows bottom to top).  An image extension (`IMAGE_EXTENSIONS`), with an engine: the colour-mapped image of `ExportDepthMap` (DepthMap2Image with the range of its
    X84 rule), made by the engine (`depth_image`, pmhip_depth_image) and written by `image_saver(path, array)` (default `mapexport.save_image`, PIL).  The image is the engine's work:
    without an engine an image extension raises ValueError like any other name, it is not made on the host instead.
    `mesh`: a PLY file name or (vertices, faces); `engine`: a `PatchMatchHIP` that renders every image in one call (the mesh is released afterwards), None: the host
    twin `views.project_mesh`.  Returns the file names."""
    import numpy as np
    from . import dmap, mapexport, meshio, views
    i = base_name.rfind(".")
    ext = base_name[i:].lower() if i >= 0 else ""
    if ext not in (".dmap", ".pfm") + (IMAGE_EXTENSIONS if engine is not None else ()):
        raise ValueError("export_mesh_depth_maps: extension '%s' of %s (.dmap: depth and normals, .pfm: depth; with an engine also %s: the colour-mapped depth)"
                         % (ext, base_name, " ".join(IMAGE_EXTENSIONS)))
    V, F = meshio.load_ply(mesh) if isinstance(mesh, (str, os.PathLike)) else mesh
    want_n = ext == ".dmap"
    n_img = scene.n_views - len(getattr(scene, "alias_of", None) or {})
    valid = getattr(scene, "valid", None) or [True] * n_img
    ids = [v for v in range(n_img) if valid[v]]
    if engine is not None:
        engine.mesh_set(V, F)
        try:
            maps = engine.mesh_project([scene.K[v] for v in ids], [scene.R[v] for v in ids], [scene.C[v] for v in ids], [scene.sizes[v] for v in ids], normals=want_n)
        finally:
            engine.mesh_release()
    else:
        N = views.compute_normal_vertices(V, F) if want_n else None
        maps = [views.project_mesh(scene.K[v], scene.R[v], scene.C[v], scene.sizes[v][0], scene.sizes[v][1], V, F, N) for v in ids]
    out = []
    for v, (depth, normal) in zip(ids, maps):
        name = (base_name[:i] + "%04u" % v + base_name[i:]) if i >= 0 else base_name + "%04u" % v
        if want_n:
            nbs = scene.all_view_scores[v]["ID"] if v in (getattr(scene, "all_view_scores", None) or {}) else scene.neighbors[v]
            dmap.save(name, scene.names[v], [v] + [int(k) for k in nbs], scene.sizes[v], scene.K[v], scene.R[v], scene.C[v], 0.001, float(np.finfo(np.float32).max), depth, normal)
        elif ext == ".pfm":
            mapexport.save_pfm(name, depth)
        else:
            (image_saver or mapexport.save_image)(name, engine.depth_image(depth)[0])
        out.append(name)
    return out


# ---- the consumer of the depth maps: fusion and the dense scene archive ---------------------------------------------------------------------------

def fuse_order(scene) -> list:
    """Processing order of `DepthMapsData::FuseDepthMaps` (libs/MVS/SceneDensify.cpp:1406-1452): the images that have a depth map, best connected first -- by the size
    of the image's whole neighbour list (`Image::neighbors`), images without neighbours dropped; equal counts in index order (the reference's sort is not stable there)."""
    n_all = {i: len(scene.all_view_scores[i]) if i in getattr(scene, "all_view_scores", {}) else len(scene.neighbors[i]) for i in scene.ids}
    return sorted((i for i in scene.ids if n_all[i] > 0), key=lambda i: (-n_all[i], i))


def fuse_depth_maps(engine, scene, opt=None, bgr=None) -> dict:
    """`Scene::DenseReconstruction`'s last step (SceneDensify.cpp:1695-1712) on the resident maps: `FuseDepthMaps(pointcloud, nEstimateColors == 2, nEstimateNormals == 2)`
    with `opt` = an `optdense.OptDense` (default: the table's defaults with the application's `--estimate-normals 2`).  `bgr`: {image: (h, w, 3) uint8 BGR} for the colours.
    Returns the MVS::PointCloud fields of `PatchMatchHIP.scene_fuse`."""
    n_min, f_depth, f_normal, colors, normals = 2, 0.01, 25.0, 2, 2
    if opt is not None:
        n_min, f_depth, f_normal, colors, normals = int(opt.nMinViewsFuse), float(opt.fDepthDiffThreshold), float(opt.fNormalDiffThreshold), int(opt.nEstimateColors), int(opt.nEstimateNormals)
    want_color = colors == 2 and bgr is not None
    if want_color:
        for i in range(len(scene.gray) - len(scene.alias_of)):
            if bgr[i] is not None:                                    # (None: the colour image came with the view from the image store)
                engine.scene_set_color(i, bgr[i])
    return engine.scene_fuse(fuse_order(scene), n_min, f_depth, f_normal, want_color, normals == 2)


def finish_point_cloud(engine, scene_or_archive, opt, crop_to_roi: bool = False, border_roi: float = 0.0, cloud: dict | None = None) -> dict | None:
    """The last block of `Scene::DenseReconstruction` (SceneDensify.cpp:1724-1737) on the engine's resident cloud: `RemovePointsOutside(ROI)` when `crop_to_roi` and the
    scene is bounded (the ROI enlarged by `border_roi`: > 0 EnlargePercent, < 0 Enlarge(-border_roi)), then `EstimatePointColors` if `opt.nEstimateColors == 1` and the
    cloud has no colours, then `EstimatePointNormals` (k = 16) if `opt.nEstimateNormals == 1` and it has no normals.  The application crops by default
    (`--crop-to-roi 1`); here it is opt-in.  `scene_or_archive`: the `SceneViews` (its `bgr` images feed the colours), an `mvsi` scene (its OBB is the ROI), or a
    (SceneViews, mvsi scene) pair.  `cloud`: the resident cloud as last returned, handed back unchanged when there is nothing to do.  Returns the finished cloud."""
    parts = scene_or_archive if isinstance(scene_or_archive, tuple) else (scene_or_archive,)
    views = next((p for p in parts if p is not None and hasattr(p, "bgr")), None)
    archive = next((p for p in parts if p is not None and hasattr(p, "obb_rot")), None)
    colors = opt is not None and int(opt.nEstimateColors) == 1 and (cloud is None or cloud.get("colors") is None)
    normals = opt is not None and int(opt.nEstimateNormals) == 1 and (cloud is None or cloud.get("normals") is None)
    obb = archive._obb() if crop_to_roi and archive is not None and archive.is_bounded() else None
    if cloud is not None and cloud.get("nPoints", 0) == 0:
        return cloud                                                  # the reference skips the block for an empty cloud
    if obb is None and not colors and not normals:
        return cloud
    if colors:
        if views is None:
            raise ValueError("finish_point_cloud: colours need the SceneViews with the images")
        for i in range(len(views.gray) - len(getattr(views, "alias_of", {}))):
            if views.bgr[i] is not None:
                engine.scene_set_color(i, views.bgr[i])
    out = engine.scene_cloud_finish(crop_obb=obb, border_roi=float(border_roi), estimate_colors=colors, estimate_normals=normals)
    out.setdefault("nDepths", (cloud or {}).get("nDepths", 0))
    if cloud is not None and "rounds" in cloud:
        out["rounds"] = cloud["rounds"]
    return out


def save_dense_scene(mvs_in: str, mvs_out: str, cloud: dict, scene=None, version: int | None = None) -> None:
    """What `DensifyPointCloud` leaves behind as `<scene>_dense.mvs` (`Scene::SaveInterface`, libs/MVS/Scene.cpp:218-300): the input archive with the fused cloud in place
    of the sparse points -- position, the images that see the point with the fusion weight as `confidence`, normal, colour (Col3: B, G, R) -- and, when `scene`
    (the `SceneViews`) is given and the archive version stores them (> 6), every image's whole scored neighbour list and average depth."""
    import numpy as np
    from . import mvsi
    sc = mvsi.load(mvs_in)
    P = int(cloud["nPoints"])
    sc.vertices = np.ascontiguousarray(cloud["points"], np.float32).reshape(P, 3)
    sc.vertex_view_start = np.asarray(cloud["viewStart"], np.int64)
    vv = np.zeros(len(cloud["views"]), mvsi.VIEW_DTYPE)
    vv["image_id"] = cloud["views"]; vv["confidence"] = cloud["weights"]
    sc.vertex_views = vv
    sc.vertices_normal = np.zeros((0, 3), np.float32) if cloud.get("normals") is None else np.ascontiguousarray(cloud["normals"], np.float32).reshape(P, 3)
    sc.vertices_color = np.zeros((0, 3), np.uint8) if cloud.get("colors") is None else np.ascontiguousarray(cloud["colors"], np.uint8).reshape(P, 3)
    if scene is not None:
        for i, nb in getattr(scene, "all_view_scores", {}).items():
            sc.images[i].view_scores = np.ascontiguousarray(nb, mvsi.VIEW_SCORE_DTYPE)
        for i, a in getattr(scene, "avg_depth", {}).items():
            sc.images[i].avg_depth = float(a)
    mvsi.save(mvs_out, sc, version=version)


def archive_cones(sc):
    """The cones of `Scene::PointCloudFilter` for an `mvsi` scene: (C (n, 3) double, angle (n,) float32) with angle = float(ComputeFOV(0) / width) and
    ComputeFOV(0) = 2 atan(width / (2 K00)) at each image's own resolution (Image.cpp:209-213); zeros for an image without a pose."""
    import numpy as np
    n = len(sc.images)
    C = np.zeros((n, 3), np.float64); ang = np.zeros(n, np.float32)
    for i, im in enumerate(sc.images):
        if not im.is_valid():
            continue
        K, _, Ci, w, _ = sc.camera(i)
        C[i] = Ci; ang[i] = np.float32(2.0 * np.arctan(float(w) / (2.0 * float(K[0, 0]))) / float(w))
    return C, ang


def filter_point_cloud(engine, mvs_in: str, mvs_out: str | None = None, th_remove: int = -1, min_views: int = 0) -> dict:
    """The application's modes `--filter-point-cloud th_remove` (DensifyPointCloud.cpp:367-374, `Scene::PointCloudFilter`; run when negative) and
    `--export-number-views -min_views` (:375-388, `PointCloud::RemoveMinViews`) on an archive: its vertices, view lists, confidences, colours and normals are the
    cloud, the cameras are taken at each image's own resolution, the cloud is filtered on the engine and the archive is written to `mvs_out` with the fields of
    `save_dense_scene`.  No image file is read, and the engine needs no scene.  Returns the filtered cloud (`PatchMatchHIP.scene_cloud_filter`)."""
    import numpy as np
    from . import mvsi
    sc = mvsi.load(mvs_in)
    P = len(sc.vertices)
    C, ang = archive_cones(sc)
    col = sc.vertices_color if len(sc.vertices_color) == P and P else None
    nrm = sc.vertices_normal if len(sc.vertices_normal) == P and P else None
    engine.scene_cloud_load(sc.vertices, np.asarray(sc.vertex_view_start, np.uint32), sc.vertex_views["image_id"], sc.vertex_views["confidence"], col, nrm, n_cams=len(sc.images))
    out = engine.scene_cloud_filter(th_remove=int(th_remove) if th_remove < 0 else None, min_views=int(min_views), cam_C=C, cam_angle=ang)
    if mvs_out:
        n = int(out["nPoints"])
        sc.vertices = out["points"].reshape(n, 3)
        sc.vertex_view_start = np.asarray(out["viewStart"], np.int64)
        vv = np.zeros(len(out["views"]), mvsi.VIEW_DTYPE)
        vv["image_id"] = out["views"]; vv["confidence"] = out["weights"]
        sc.vertex_views = vv
        sc.vertices_normal = np.zeros((0, 3), np.float32) if out["normals"] is None else out["normals"].reshape(n, 3)
        sc.vertices_color = np.zeros((0, 3), np.uint8) if out["colors"] is None else out["colors"].reshape(n, 3)
        mvsi.save(mvs_out, sc)
    return out


def dense_reconstruction(engine, mvs_in: str, mvs_out: str | None = None, opt=None, seed: int = 0, fusion_mode: int = 0, dmap_dir: str | None = None,
                         crop_to_roi: bool = False, border_roi: float = 0.0, filter_point_cloud: int = 0, prepare_on_device: bool = False, mesh_file: str | None = None,
                         export_level: int = 0, export_dir: str | None = None, ply_out: str | None = None, image_saver=None, export_number_views: int = 0,
                         estimate_scale: float = 0.0, seed_on_device: bool = False, **load_args):
    """`Scene::DenseReconstruction(nFusionMode)` (libs/MVS/SceneDensify.cpp:1655-1750) for the PatchMatch path on one engine: prepare the views (`load_scene`), estimate all
    depth maps with the geometric rounds and the filters the option table asks for (`compute_depth_maps`; with `dmap_dir` under the reference's file contract), and -- unless
    `fusion_mode` is 1, "export depth maps only" -- fuse them and write `<scene>_dense.mvs` to `mvs_out`.  `opt`: an `optdense.OptDense` (default: the table's defaults with the
    application's own `--number-views 8`, `--estimate-normals 2`, `--number-views-fuse` left at the table's 2); `load_args` go to `load_scene` (image_loader,
    view_neighbors_file, ignore_mask_label, mask_path, mask_loader).  The SGM modes (-1, -2) are openmvs_amd.sgm_pipeline's.  After the fusion the cloud is finished
    (`finish_point_cloud`): `crop_to_roi` / `border_roi` as the application's `--crop-to-roi` (default 1 there, off here) / `--border-roi`, colours and normals of modes 1.
    `filter_point_cloud` < 0: `Scene::PointCloudFilter` with that threshold on the finished cloud (`PatchMatchHIP.scene_cloud_filter`; default 0: off).
    `prepare_on_device`: the decoded images are resized, converted and resampled on the engine (`load_scene(..., engine=engine)`) -- the same depth maps and cloud, but the
    returned `SceneViews` has no host images (`gray[i]` / `bgr[i]` are None), which is why it is off by default.
    `seed_on_device`: the initial depth and normal maps are rasterised on the engine from each view's point mesh (`load_scene(..., seed_on_device=True)`,
    `scene_seed_view`) instead of being made on the host and uploaded -- the same bits; off by default, like `prepare_on_device`.
    `mesh_file` (`--mesh-file`): a scene whose images carry no neighbours takes its sparse cloud from this mesh, rendered and tested on the engine (`load_scene(mesh=...)`).
    `export_level` (the application's `-v`): above 2 the reference's per-view images and clouds are written into `export_dir` (default: `dmap_dir`, else the directory of
    `ply_out` or `mvs_out`) by `export_view_files` -- `depthNNNN.raw.png` before the per-map filters (above 3), the `depthNNNN.*` set after them, `depthNNNN.filtered.*`
    after the cross-view filter -- through `image_saver`.  `ply_out`: the final cloud as `<ply_out>.ply` (`PointCloud::Save`, DensifyPointCloud.cpp:421-423; a name that
    already ends in .ply is used as it is).
    `export_number_views` > 0 or `estimate_scale` > 0: `mvs_in` is an existing dense archive, as in the application (DensifyPointCloud.cpp:367-404): nothing is
    estimated, `export_archive_clouds` writes `<ply_out>_Nviews.ply` / `<ply_out>_scale.ply`, and the call returns (None, None).
    Returns (SceneViews, cloud or None)."""
    from . import optdense
    th_filter = int(filter_point_cloud)
    if fusion_mode not in (0, 1):
        raise ValueError("fusion_mode %d: the PatchMatch path is modes 0 (estimate + fuse) and 1 (depth maps only)" % fusion_mode)
    if export_number_views > 0 or estimate_scale > 0:
        base = ply_out or mvs_out or os.path.splitext(mvs_in)[0]
        export_archive_clouds(engine, mvs_in, base[:-4] if base.lower().endswith((".ply", ".mvs")) else base, export_number_views, estimate_scale)
        return None, None
    if opt is None:
        opt = optdense.defaults(); opt.nNumViews = 8; opt.nEstimateNormals = 2
    if mesh_file is not None:
        load_args = dict(load_args, mesh=mesh_file, mesh_engine=engine)
    sv = load_scene(mvs_in, opt=opt, engine=engine if prepare_on_device else None, seed_on_device=seed_on_device, **load_args)
    engine.scene_load(sv, n_levels=int(opt.nSubResolutionLevels))
    export = None
    if export_level > 2:
        where = export_dir or dmap_dir or os.path.dirname(os.path.abspath(ply_out or mvs_out or "."))
        for i in sv.ids:                                             # the per-view clouds take their colours from the resident colour images
            if sv.bgr[i] is not None:
                engine.scene_set_color(i, sv.bgr[i])

        def export(stage, ids):
            export_view_files(engine, sv, ids, where, export_level, stage, image_saver)
    compute_depth_maps(engine, sv.ids, opt.params(seed), n_optimize=int(opt.nOptimize), b_filter_adjust=bool(opt.bFilterAdjust), n_speckle_size=int(opt.nSpeckleSize),
                       n_ipol_gap_size=int(opt.nIpolGapSize), f_depth_diff_threshold=float(opt.fDepthDiffThreshold), n_min_views_filter=int(opt.nMinViewsFilter),
                       n_min_views_filter_adjust=int(opt.nMinViewsFilterAdjust), init_depth=sv.init_depth, init_normal=sv.init_normal, scene=sv, dmap_dir=dmap_dir,
                       image_names=sv.names, export=export, seed_mesh=sv.seed_mesh)
    if fusion_mode == 1:
        return sv, None
    cloud = fuse_depth_maps(engine, sv, opt, bgr=sv.bgr)
    from . import mvsi
    cloud = finish_point_cloud(engine, (sv, mvsi.load(mvs_in) if crop_to_roi else None), opt, crop_to_roi, border_roi, cloud=cloud)
    if th_filter < 0 and cloud["nPoints"]:
        # the cones of the archive's images at their own resolution, as the application's Scene::Load leaves them; aliases of rescaled views are never listed
        C, ang = archive_cones(mvsi.load(mvs_in))
        extra = {k: cloud[k] for k in ("nDepths", "rounds") if k in cloud}
        cloud = dict(engine.scene_cloud_filter(th_remove=th_filter, cam_C=C, cam_angle=ang), **extra)
    if mvs_out:
        save_dense_scene(mvs_in, mvs_out, cloud, sv)
    if ply_out:
        from . import plyio
        plyio.save_point_cloud(ply_out if ply_out.lower().endswith(".ply") else ply_out + ".ply", cloud)
    return sv, cloud


def export_archive_clouds(engine, mvs_in: str, base_name: str, export_number_views: int = 0, estimate_scale: float = 0.0) -> list:
    """The application's two PLY exports of an existing archive: `--export-number-views N` with N > 0 writes `<base>_Nviews.ply` (`PointCloud::SaveNViews`,
    DensifyPointCloud.cpp:375-382), `--estimate-scale s` with s > 0 writes `<base>_scale.ply` (`PointCloud::SaveWithScale` with scaleMult = s, :390-402) -- an archive
    without normals gets them first from `pmhip_scene_cloud_finish`'s PCA normals (EstimatePointNormals, as there).  The cloud is the archive's, the cameras are each
    image's at its own resolution, and the per-point scales are computed on the engine (`scene_cloud_scale`), which gets a scene of cameras only.  Returns the files."""
    import numpy as np
    from . import mvsi, plyio
    sc = mvsi.load(mvs_in)
    P = len(sc.vertices)
    cloud = dict(nPoints=P, points=sc.vertices, viewStart=np.asarray(sc.vertex_view_start, np.uint32), views=np.ascontiguousarray(sc.vertex_views["image_id"], np.uint32),
                 weights=np.ascontiguousarray(sc.vertex_views["confidence"], np.float32), colors=sc.vertices_color if len(sc.vertices_color) == P and P else None,
                 normals=sc.vertices_normal if len(sc.vertices_normal) == P and P else None)
    out = []
    if export_number_views > 0:
        name = "%s_%dviews.ply" % (base_name, export_number_views)
        if plyio.save_point_cloud(name, cloud, min_views=int(export_number_views)):
            out.append(name)
    if estimate_scale > 0 and P:
        n = len(sc.images)
        cams = [sc.camera(i) if sc.images[i].is_valid() else None for i in range(n)]
        w, h = next((c[3], c[4]) for c in cams if c is not None)
        engine.scene_create(max(n, 2), max(int(w), 9), max(int(h), 9), 0)
        for i, c in enumerate(cams):
            if c is not None:
                engine.scene_set_view(i, None, c[0], c[1], c[2], 0.1, 100.0, [])
        engine.scene_cloud_load(cloud["points"], cloud["viewStart"], cloud["views"], cloud["weights"], cloud["colors"], cloud["normals"])
        if cloud["normals"] is None:
            cloud = dict(cloud, normals=engine.scene_cloud_finish(estimate_normals=True)["normals"])
        name = base_name + "_scale.ply"
        if plyio.save_point_cloud(name, cloud, scales=engine.scene_cloud_scale(float(estimate_scale))):
            out.append(name)
    return out
