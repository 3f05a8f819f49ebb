"""ctypes binding of libpmhip.so -- the host-side mirror of the reference's GPU plug-in.

`PatchMatchHIP` has the same four-method surface as the reference's `PatchMatchCUDA`
(libs/MVS/PatchMatchCUDA.inl:102-108: ctor(device), Init(bGeomConsistency), Release(),
EstimateDepthMap(DepthData&)), plus the HBM-resident scene interface of include/pmhip.h.
There is no CPU fallback: if the HIP library or a GPU is missing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _cabi, build as _build

MAX_SOURCES = 16


class PMHipParams(C.Structure):
    _fields_ = [("nSubResolutionLevels", C.c_uint32), ("nEstimationIters", C.c_uint32),
                ("nEstimationGeometricIters", C.c_uint32), ("nRandomIters", C.c_uint32),
                ("fEstimationGeometricWeight", C.c_float), ("fRandomDepthRatio", C.c_float),
                ("fRandomAngle1Range", C.c_float), ("fRandomAngle2Range", C.c_float),
                ("fRandomSmoothDepth", C.c_float), ("fRandomSmoothNormal", C.c_float),
                ("fRandomSmoothBonus", C.c_float), ("fNCCThresholdKeep", C.c_float),
                ("fDescriptorMinMagnitudeThreshold", C.c_float), ("seed", C.c_uint32)]


class PMHipView(C.Structure):
    _fields_ = [("image", C.POINTER(C.c_float)), ("w", C.c_int32), ("h", C.c_int32),
                ("K", C.c_double * 9), ("R", C.c_double * 9), ("C", C.c_double * 3),
                ("depth", C.POINTER(C.c_float)),
                ("Kd", C.c_double * 9), ("Rd", C.c_double * 9), ("Cd", C.c_double * 3),
                ("id", C.c_uint32), ("dw", C.c_int32), ("dh", C.c_int32)]


class PMHipDepthData(C.Structure):
    _fields_ = [("views", C.POINTER(PMHipView)), ("nViews", C.c_int32),
                ("depthMap", C.POINTER(C.c_float)), ("normalMap", C.POINTER(C.c_float)),
                ("confMap", C.POINTER(C.c_float)), ("dMin", C.c_float), ("dMax", C.c_float)]


class PMHipKernelStats(C.Structure):
    _fields_ = [("sweepLaunches", C.c_uint64), ("sweepMs", C.c_double), ("sweepBytes", C.c_double),
                ("sweepPixels", C.c_uint64), ("initLaunches", C.c_uint64), ("initMs", C.c_double), ("sweepWallMs", C.c_double), ("sweepHostMs", C.c_double)]


class PMHipFuseParams(C.Structure):
    _fields_ = [("nMinViewsFuse", C.c_uint32), ("fDepthDiffThreshold", C.c_float), ("fNormalDiffThreshold", C.c_float),
                ("bEstimateColor", C.c_int32), ("bEstimateNormal", C.c_int32)]


class PMHipCloudParams(C.Structure):
    _fields_ = [("bCrop", C.c_int32), ("obbRot", C.c_float * 9), ("obbPos", C.c_float * 3), ("obbExt", C.c_float * 3), ("fBorderROI", C.c_float),
                ("bEstimateColor", C.c_int32), ("bEstimateNormal", C.c_int32), ("nNeighbors", C.c_int32)]


class PMHipCloudFilterParams(C.Structure):
    _fields_ = [("bVisibility", C.c_int32), ("thRemove", C.c_int32), ("nMinViews", C.c_uint32), ("nCams", C.c_int32),
                ("camC", C.POINTER(C.c_double)), ("camAngle", C.POINTER(C.c_float))]


class PMHipImageStats(C.Structure):
    _fields_ = [("nPrepared", C.c_uint64), ("nScaled", C.c_uint64), ("bytesUploaded", C.c_uint64), ("kernelMs", C.c_double), ("uploadMs", C.c_double)]


PMHIP_ABI_VERSION = 7      # include/pmhip.h


class PMHipTuning(C.Structure):
    _fields_ = [("viewGroups", C.c_int32), ("wideMaxViews", C.c_int32), ("wideHyps", C.c_int32), ("sweepLanes", C.c_int32), ("quadBuffer", C.c_int32), ("widePixels", C.c_int32), ("wide8Pixels", C.c_int32), ("reserved0", C.c_int32)]


_TYPES = {c.__name__: c for c in (PMHipParams, PMHipView, PMHipDepthData, PMHipKernelStats, PMHipFuseParams, PMHipCloudParams, PMHipCloudFilterParams, PMHipImageStats, PMHipTuning)}
_SIGNATURES = _cabi.signatures("pmhip.h", _TYPES)
EXPORTS = list(_SIGNATURES)          # every function include/pmhip.h declares
_NORMALS_SIGNATURES = _cabi.signatures("pmhip_normals.h", _TYPES)          # ... and its companion header, which pmhip.h includes
NORMALS_EXPORTS = list(_NORMALS_SIGNATURES)
_MESH_SIGNATURES = _cabi.signatures("pmhip_mesh.h", _TYPES)
MESH_EXPORTS = list(_MESH_SIGNATURES)
_EXPORT_SIGNATURES = _cabi.signatures("pmhip_export.h", _TYPES)
EXPORT_EXPORTS = list(_EXPORT_SIGNATURES)
_SEED_SIGNATURES = _cabi.signatures("pmhip_seed.h", _TYPES)
SEED_EXPORTS = list(_SEED_SIGNATURES)
SEED_POINTS, SEED_FACES = 0, 1       # include/pmhip_seed.h

_LIB = None


def load_library() -> C.CDLL:
    """Load libpmhip.so (building it first when the sources are newer).  Fails loudly."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("PMHIP_LIB") or _build.build_lib("libpmhip.so")   # PMHIP_LIB: tuning experiments only
        if path is None or not os.path.exists(path):
            raise RuntimeError("libpmhip.so is not built (python -m openmvs_amd.build)")
        lib = C.CDLL(path)
        if hasattr(lib, "hipemu_counters") and os.environ.get("OPENMVS_AMD_TEST_EMULATOR") != "1":
            # tests/cpp/hipemu builds of the kernels exist for the CPU test-suite only; the product never computes on the host
            raise RuntimeError("%s is a CPU-emulated test build, not a device library: refusing to load it outside the test-suite" % path)
        experiment = bool(os.environ.get("PMHIP_LIB"))        # (an older build of the library in an A/B run may lack some entry points; otherwise a missing one raises)
        _cabi.declare(lib, _SIGNATURES, allow_missing=experiment)
        _cabi.declare(lib, _NORMALS_SIGNATURES, allow_missing=experiment)
        _cabi.declare(lib, _MESH_SIGNATURES, allow_missing=experiment)
        _cabi.declare(lib, _EXPORT_SIGNATURES, allow_missing=experiment)
        _cabi.declare(lib, _SEED_SIGNATURES, allow_missing=experiment)
        if hasattr(lib, "pmhip_abi_version") and lib.pmhip_abi_version() != PMHIP_ABI_VERSION and not experiment:
            raise RuntimeError("%s has struct layout version %d, these bindings are written for %d (include/pmhip.h)" % (path, lib.pmhip_abi_version(), PMHIP_ABI_VERSION))
        _LIB = lib
    return _LIB


def default_params(**kw) -> PMHipParams:
    p = PMHipParams()
    load_library().pmhip_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def working_size(W0: int, H0: int, n_resolution_level: int = 1, n_min_resolution: int = 640, n_max_resolution: int = 0):
    """pmhip_working_size: the (w, h) an image of W0 x H0 is brought to (`views.compute_max_resolution` + `views.resized_size`).  Needs no device."""
    w, h = C.c_int(), C.c_int()
    rc = load_library().pmhip_working_size(W0, H0, n_resolution_level, n_min_resolution, n_max_resolution, C.byref(w), C.byref(h))
    if rc != 0:
        raise ValueError("pmhip_working_size(%d, %d): error %d" % (W0, H0, rc))
    return w.value, h.value


def scaled_size(W: int, H: int, scale):
    """pmhip_scaled_size: the (w, h) of `ScaleImage(scale)` of a W x H image, or None when `NeedScaleImage` is false.  Needs no device."""
    w, h = C.c_int(), C.c_int()
    return (w.value, h.value) if load_library().pmhip_scaled_size(W, H, scale, C.byref(w), C.byref(h)) else None


class PatchMatchError(RuntimeError):
    pass


class PatchMatchHIP:
    """Mirror of `class PatchMatchCUDA` (libs/MVS/PatchMatchCUDA.inl:76-139)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._scene = None        # (n_images, w, h) of scene_create
        self._sizes = {}          # slot -> (w, h) of a view with its own size
        self._images = {}         # image-store key -> (w, h, has colour)
        rc = self._lib.pmhip_create(device, C.byref(self._h))
        if rc != 0:
            raise PatchMatchError(f"pmhip_create failed ({rc}): no usable MI355X / HIP device")
        self.params = default_params()

    def _chk(self, rc):
        if rc != 0:
            raise PatchMatchError(f"pmhip error {rc}: {self._lib.pmhip_last_error(self._h).decode()}")

    # -- the four reference methods ---------------------------------------------------------
    def Init(self, bGeomConsistency: bool):
        self._chk(self._lib.pmhip_init(self._h, bool(bGeomConsistency)))

    def Release(self):
        if self._h:
            self._chk(self._lib.pmhip_release(self._h))

    def EstimateDepthMap(self, gray, K, R, Cc, ids, dmin, dmax, depth=None, normal=None, src_depths=None,
                         nGeometricIter: int = -1, params: PMHipParams | None = None, mask=None, mask_option=False, src_depth_cams=None):
        """One depth map.  ids[0] = reference view, ids[1:] = sources (indices into gray/K/R/Cc; the source images may have any size).
        src_depths: dict id -> depth map (any size), required for a geometric round; src_depth_cams: dict id -> (Kd, Rd, Cd), the camera
        stored with that depth map (default: the view's own).  mask: (h, w) uint8, 0 = ignored pixel (DepthData::mask);
        mask_option: OPTDENSE::nIgnoreMaskLabel is set although this view has no mask.  Returns (depth, normal, conf)."""
        p = params or self.params
        n = len(ids)
        views = (PMHipView * n)()
        keep = []
        for k, i in enumerate(ids):
            img = np.ascontiguousarray(gray[i], np.float32); keep.append(img)
            v = views[k]
            v.image = img.ctypes.data_as(C.POINTER(C.c_float)); v.h, v.w = img.shape
            v.K[:] = np.asarray(K[i], np.float64).ravel(); v.R[:] = np.asarray(R[i], np.float64).ravel(); v.C[:] = np.asarray(Cc[i], np.float64).ravel()
            v.id = int(i)
            if k > 0 and src_depths is not None:
                d = np.ascontiguousarray(src_depths[i], np.float32); keep.append(d)
                v.depth = d.ctypes.data_as(C.POINTER(C.c_float)); v.dh, v.dw = d.shape
                if src_depth_cams is not None and i in src_depth_cams:
                    kd, rd, cd = src_depth_cams[i]
                    v.Kd[:] = np.asarray(kd, np.float64).ravel(); v.Rd[:] = np.asarray(rd, np.float64).ravel(); v.Cd[:] = np.asarray(cd, np.float64).ravel()
                else:
                    v.Kd[:] = v.K[:]; v.Rd[:] = v.R[:]; v.Cd[:] = v.C[:]
        h, w = keep[0].shape
        depth = np.zeros((h, w), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32).copy()
        normal = np.zeros((h, w, 3), np.float32) if normal is None else np.ascontiguousarray(normal, np.float32).copy()
        conf = np.zeros((h, w), np.float32)
        dd = PMHipDepthData(views, n, *(a.ctypes.data_as(C.POINTER(C.c_float)) for a in (depth, normal, conf)), float(dmin), float(dmax))
        if mask is None and not mask_option:
            self._chk(self._lib.pmhip_estimate_depth_map(self._h, C.byref(dd), C.byref(p), nGeometricIter))
        else:
            m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
            if m is not None and m.shape != (h, w):
                raise ValueError("mask must have the reference view's size")
            self._chk(self._lib.pmhip_estimate_depth_map_masked(self._h, C.byref(dd), m, bool(mask_option), C.byref(p), nGeometricIter))
        return depth, normal, conf

    # -- HBM-resident scene interface --------------------------------------------------------
    def scene_create(self, n_images, w, h, n_levels=2):
        self._chk(self._lib.pmhip_scene_create(self._h, n_images, w, h, n_levels))
        self._scene = (n_images, w, h); self._sizes = {}

    def scene_set_view(self, idx, gray, K, R, Cc, dmin, dmax, neighbors, device_ptr=None):
        K = np.ascontiguousarray(K, np.float64); R = np.ascontiguousarray(R, np.float64); Cc = np.ascontiguousarray(Cc, np.float64)
        nb = np.ascontiguousarray(neighbors, np.int32)
        src = device_ptr if device_ptr is not None else None if gray is None else np.ascontiguousarray(gray, np.float32)
        if src is not None:
            self._sizes.pop(int(idx), None)       # (an image of the scene's size takes the view back into the scene arrays)
        self._chk(self._lib.pmhip_scene_set_view(self._h, idx, src, device_ptr is not None, K, R, Cc, dmin, dmax, nb, len(nb)))

    def tuning(self, **kw):
        """pmhip_get_tuning / pmhip_set_tuning: how a batch is mapped onto the GPU (viewGroups, wideMaxViews, wideHyps, sweepLanes, quadBuffer, widePixels, wide8Pixels); returns the settings
        in force as a dict.  The results never depend on them."""
        t = PMHipTuning()
        if kw:
            names = {k for k, _ in PMHipTuning._fields_}
            for k, v in kw.items():
                if k not in names:
                    raise KeyError("PMHipTuning has no field %r" % k)
                setattr(t, k, int(v))
            self._chk(self._lib.pmhip_set_tuning(self._h, C.byref(t)))
        self._chk(self._lib.pmhip_get_tuning(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in PMHipTuning._fields_}

    def set_sweep_tiles(self, tile_w: int = 0, tile_h: int = 0):
        """OPT-IN, not the reference's estimator (pmhip_set_sweep_tiles): sweeps run inside tile_w x tile_h tiles, neighbours across a tile border are read as the previous
        sweep left them.  0, 0 = off (the reference's sweep, bit for bit).  The result equals the oracle's with tileW / tileH set."""
        self._chk(self._lib.pmhip_set_sweep_tiles(self._h, tile_w, tile_h))

    def scene_set_view_id(self, idx, view_id):
        """The identity slot idx draws its random numbers under (pmhip_scene_set_view_id): the view's index in the whole scene when this engine holds a part of it."""
        self._chk(self._lib.pmhip_scene_set_view_id(self._h, idx, view_id))

    def scene_load(self, scene, n_levels=2, drop_stored=True):
        """Upload a synth.Scene (or anything with the same attributes).  Slots listed in `scene.stored` ({slot: key}; densify.load_scene(..., engine=self)) adopt their
        images from the image store on the device (scene_set_view_stored); `drop_stored`: the entries are dropped afterwards."""
        self.scene_create(scene.n_views, scene.width, scene.height, n_levels)
        sizes = getattr(scene, "sizes", None) or []
        stored = getattr(scene, "stored", None) or {}
        nbs = getattr(scene, "estimate_neighbors", None) or scene.neighbors       # (a densify.SceneViews lists resampled copies of neighbours here, ViewData::ScaleImage)
        for i in range(scene.n_views):
            if i in stored:
                self.scene_set_view_stored(i, stored[i], scene.K[i], scene.R[i], scene.C[i], float(scene.dmin[i]), float(scene.dmax[i]), nbs[i])
                continue
            own = i < len(sizes) and tuple(sizes[i]) != (scene.width, scene.height)
            (self.scene_set_view_sized if own else self.scene_set_view)(i, scene.gray[i], scene.K[i], scene.R[i], scene.C[i], float(scene.dmin[i]), float(scene.dmax[i]), nbs[i])
        if drop_stored:
            for k in sorted(set(stored.values())):
                self.image_drop(k)
        # ignore masks of a scene loaded with --ignore-mask-label (densify.load_scene): per image where a mask file was found; the option alone already selects the
        # nearest-neighbour level hand-off (SceneDensify.cpp:661)
        for i, m in getattr(scene, "masks", {}).items():
            self.scene_set_mask(i, m)
        if getattr(scene, "mask_option", False):
            self.scene_set_mask_mode(1)

    def scene_set_view_sized(self, idx, gray, K, R, Cc, dmin, dmax, neighbors):
        """A view whose image -- and therefore its depth, normal and confidence maps -- has its own size (pmhip_scene_set_view_sized): a source view or a reference view."""
        g = np.ascontiguousarray(gray, np.float32)
        self._sizes[int(idx)] = (g.shape[1], g.shape[0])
        K = np.ascontiguousarray(K, np.float64); R = np.ascontiguousarray(R, np.float64); Cc = np.ascontiguousarray(Cc, np.float64)
        nb = np.ascontiguousarray(neighbors, np.int32)
        self._chk(self._lib.pmhip_scene_set_view_sized(self._h, idx, g, g.shape[1], g.shape[0], False, K, R, Cc, dmin, dmax, nb, len(nb)))

    # -- the image store: working-resolution images made on the device (include/pmhip.h, section 2b) ---------------------------------
    def image_prepare(self, key, img, w, h, channel_order=1):
        """Entry `key` of the image store gets the BGR u8 and gray f32 images at w x h of the decoded (H0, W0, 3) uint8 image `img` (pmhip_image_prepare: INTER_AREA as
        `densify._resize_area_u8`, gray as `views.to_gray`).  channel_order: 0 = the array is B, G, R; 1 = R, G, B."""
        a = np.ascontiguousarray(img, np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("img must be (h, w, 3) uint8")
        self._chk(self._lib.pmhip_image_prepare(self._h, key, a, a.shape[1], a.shape[0], channel_order, w, h))
        self._images[int(key)] = (int(w), int(h), True)

    def image_scale(self, key, src_key, scale):
        """Entry `key` gets `ScaleImage(gray of entry src_key, scale)`, gray only (pmhip_image_scale: `densify.scale_image`); returns its (w, h)."""
        w, h = C.c_int(), C.c_int()
        self._chk(self._lib.pmhip_image_scale(self._h, key, src_key, scale, C.byref(w), C.byref(h)))
        self._images[int(key)] = (w.value, h.value, False)
        return w.value, h.value

    def image_get(self, key):
        """(gray (h, w) float32, bgr (h, w, 3) uint8 or None for a gray-only entry) of entry `key` (pmhip_image_get)."""
        w, h = C.c_int(), C.c_int()
        self._chk(self._lib.pmhip_image_get(self._h, key, C.byref(w), C.byref(h), None, None))
        gray = np.zeros((h.value, w.value), np.float32)
        self._chk(self._lib.pmhip_image_get(self._h, key, None, None, gray, None))
        bgr = np.zeros((h.value, w.value, 3), np.uint8)
        if self._lib.pmhip_image_get(self._h, key, None, None, None, bgr) != 0:
            bgr = None
        return gray, bgr

    def image_drop(self, key=-1):
        """Free entry `key` of the image store; key < 0: everything (pmhip_image_drop)."""
        self._chk(self._lib.pmhip_image_drop(self._h, key))
        if int(key) < 0:
            self._images = {}
        else:
            self._images.pop(int(key), None)

    def image_bytes(self) -> int:
        """Device memory the image store holds right now (pmhip_image_bytes)."""
        return int(self._lib.pmhip_image_bytes(self._h))

    def image_stats(self, reset=False) -> dict:
        """pmhip_image_stats_get: images prepared / resampled, bytes of decoded images uploaded, kernel time by HIP events and upload time, in ms."""
        s = PMHipImageStats()
        self._chk(self._lib.pmhip_image_stats_get(self._h, C.byref(s), bool(reset)))
        return dict(prepared=int(s.nPrepared), scaled=int(s.nScaled), bytes_uploaded=int(s.bytesUploaded), kernel_ms=float(s.kernelMs), upload_ms=float(s.uploadMs))

    def scene_set_view_stored(self, idx, key, K, R, Cc, dmin, dmax, neighbors):
        """scene_set_view / scene_set_view_sized (by the entry's size) with the stored gray image of entry `key`, read on the device, and its colour image if it has one
        (pmhip_scene_set_view_stored).  The view holds copies."""
        K = np.ascontiguousarray(K, np.float64); R = np.ascontiguousarray(R, np.float64); Cc = np.ascontiguousarray(Cc, np.float64)
        nb = np.ascontiguousarray(neighbors, np.int32)
        self._chk(self._lib.pmhip_scene_set_view_stored(self._h, idx, key, K, R, Cc, dmin, dmax, nb, len(nb)))
        w, h, _ = self._images.get(int(key), (None, None, False))
        if w is None:                                          # (an entry made through the C ABI directly)
            cw, ch = C.c_int(), C.c_int()
            self._chk(self._lib.pmhip_image_get(self._h, key, C.byref(cw), C.byref(ch), None, None)); w, h = cw.value, ch.value
        if (w, h) == tuple(self._scene[1:]):
            self._sizes.pop(int(idx), None)
        else:
            self._sizes[int(idx)] = (w, h)

    def scene_set_source_depth(self, idx, depth, Kd=None, Rd=None, Cd=None):
        """Known depth map of a source view with the camera stored next to it (pmhip_scene_set_source_depth); depth None removes it."""
        if depth is None:
            self._chk(self._lib.pmhip_scene_set_source_depth(self._h, idx, None, 0, 0, None, None, None)); return
        d = np.ascontiguousarray(depth, np.float32)
        Kd = np.ascontiguousarray(Kd, np.float64); Rd = np.ascontiguousarray(Rd, np.float64); Cd = np.ascontiguousarray(Cd, np.float64)
        self._chk(self._lib.pmhip_scene_set_source_depth(self._h, idx, d, d.shape[1], d.shape[0], Kd, Rd, Cd))

    def scene_estimate(self, view_ids, nGeometricIter=-1, params=None, sync=True):
        ids = np.ascontiguousarray(view_ids, np.int32)
        p = params or self.params
        self._chk(self._lib.pmhip_scene_estimate(self._h, ids, len(ids), C.byref(p), nGeometricIter, bool(sync)))

    def scene_commit_round(self):
        self._chk(self._lib.pmhip_scene_commit_round(self._h))

    def scene_reset_view(self, idx):
        self._chk(self._lib.pmhip_scene_reset_view(self._h, idx))

    def scene_set_maps(self, idx, depth=None, normal=None):
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, np.float32)
        self._chk(self._lib.pmhip_scene_set_maps(self._h, idx, d, n))

    def scene_set_mask(self, idx, mask):
        """Ignore mask of a view: (h, w) array, 0 = ignore the pixel (--ignore-mask-label); None removes it."""
        if mask is None:
            self._chk(self._lib.pmhip_scene_set_mask(self._h, idx, None)); return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        w, h = self.view_size(idx)
        if m.shape != (h, w):
            raise ValueError("mask must be (h, w)")
        self._chk(self._lib.pmhip_scene_set_mask(self._h, idx, m))

    def scene_set_mask_mode(self, mode):
        self._chk(self._lib.pmhip_scene_set_mask_mode(self._h, mode))

    def scene_set_conf(self, idx, conf):
        c = np.ascontiguousarray(conf, np.float32)
        self._chk(self._lib.pmhip_scene_set_conf(self._h, idx, c))

    def view_size(self, idx):
        """(w, h) of a view's maps: the scene's, or the view's own (scene_set_view_sized)."""
        _, w, h = self._scene
        return self._sizes.get(int(idx), (w, h))

    def scene_get_maps(self, idx):
        w, h = self.view_size(idx)
        d = np.zeros((h, w), np.float32); n = np.zeros((h, w, 3), np.float32); c = np.zeros((h, w), np.float32)
        self._chk(self._lib.pmhip_scene_get_maps(self._h, idx, d, n, c))
        return d, n, c

    def scene_device_ptr(self, what, idx=0) -> int:
        return int(self._lib.pmhip_scene_device_ptr(self._h, what, idx) or 0)

    def scene_filter(self, view_ids, bAdjust=True, nMinViewsFilter=2, nMinViewsFilterAdjust=1, fDepthDiffThreshold=0.01, commit=True):
        """DepthMapsData::FilterDepthMap for these views (Scene::DenseReconstructionFilter); commit installs the results."""
        ids = np.ascontiguousarray(view_ids, np.int32)
        self._chk(self._lib.pmhip_scene_filter(self._h, ids, len(ids), bool(bAdjust), nMinViewsFilter, nMinViewsFilterAdjust, fDepthDiffThreshold, True))
        if commit:
            self._chk(self._lib.pmhip_scene_filter_commit(self._h))

    def scene_remove_small_segments(self, view_ids, nSpeckleSize=100, fDepthDiffThreshold=0.01):
        ids = np.ascontiguousarray(view_ids, np.int32)
        self._chk(self._lib.pmhip_scene_remove_small_segments(self._h, ids, len(ids), nSpeckleSize, fDepthDiffThreshold))

    def scene_gap_interpolation(self, view_ids, nIpolGapSize=7, fDepthDiffThreshold=0.01):
        ids = np.ascontiguousarray(view_ids, np.int32)
        self._chk(self._lib.pmhip_scene_gap_interpolation(self._h, ids, len(ids), nIpolGapSize, fDepthDiffThreshold))

    def scene_estimate_normals(self, view_ids):
        """MVS::EstimateNormalMap on the device for these views (pmhip_scene_estimate_normals): each one's resident normal map becomes
        `views.estimate_normal_map(K, resident depth)`, bit for bit; depth and confidence stay.  Asynchronous on the engine stream."""
        ids = np.ascontiguousarray(view_ids, np.int32).ravel()
        self._chk(self._lib.pmhip_scene_estimate_normals(self._h, ids, len(ids)))

    def estimate_normal_map(self, K, depth):
        """`views.estimate_normal_map(K, depth)` on the device, host arrays in and out (pmhip_estimate_normal_map); needs no scene."""
        d = np.ascontiguousarray(depth, np.float32)
        if d.ndim != 2:
            raise ValueError("depth must be (h, w)")
        n = np.zeros(d.shape + (3,), np.float32)
        self._chk(self._lib.pmhip_estimate_normal_map(self._h, np.ascontiguousarray(K, np.float64).reshape(9), d, d.shape[1], d.shape[0], n))
        return n

    # -- a mesh rendered into depth and normal maps (include/pmhip_mesh.h) ---------------------
    def mesh_set(self, vertices, faces, vertex_normals=None):
        """The mesh becomes resident (pmhip_mesh_set): vertices (n, 3) float32, faces (m, 3) vertex indices; `vertex_normals` (n, 3), or None: the engine computes them
        as `views.compute_normal_vertices` does.  Returns the vertex normals in use."""
        V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        F = np.asarray(faces).reshape(-1, 3)
        if len(F) and (F.min() < 0 or F.max() > 0xFFFFFFFF):
            raise ValueError("face indices must be vertex indices")
        F = np.ascontiguousarray(F, np.uint32)
        N = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, np.float32).reshape(-1, 3)
        if N is not None and N.shape != V.shape:
            raise ValueError("one normal per vertex")
        self._chk(self._lib.pmhip_mesh_set(self._h, V, len(V), F, len(F), N))
        out = np.zeros_like(V)
        self._chk(self._lib.pmhip_mesh_get_vertex_normals(self._h, out))
        return out

    @staticmethod
    def _mesh_views(K, R, Cc, sizes):
        K = np.ascontiguousarray(K, np.float64).reshape(-1, 9); R = np.ascontiguousarray(R, np.float64).reshape(-1, 9); Cc = np.ascontiguousarray(Cc, np.float64).reshape(-1, 3)
        wh = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        if not (len(K) == len(R) == len(Cc) == len(wh)):
            raise ValueError("one K, R, C and (w, h) per view")
        return K, R, Cc, wh

    def mesh_project(self, K, R, Cc, sizes, normals=True):
        """`views.project_mesh` of the resident mesh for many views in one call (pmhip_mesh_project): K, R (n, 3, 3), Cc (n, 3), sizes n x (w, h).  `normals`: a bool, or
        one per view.  Returns [(depth (h, w), normal (h, w, 3) | None)] per view."""
        K, R, Cc, wh = self._mesh_views(K, R, Cc, sizes)
        n = len(wh)
        want = [bool(normals)] * n if np.isscalar(normals) else [bool(v) for v in normals]
        ok = bool((wh > 0).all())                 # (a refused size reaches the library, which says why; no array is made for it)
        depth = [np.zeros((h, w) if ok else (1, 1), np.float32) for w, h in wh]
        normal = [np.zeros((h, w, 3) if ok else (1, 1, 3), np.float32) if want[i] else None for i, (w, h) in enumerate(wh)]
        fp = C.POINTER(C.c_float)
        dp = (fp * max(n, 1))(*[a.ctypes.data_as(fp) for a in depth])
        np_ = (fp * max(n, 1))(*[fp() if a is None else a.ctypes.data_as(fp) for a in normal])
        self._chk(self._lib.pmhip_mesh_project(self._h, n, K, R, Cc, wh, dp, np_ if any(want) else None))
        return list(zip(depth, normal))

    def mesh_visibility(self, K, R, Cc, sizes, n_vertices, th_front_depth=0.985):
        """The visibility test of `views.sample_mesh_with_visibility` for every (vertex, view) on the device (pmhip_mesh_visibility) -> (n_vertices, n_views) bool."""
        K, R, Cc, wh = self._mesh_views(K, R, Cc, sizes)
        n = len(wh)
        words = (n + 31) // 32
        bits = np.zeros((int(n_vertices), max(words, 1)), np.uint32)
        self._chk(self._lib.pmhip_mesh_visibility(self._h, n, K, R, Cc, wh, bits, float(th_front_depth)))
        return ((bits[:, np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool) if n else np.zeros((int(n_vertices), 0), bool)

    def mesh_release(self):
        self._chk(self._lib.pmhip_mesh_release(self._h))

    def mesh_tuning(self, box_pixels=0, batch_bytes=0):
        """pmhip_mesh_set_tuning + pmhip_mesh_get_stats -> {batches, large_faces, device_us (of the last call), box_pixels, batch_bytes (in force)}; the results never
        depend on it."""
        self._chk(self._lib.pmhip_mesh_set_tuning(self._h, int(box_pixels), int(batch_bytes)))
        out = np.zeros(5, np.uint64)
        self._chk(self._lib.pmhip_mesh_get_stats(self._h, out))
        return dict(zip(("batches", "large_faces", "box_pixels", "batch_bytes", "device_us"), (int(v) for v in out)))

    # -- the seed maps of an image's sparse points (include/pmhip_seed.h) ------------------------
    @staticmethod
    def _seed_mesh(proj, z, normals, faces):
        P = np.ascontiguousarray(proj, np.float32).reshape(-1, 2)
        Z = np.ascontiguousarray(z, np.float32).ravel()
        N = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        F = np.zeros((0, 3), np.int64) if faces is None else np.asarray(faces).reshape(-1, 3)
        if len(Z) != len(P) or (N is not None and len(N) != len(P)):
            raise ValueError("one depth (and one normal) per projected vertex")
        if len(F) and (F.min() < 0 or F.max() > 0xFFFFFFFF):
            raise ValueError("face indices must be vertex indices")
        return P, Z, N, np.ascontiguousarray(F, np.uint32)

    def seed_raster(self, mode, w, h, proj, z, normals=None, faces=None):
        """The map part of `views.init_depth_map` / `views.triangulate_points_depth_map` on the device (pmhip_seed_raster), host arrays in and out; needs no scene.
        `mode`: SEED_POINTS (the 2x2 splats of bInitSparse) or SEED_FACES (the faces rasterised in the order given; the highest-numbered face that covers a pixel
        wins).  -> (depth (h, w), normal (h, w, 3) | None without `normals`), bit for bit the sequential walk."""
        P, Z, N, F = self._seed_mesh(proj, z, normals, faces)
        ok = int(w) > 0 and int(h) > 0 and int(w) * int(h) <= 0x7FFFFFFF     # (a refused size reaches the library, which says why; no array is made for it)
        d = np.zeros((int(h), int(w)) if ok else (1, 1), np.float32)
        n = None if N is None else np.zeros(d.shape + (3,), np.float32)
        self._chk(self._lib.pmhip_seed_raster(self._h, int(mode), int(w), int(h), P, Z, N, len(P), F, len(F), d, n))
        return d, n

    def scene_seed_view(self, idx, mode, proj, z, normals=None, faces=None):
        """`scene_set_maps(idx, *seed_raster(...))` with only the mesh crossing to the device (pmhip_scene_seed_view): the view's resident depth map, and with `normals`
        its normal map, at the view's own size."""
        P, Z, N, F = self._seed_mesh(proj, z, normals, faces)
        self._chk(self._lib.pmhip_scene_seed_view(self._h, int(idx), int(mode), P, Z, N, len(P), F, len(F)))

    def seed_set_tuning(self, box_pixels=0):
        """pmhip_seed_set_tuning: faces whose clipped box holds more pixels go to the workgroup route (0 keeps, < 0 restores the default); the maps never depend on it."""
        self._chk(self._lib.pmhip_seed_set_tuning(self._h, int(box_pixels)))

    def seed_stats(self):
        """pmhip_seed_get_stats -> {large_faces, device_us, mesh_bytes (of the last call), box_pixels (in force)}."""
        out = np.zeros(4, np.uint64)
        self._chk(self._lib.pmhip_seed_get_stats(self._h, out))
        return dict(zip(("large_faces", "box_pixels", "device_us", "mesh_bytes"), (int(v) for v in out)))

    # -- the reference's image and PLY outputs from the resident scene (include/pmhip_export.h) ----
    def x84_threshold(self, values, mul=5.2):
        """`mapexport.x84_threshold` on the device (pmhip_x84_threshold): (median, mul * MAD, min, max) of the values > 0 as float32; raises without one."""
        v = np.ascontiguousarray(values, np.float32).ravel()
        out = np.zeros(4, np.float32)
        self._chk(self._lib.pmhip_x84_threshold(self._h, v, v.size, float(mul), out))
        return tuple(out)

    @staticmethod
    def _range(min_depth, max_depth):
        auto = min_depth is None or max_depth is None
        return (float(np.finfo(np.float32).max), 0.0) if auto else (float(min_depth), float(max_depth))

    def scene_depth_image(self, idx, min_depth=None, max_depth=None):
        """`mapexport.depth_map_to_image` of a view's resident depth map (pmhip_scene_depth_image) -> ((h, w, 3) uint8 red first, (minDepth, maxDepth) in use)."""
        w, h = self.view_size(idx)
        rgb = np.zeros((h, w, 3), np.uint8); rng = np.zeros(2, np.float32)
        self._chk(self._lib.pmhip_scene_depth_image(self._h, idx, *self._range(min_depth, max_depth), rgb, rng))
        return rgb, (rng[0], rng[1])

    def depth_image(self, depth, min_depth=None, max_depth=None):
        """The same of a depth map on the host, a rendered mesh for one (pmhip_depth_image); needs no scene."""
        d = np.ascontiguousarray(depth, np.float32)
        if d.ndim != 2:
            raise ValueError("depth must be (h, w)")
        rgb = np.zeros(d.shape + (3,), np.uint8); rng = np.zeros(2, np.float32)
        self._chk(self._lib.pmhip_depth_image(self._h, d, d.shape[1], d.shape[0], *self._range(min_depth, max_depth), rgb, rng))
        return rgb, (rng[0], rng[1])

    def scene_normal_image(self, idx):
        """`mapexport.normal_map_to_image` of a view's resident normal map (pmhip_scene_normal_image) -> (h, w, 3) uint8."""
        w, h = self.view_size(idx)
        rgb = np.zeros((h, w, 3), np.uint8)
        self._chk(self._lib.pmhip_scene_normal_image(self._h, idx, rgb))
        return rgb

    def scene_conf_image(self, idx):
        """`mapexport.conf_map_to_image` of a view's resident confidence map (pmhip_scene_conf_image) -> ((h, w) uint8, (minConf, maxConf)), or None when no
        confidence is positive."""
        w, h = self.view_size(idx)
        gray = np.zeros((h, w), np.uint8); rng = np.zeros(2, np.float32); empty = C.c_int(0)
        self._chk(self._lib.pmhip_scene_conf_image(self._h, idx, gray, rng, C.byref(empty)))
        return None if empty.value else (gray, (rng[0], rng[1]))

    def scene_view_cloud(self, idx, with_normals=True, capacity=None):
        """`mapexport.view_point_cloud` of a view's resident maps and colour image (pmhip_scene_view_cloud): the records as `mapexport.VIEW_VERTEX_N` /
        `VIEW_VERTEX`.  `capacity` None: asked for first (two calls); a capacity that is too small raises, as the library refuses it."""
        from . import mapexport
        dt = mapexport.VIEW_VERTEX_N if with_normals else mapexport.VIEW_VERTEX
        cnt = C.c_uint64(0)
        if capacity is None:
            rc = self._lib.pmhip_scene_view_cloud(self._h, idx, bool(with_normals), None, 0, C.byref(cnt))
            if rc != 0 and cnt.value == 0:
                self._chk(rc)
            capacity = cnt.value
        rec = np.zeros(int(capacity), dt)
        self._chk(self._lib.pmhip_scene_view_cloud(self._h, idx, bool(with_normals), rec if capacity else None, int(capacity), C.byref(cnt)))
        return rec[:cnt.value]

    def scene_cloud_scale(self, scale_mult=1.0):
        """`mapexport.point_scales` of the resident cloud with the scene's cameras (pmhip_scene_cloud_scale) -> (scale, confidence), float32 per point."""
        nP = C.c_uint64()
        self._chk(self._lib.pmhip_scene_cloud_finish(self._h, C.byref(PMHipCloudParams()), C.byref(nP), None))
        scale = np.zeros(int(nP.value), np.float32); conf = np.zeros(int(nP.value), np.float32)
        self._chk(self._lib.pmhip_scene_cloud_scale(self._h, float(scale_mult), scale, conf))
        return scale, conf

    def export_stats(self):
        """pmhip_export_get_stats -> {quantum, grid_cap, scan_tile (work quanta in force), launches, device_us (of the last export call: kernels and download, by HIP events)}."""
        out = np.zeros(8, np.uint64)
        self._chk(self._lib.pmhip_export_get_stats(self._h, out))
        return dict(zip(("quantum", "grid_cap", "scan_tile", "launches", "device_us"), (int(v) for v in out)))

    def scene_set_color(self, idx, bgr):
        """8-bit BGR image of a view at depth-map resolution (only fusion with bEstimateColor reads it)."""
        b = np.ascontiguousarray(bgr, np.uint8)
        w, h = self.view_size(idx)
        if b.shape != (h, w, 3):
            raise ValueError("bgr must be (h, w, 3) uint8")
        self._chk(self._lib.pmhip_scene_set_color(self._h, idx, b))

    def scene_fuse(self, order, nMinViewsFuse=2, fDepthDiffThreshold=0.01, fNormalDiffThreshold=25.0, bEstimateColor=True, bEstimateNormal=True):
        """DepthMapsData::FuseDepthMaps over the resident maps (libs/MVS/SceneDensify.cpp:1372-1650); `order` = views, best connected
        first.  Returns a dict with the fields of MVS::PointCloud: points, viewStart/views/weights (CSR), projs, colors (BGR), normals."""
        od = np.ascontiguousarray(order, np.int32)
        prm = PMHipFuseParams(nMinViewsFuse, fDepthDiffThreshold, fNormalDiffThreshold, bool(bEstimateColor), bool(bEstimateNormal))
        nP, nV, nD = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.pmhip_scene_fuse(self._h, od, len(od), C.byref(prm), C.byref(nP), C.byref(nV), C.byref(nD)))
        P, V = int(nP.value), int(nV.value)
        pts = np.zeros((P, 3), np.float32); vs = np.zeros(P + 1, np.uint32); views = np.zeros(V, np.uint32); wts = np.zeros(V, np.float32)
        projs = np.zeros((V, 2), np.uint16)
        cols = np.zeros((P, 3), np.uint8) if bEstimateColor else None
        nrm = np.zeros((P, 3), np.float32) if bEstimateNormal else None
        self._chk(self._lib.pmhip_scene_fuse_get(self._h, pts, vs, views, wts, projs, cols, nrm))
        return dict(nPoints=P, nDepths=int(nD.value), points=pts, viewStart=vs, views=views, weights=wts, projs=projs, colors=cols, normals=nrm,
                    rounds=int(self._lib.pmhip_scene_fuse_rounds(self._h)))

    def scene_cloud_get(self):
        """The resident cloud (after scene_fuse, scene_cloud_set or scene_cloud_finish) in the layout of scene_fuse's result; colors / normals are None when the
        cloud has none."""
        nP, nV = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.pmhip_scene_cloud_finish(self._h, C.byref(PMHipCloudParams()), C.byref(nP), C.byref(nV)))
        P, V = int(nP.value), int(nV.value)
        pts = np.zeros((P, 3), np.float32); vs = np.zeros(P + 1, np.uint32); views = np.zeros(V, np.uint32); wts = np.zeros(V, np.float32)
        projs = np.zeros((V, 2), np.uint16)
        self._chk(self._lib.pmhip_scene_fuse_get(self._h, pts, vs, views, wts, projs, None, None))
        cols = np.zeros((P, 3), np.uint8); nrm = np.zeros((P, 3), np.float32)
        if self._lib.pmhip_scene_fuse_get(self._h, None, None, None, None, None, cols, None) != 0:
            cols = None
        if self._lib.pmhip_scene_fuse_get(self._h, None, None, None, None, None, None, nrm) != 0:
            nrm = None
        return dict(nPoints=P, points=pts, viewStart=vs, views=views, weights=wts, projs=projs, colors=cols, normals=nrm)

    def scene_cloud_finish(self, crop_obb=None, border_roi=0.0, estimate_colors=False, estimate_normals=False, n_neighbors=16):
        """The last block of Scene::DenseReconstruction on the resident cloud (pmhip_scene_cloud_finish): crop to `crop_obb` = (rot 3x3, pos 3, ext 3) of
        TOBB<float,3> (None: no crop) enlarged by `border_roi`, then colours and PCA normals (each only if the cloud has none).  Returns scene_cloud_get()
        plus the step times in ms (`times`: crop, grid, knn_pca, colors)."""
        prm = PMHipCloudParams()
        if crop_obb is not None:
            rot, pos, ext = crop_obb
            prm.bCrop = 1
            prm.obbRot[:] = [float(v) for v in np.asarray(rot, np.float32).ravel()]
            prm.obbPos[:] = [float(v) for v in np.asarray(pos, np.float32).ravel()]
            prm.obbExt[:] = [float(v) for v in np.asarray(ext, np.float32).ravel()]
        prm.fBorderROI = float(border_roi)
        prm.bEstimateColor = bool(estimate_colors)
        prm.bEstimateNormal = bool(estimate_normals)
        prm.nNeighbors = int(n_neighbors)
        self._chk(self._lib.pmhip_scene_cloud_finish(self._h, C.byref(prm), None, None))
        t = (C.c_double * 4)()
        self._chk(self._lib.pmhip_scene_cloud_times(self._h, t))
        out = self.scene_cloud_get()
        out["times"] = dict(crop=t[0], grid=t[1], knn_pca=t[2], colors=t[3])
        return out

    def scene_cloud_set(self, points, viewStart, views, weights=None):
        """Replace the resident cloud (pmhip_scene_cloud_set); views are image indices of the loaded scene."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        vs = np.ascontiguousarray(viewStart, np.uint32); vv = np.ascontiguousarray(views, np.uint32)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        if len(vs) != len(pts) + 1:
            raise ValueError("viewStart must have nPoints + 1 entries")
        self._chk(self._lib.pmhip_scene_cloud_set(self._h, pts, vs, vv, w, len(pts)))

    def scene_cloud_load(self, points, viewStart, views, weights=None, colors=None, normals=None, n_cams=0):
        """Replace the resident cloud, colours (BGR bytes) and normals included when given (pmhip_scene_cloud_load).  `n_cams` > 0: the number of cameras the
        view indices refer to, for an engine that holds no scene (an archive's cloud); 0: the loaded scene's images."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        vs = np.ascontiguousarray(viewStart, np.uint32); vv = np.ascontiguousarray(views, np.uint32)
        if len(vs) != len(pts) + 1:
            raise ValueError("viewStart must have nPoints + 1 entries")
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if (w is not None and len(w) != len(vv)) or (col is not None and len(col) != len(pts)) or (nrm is not None and len(nrm) != len(pts)):
            raise ValueError("weights go with the views, colours and normals with the points")
        self._chk(self._lib.pmhip_scene_cloud_load(self._h, pts, vs, vv, w, col, nrm, len(pts), n_cams))

    def scene_cloud_filter(self, th_remove=None, min_views=0, cam_C=None, cam_angle=None):
        """Scene::PointCloudFilter(th_remove) (--filter-point-cloud) on the resident cloud, after PointCloud::RemoveMinViews(min_views) when `min_views` > 0
        (pmhip_scene_cloud_filter); `th_remove` None: no visibility filter.  `cam_C` (n, 3) / `cam_angle` (n,): the camera centres and cone half-angles in
        radians (FOV / width) -- both or neither; without them the loaded scene's cameras.  Returns scene_cloud_get() plus `visibility` (int32 per point of the
        cloud the vote ran on, None without one), `cones` ((n, 2): angle, cosAngleSq as used, or None), `times` in ms (binning, cones, removal) and the
        diagnostics `n_cones` / `n_candidates` (cones formed, candidates classified)."""
        prm = PMHipCloudFilterParams()
        prm.bVisibility = 0 if th_remove is None else 1
        prm.thRemove = 0 if th_remove is None else int(th_remove)
        prm.nMinViews = int(min_views)
        if (cam_C is None) != (cam_angle is None):
            raise ValueError("cam_C and cam_angle go together")
        keep = None
        if cam_C is not None:
            cc = np.ascontiguousarray(cam_C, np.float64).reshape(-1, 3); ca = np.ascontiguousarray(cam_angle, np.float32).ravel()
            if len(cc) != len(ca):
                raise ValueError("cam_C and cam_angle must have one entry per camera")
            keep = (cc, ca)
            prm.nCams = len(ca); prm.camC = cc.ctypes.data_as(C.POINTER(C.c_double)); prm.camAngle = ca.ctypes.data_as(C.POINTER(C.c_float))
        n_cams = prm.nCams if cam_C is not None else (self._scene or (0,))[0]
        # two calls when both are asked for: the size of the cloud between them is the size of `visibility`
        before = C.c_uint64(); t = (C.c_double * 3)(); t_min = 0.0
        if prm.nMinViews and prm.bVisibility:
            only = PMHipCloudFilterParams(); only.nMinViews = prm.nMinViews
            self._chk(self._lib.pmhip_scene_cloud_filter(self._h, C.byref(only), None, None))
            self._chk(self._lib.pmhip_scene_cloud_filter_times(self._h, t))
            t_min = t[2]; prm.nMinViews = 0
        self._chk(self._lib.pmhip_scene_cloud_finish(self._h, C.byref(PMHipCloudParams()), C.byref(before), None))
        self._chk(self._lib.pmhip_scene_cloud_filter(self._h, C.byref(prm), None, None))
        del keep
        out = self.scene_cloud_get()
        self._chk(self._lib.pmhip_scene_cloud_filter_times(self._h, t))
        out["times"] = dict(binning=t[0], cones=t[1], removal=t[2] + t_min)
        cnt = (C.c_uint64 * 2)()
        self._chk(self._lib.pmhip_scene_cloud_filter_counts(self._h, cnt))
        out["n_cones"], out["n_candidates"] = int(cnt[0]), int(cnt[1])
        out["visibility"] = None; out["cones"] = None
        if th_remove is not None and int(before.value) > 0:
            cones = np.zeros((n_cams, 2), np.float32)
            self._chk(self._lib.pmhip_scene_cloud_filter_cones(self._h, cones))
            vis = np.zeros(int(before.value), np.int32)
            self._chk(self._lib.pmhip_scene_cloud_visibility(self._h, vis, len(vis)))
            out["cones"] = cones; out["visibility"] = vis
        return out

    def scene_cloud_knn(self, queries, k=16):
        """The k nearest points of the resident cloud for each query index, nearest first (pmhip_scene_cloud_knn): (nq, k) uint32."""
        q = np.ascontiguousarray(queries, np.uint32)
        out = np.zeros((len(q), int(k)), np.uint32)
        self._chk(self._lib.pmhip_scene_cloud_knn(self._h, k, q, len(q), out))
        return out

    def scene_copy(self, what, first, count, device_ptr, to_engine):
        self._chk(self._lib.pmhip_scene_copy(self._h, what, first, count, device_ptr, bool(to_engine)))

    def scene_images_updated(self):
        self._chk(self._lib.pmhip_scene_images_updated(self._h))

    def scene_maps_updated(self, first, count):
        """Depth maps of these views were written through scene_device_ptr(1, ...): see include/pmhip.h."""
        self._chk(self._lib.pmhip_scene_maps_updated(self._h, first, count))

    def sync(self):
        self._chk(self._lib.pmhip_sync(self._h))

    def scene_bytes(self) -> int:
        """Device memory the resident scene holds right now (pmhip_scene_bytes)."""
        return int(self._lib.pmhip_scene_bytes(self._h))

    def stream(self) -> int:
        return int(self._lib.pmhip_stream(self._h) or 0)

    def stats_reset(self, enable=True):
        self._chk(self._lib.pmhip_stats_reset(self._h, bool(enable)))

    def stats_get(self) -> PMHipKernelStats:
        s = PMHipKernelStats()
        self._chk(self._lib.pmhip_stats_get(self._h, C.byref(s)))
        return s

    def prof_get(self, reset=True):
        out = (C.c_ulonglong * 16)()
        self._chk(self._lib.pmhip_prof_get(self._h, out, bool(reset)))
        return list(out)

    # -- self-test hooks -----------------------------------------------------------------------
    def math_eval(self, kind, a, b=None):
        a = np.ascontiguousarray(a, np.float32); b = a if b is None else np.ascontiguousarray(b, np.float32)
        o = np.zeros_like(a)
        self._chk(self._lib.pmhip_math_eval(self._h, kind, a, b, o, a.size))
        return o

    def resize(self, kind, img, arg=2):
        img = np.ascontiguousarray(img, np.float32); h, w = img.shape
        o = np.zeros((int(np.rint(h / arg)), int(np.rint(w / arg))) if kind == 0 else (h * 2, w * 2), np.float32)
        self._chk(self._lib.pmhip_resize(self._h, kind, img, w, h, arg, o))
        return o

    RESAMPLE_AREA, RESAMPLE_UPSAMPLE, RESAMPLE_NEAREST_DOWN, RESAMPLE_NEAREST_UP, RESAMPLE_MASK_LEVEL, RESAMPLE_SKEW, RESAMPLE_QUAD, RESAMPLE_DEPTH_QUADS = range(8)

    def resample(self, kind, src, src_size, dst, dst_size, arg=0, n_img=1):
        """pmhip_resample: one resampler of csrc/pm_kernels.hip through production's launch, `src_size` = (sw, sh) -> `dst_size` = (dw, dh).  `src` and `dst` are flat
        C-contiguous buffers laid out as include/pmhip.h says for the kind (uint8 for the mask level, float32 otherwise); `dst` is uploaded first and written in place, so
        what the kernel leaves alone keeps the caller's fill.  Returns `dst`."""
        u8 = kind == self.RESAMPLE_MASK_LEVEL
        dt = np.uint8 if u8 else np.float32
        (sw, sh), (dw, dh) = src_size, dst_size
        ps, pd = sw * sh, dw * dh
        ns, nd = {self.RESAMPLE_UPSAMPLE: (4 * ps, 5 * pd), self.RESAMPLE_NEAREST_DOWN: (4 * ps, 4 * pd),
                  self.RESAMPLE_QUAD: (ps * n_img, (dw + dh - 1) * dh * 4 * n_img), self.RESAMPLE_DEPTH_QUADS: (ps, pd * 4)}.get(kind, (ps * n_img, pd * n_img))
        if not (isinstance(dst, np.ndarray) and dst.dtype == dt and dst.flags.c_contiguous and dst.flags.writeable and dst.size == nd):
            raise ValueError("resample: dst must be a writable C-contiguous %s array of %d elements" % (np.dtype(dt).name, nd))
        src = np.ascontiguousarray(src, dt)
        if src.size != ns:
            raise ValueError("resample: src must hold %d elements" % ns)
        self._chk(self._lib.pmhip_resample(self._h, kind, src, sw, sh, dst, dw, dh, arg, n_img))
        return dst

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pmhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
