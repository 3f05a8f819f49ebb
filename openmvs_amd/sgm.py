"""ctypes binding of libsgmhip.so: host-side mirror of SemiGlobalMatcher::Match(ViewData, ViewData,
DisparityMap&, AccumCostMap&) (libs/MVS/SemiGlobalMatcher.cpp:863-1302).  No CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _cabi, build as _build

PIXEL_DTYPE = np.dtype([("idx", np.uint64), ("minDisp", np.int16), ("maxDisp", np.int16), ("pad_", np.int32)])       # SGMHipPixelData
NO_DISP = 32767          # SemiGlobalMatcher::NO_DISP
INVALID, VALID = 0, 255  # MaskMap values
SUBPIXEL_NA, SUBPIXEL_LINEAR, SUBPIXEL_POLY4, SUBPIXEL_PARABOLA, SUBPIXEL_SINE, SUBPIXEL_COSINE, SUBPIXEL_LC_BLEND = range(7)


class SGMHipStats(C.Structure):
    _fields_ = [("costMs", C.c_double), ("aggrMs", C.c_double), ("wtaMs", C.c_double), ("calls", C.c_uint64), ("aggrLaunches", C.c_uint64)]


_TYPES = {"SGMHipPixelData": PIXEL_DTYPE, "SGMHipStats": SGMHipStats}          # the mirrors by their names in include/sgmhip.h
_SIGNATURES = _cabi.signatures("sgmhip.h", _TYPES)
EXPORTS = list(_SIGNATURES)          # every function include/sgmhip.h declares
_PLAIN_SIGNATURES = _cabi.signatures("sgmhip_plain.h", _TYPES)          # ... and its companion header, which sgmhip.h includes
PLAIN_EXPORTS = list(_PLAIN_SIGNATURES)
_SEED_SIGNATURES = _cabi.signatures("sgmhip_seed.h", _TYPES)
SEED_EXPORTS = list(_SEED_SIGNATURES)
_LIB = None


def load_library() -> C.CDLL:
    global _LIB
    if _LIB is None:
        path = os.environ.get("SGMHIP_LIB") or _build.build_lib("libsgmhip.so")
        if path is None or not os.path.exists(path):
            raise RuntimeError("libsgmhip.so is not built (python -m openmvs_amd.build)")
        lib = C.CDLL(path)
        if hasattr(lib, "hipemu_counters") and os.environ.get("OPENMVS_AMD_TEST_EMULATOR") != "1":
            # tests/cpp/hipemu builds of the kernels exist for the CPU test-suite only; the product never computes on the host
            raise RuntimeError("%s is a CPU-emulated test build, not a device library: refusing to load it outside the test-suite" % path)
        _LIB = _cabi.declare(_cabi.declare(_cabi.declare(lib, _SIGNATURES), _PLAIN_SIGNATURES), _SEED_SIGNATURES)
    return _LIB


def generate_p2s(P2=4, alpha=14.0, beta=38.0) -> np.ndarray:
    """SemiGlobalMatcher::GenerateP2s with the ctor defaults (SemiGlobalMatcher.h:151)."""
    out = np.zeros(256, np.uint16)
    load_library().sgmhip_generate_p2s(P2, alpha, beta, out)
    return out


def make_pixels(ranges_min: np.ndarray, ranges_max: np.ndarray):
    """Build the PixelData table (SemiGlobalMatcher.h:79-82) for a valid grid: idx = running sum of numDisp."""
    mn = np.ascontiguousarray(ranges_min, np.int16); mx = np.ascontiguousarray(ranges_max, np.int16)
    nd = np.maximum(mx.astype(np.int64) - mn.astype(np.int64), 0).ravel()
    idx = np.concatenate([[0], np.cumsum(nd)[:-1]]).astype(np.uint64)
    px = np.zeros(nd.size, PIXEL_DTYPE)
    px["idx"] = idx; px["minDisp"] = mn.ravel(); px["maxDisp"] = mx.ravel()
    return px, int(nd.sum()), int(nd.max())


class SGMError(RuntimeError):
    pass


MAX_UNIFORM_DISP = 1024      # SGMHIP_MAX_UNIFORM_DISP


def plain_range(seed):
    """sgmhip_plain_range: the global range of plain SGM from the seed disparity map (host code of the library; no engine needed)."""
    a = np.ascontiguousarray(seed, np.int16)
    mn = C.c_int16(0); mx = C.c_int16(0)
    if load_library().sgmhip_plain_range(a, a.size, C.byref(mn), C.byref(mx)) != 0:
        raise SGMError("plain_range: the seed map is empty")
    return int(mn.value), int(mx.value)


class SemiGlobalMatcherHIP:
    def __init__(self, device: int = 0, P1: int = 3, P2: int = 4, P2alpha: float = 14.0, P2beta: float = 38.0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.sgmhip_create(device, C.byref(self._h))
        if rc != 0:
            raise SGMError(f"sgmhip_create failed ({rc}): no usable HIP device")
        self.P1 = P1
        self.P2s = generate_p2s(P2, P2alpha, P2beta)
        self.image_uploads = 0        # images sent to the device by scene_set_images since the engine was created
        self._rect_shape = None

    def _chk(self, rc):
        if rc != 0:
            raise SGMError(f"sgmhip error {rc}: {self._lib.sgmhip_last_error(self._h).decode()}")

    def set_problem(self, left_bgr, left_gray, right_gray, pixels, num_costs, max_num_disp):
        lb = np.ascontiguousarray(left_bgr, np.uint8); lg = np.ascontiguousarray(left_gray, np.float32); rg = np.ascontiguousarray(right_gray, np.float32)
        h, w = lg.shape
        px = np.ascontiguousarray(pixels)
        assert px.dtype == PIXEL_DTYPE and px.size == (w - 6) * (h - 6)
        self._shape = (h - 6, w - 6); self._num = num_costs
        self._chk(self._lib.sgmhip_set_problem(self._h, lb, lg, rg, w, h, px, num_costs, max_num_disp))

    def set_problem_uniform(self, left_bgr, left_gray, right_gray, min_disp, max_disp):
        """The problem of one range [min_disp, max_disp) for every pixel, idx = pixel * D, D <= MAX_UNIFORM_DISP: no pixel table travels
        (sgmhip_set_problem_uniform); Match, results, set_disparity and RefineDisparityMap work on it as on any other."""
        lb = np.ascontiguousarray(left_bgr, np.uint8); lg = np.ascontiguousarray(left_gray, np.float32); rg = np.ascontiguousarray(right_gray, np.float32)
        h, w = lg.shape
        assert lb.shape == (h, w, 3) and rg.shape == (h, w)
        self._chk(self._lib.sgmhip_set_problem_uniform(self._h, lb, lg, rg, w, h, int(min_disp), int(max_disp)))
        self._shape = (h - 6, w - 6); self._num = (h - 6) * (w - 6) * (int(max_disp) - int(min_disp))

    def plain_range(self, seed):
        """-> (minDisp, maxDisp) of plain SGM from the half-resolution seed map (sgmhip_plain_range: the reference's int16 arithmetic, wraps included)."""
        return plain_range(seed)

    def set_sub_group_kernels(self, lanes):
        """Match with sub-groups of `lanes` (8, 16, 32; True = 16) lanes per pixel / pair / line (narrow tSGM ranges) instead of one wavefront each
        (False / 0); same results."""
        self._chk(self._lib.sgmhip_set_sub_group_kernels(self._h, 16 if lanes is True else int(lanes)))

    def Match(self, sync=True):
        self._chk(self._lib.sgmhip_match(self._h, self.P1, self.P2s, bool(sync)))

    def results(self, volumes=False):
        d = np.zeros(self._shape, np.int16); c = np.zeros(self._shape, np.uint16)
        costs = np.zeros(self._num, np.uint8) if volumes else None
        acc = np.zeros(self._num, np.uint16) if volumes else None
        self._chk(self._lib.sgmhip_get_results(self._h, d, c, costs, acc))
        return (d, c, costs, acc) if volumes else (d, c)

    # ---- the tSGM steps around Match (libs/MVS/SemiGlobalMatcher.cpp:1449-1811) -------------------------------------------
    def ConsistencyCrossCheck(self, l2r, r2l, thCross=1):
        a = np.ascontiguousarray(l2r, np.int16).copy(); b = np.ascontiguousarray(r2l, np.int16)
        self._chk(self._lib.sgmhip_consistency_cross_check(self._h, a, b, a.shape[1], a.shape[0], b.shape[1], thCross))
        return a

    def FilterByCost(self, disparity, cost, th):
        a = np.ascontiguousarray(disparity, np.int16).copy(); c = np.ascontiguousarray(cost, np.uint16)
        self._chk(self._lib.sgmhip_filter_by_cost(self._h, a, c, a.shape[1], a.shape[0], th))
        return a

    def ExtractMask(self, disparity, mask=None, thValid=3):
        a = np.ascontiguousarray(disparity, np.int16)
        m = np.zeros(a.shape, np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8).copy()
        self._chk(self._lib.sgmhip_extract_mask(self._h, a, m, a.shape[1], a.shape[0], thValid, mask is None))
        return m

    def UpscaleMask(self, mask, size2x):
        m = np.ascontiguousarray(mask, np.uint8); w2, h2 = size2x
        o = np.zeros((h2, w2), np.uint8)
        self._chk(self._lib.sgmhip_upscale_mask(self._h, m, m.shape[1], m.shape[0], o, w2, h2))
        return o

    def FlipDirection(self, l2r):
        a = np.ascontiguousarray(l2r, np.int16); o = np.zeros_like(a)
        self._chk(self._lib.sgmhip_flip_direction(self._h, a, a.shape[1], a.shape[0], o))
        return o

    def set_disparity(self, disparity):
        a = np.ascontiguousarray(disparity, np.int16)
        assert a.shape == self._shape
        self._chk(self._lib.sgmhip_set_disparity(self._h, a))

    def RefineDisparityMap(self, subpixelMode=SUBPIXEL_LC_BLEND, subpixelSteps=4):
        """In place on the device, on the result of the last Match(); read it back with results()."""
        self._chk(self._lib.sgmhip_refine_disparity(self._h, subpixelMode, subpixelSteps))

    def Disparity2RangeMap(self, disparity, mask2x, minNumDisp=5, minNumDispInvalid=7):
        """-> (pixel table of the 2x level, numCosts, maxNumDisp), ready for set_problem."""
        a = np.ascontiguousarray(disparity, np.int16); m = np.ascontiguousarray(mask2x, np.uint8)
        px = np.zeros(m.size, PIXEL_DTYPE); n = C.c_uint64(0); mx = C.c_int(0)
        self._chk(self._lib.sgmhip_disparity2range_map(self._h, a, a.shape[1], a.shape[0], m, m.shape[1], m.shape[0], minNumDisp, minNumDispInvalid, px, C.byref(n), C.byref(mx)))
        return px, int(n.value), int(mx.value)

    def Depth2DisparityMap(self, depth, invH, invQ, subpixelSteps, size):
        d = np.ascontiguousarray(depth, np.float32); w, h = size
        o = np.zeros((h, w), np.int16)
        ih = np.ascontiguousarray(invH, np.float64); iq = np.ascontiguousarray(invQ, np.float64)
        self._chk(self._lib.sgmhip_depth2disparity_map(self._h, d, d.shape[1], d.shape[0], ih, iq, subpixelSteps, o, w, h))
        return o

    def Disparity2DepthMap(self, disparity, cost, H, Q, subpixelSteps, size):
        a = np.ascontiguousarray(disparity, np.int16); c = None if cost is None else np.ascontiguousarray(cost, np.uint16); dw, dh = size
        dep = np.zeros((dh, dw), np.float32); cf = np.zeros((dh, dw), np.float32)
        hh = np.ascontiguousarray(H, np.float64); qq = np.ascontiguousarray(Q, np.float64)
        self._chk(self._lib.sgmhip_disparity2depth_map(self._h, a, c, a.shape[1], a.shape[0], hh, qq, subpixelSteps, dep, cf, dw, dh))
        return dep, (None if c is None else cf)

    def ProjectDisparity2DepthMap(self, disparity, cost, Q, subpixelSteps, size):
        """-> (any depth produced, depthMap, depthRangeMap (h, w, 2), confMap or None)"""
        a = np.ascontiguousarray(disparity, np.int16); c = None if cost is None else np.ascontiguousarray(cost, np.uint16); dw, dh = size
        dep = np.zeros((dh, dw), np.float32); rg = np.zeros((dh, dw, 2), np.float32); cf = np.zeros((dh, dw), np.float32); anyd = C.c_int(0)
        qq = np.ascontiguousarray(Q, np.float64)
        self._chk(self._lib.sgmhip_project_disparity2depth_map(self._h, a, c, a.shape[1], a.shape[0], qq, subpixelSteps, dep, rg, None if c is None else cf, dw, dh, C.byref(anyd)))
        return bool(anyd.value), dep, rg, (None if c is None else cf)

    def FusePairs(self, depths, ranges, confs, minViews=2):
        """The per-pixel cluster fusion of SemiGlobalMatcher::Fuse over the maps of ProjectDisparity2DepthMap."""
        dh, dw = depths[0].shape
        keep = [[np.ascontiguousarray(a, np.float32) for a in arrs] for arrs in (depths, ranges, confs)]
        ptrs = [(C.POINTER(C.c_float) * len(k))(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in k]) for k in keep]
        dep = np.zeros((dh, dw), np.float32); cf = np.zeros((dh, dw), np.float32)
        self._chk(self._lib.sgmhip_fuse_pairs(self._h, ptrs[0], ptrs[1], ptrs[2], len(depths), dw, dh, minViews, dep, cf))
        return dep, cf

    def tsgm_match(self, left_bgr, right_bgr, left_gray, right_gray, left_mask, right_mask, min_resolution=320, init_left_disparity=None,
                   n_speckle_size=100, subpixel_mode=SUBPIXEL_LC_BLEND, subpixel_steps=4):
        """The whole coarse-to-fine loop for a rectified pair in one call, resident on the device (sgmhip_tsgm_match; the same result as
        openmvs_amd.tsgm.tsgm_match driving the steps).  -> (disparity, cost, levels) on the valid grid."""
        lb = np.ascontiguousarray(left_bgr, np.uint8); rb = np.ascontiguousarray(right_bgr, np.uint8)
        lg = np.ascontiguousarray(left_gray, np.float32); rg = np.ascontiguousarray(right_gray, np.float32)
        lm = np.ascontiguousarray(left_mask, np.uint8); rm = np.ascontiguousarray(right_mask, np.uint8)
        h, w = lg.shape
        assert lb.shape == (h, w, 3) and rb.shape == (h, w, 3) and rg.shape == (h, w) and lm.shape == (h, w) and rm.shape == (h, w)
        init = None if init_left_disparity is None else np.ascontiguousarray(init_left_disparity, np.int16)
        d = np.zeros((h - 6, w - 6), np.int16); c = np.zeros((h - 6, w - 6), np.uint16); lv = C.c_int(0)
        self._chk(self._lib.sgmhip_tsgm_match(self._h, lb, rb, lg, rg, lm, rm, w, h, min_resolution, init, n_speckle_size, subpixel_mode, subpixel_steps,
                                              self.P1, self.P2s, d, c, C.byref(lv)))
        self._shape = d.shape
        return d, c, int(lv.value)

    # ---- the resident scene: images uploaded once, pairs rectified on the device ------------------------------------------------------------
    def scene_set_images(self, images):
        """Replace the resident scene by `images` ((h, w, 3) uint8 BGR, each with its own size; None leaves a slot unset): one upload per image."""
        images = list(images)
        self._rect_shape = None
        self._chk(self._lib.sgmhip_scene_create(self._h, len(images)))
        for i, im in enumerate(images):
            if im is None:
                continue
            a = np.ascontiguousarray(im, np.uint8)
            assert a.ndim == 3 and a.shape[2] == 3
            self._chk(self._lib.sgmhip_scene_set_image(self._h, i, a, a.shape[1], a.shape[0]))
            self.image_uploads += 1

    def scene_clear(self):
        self._rect_shape = None
        self._chk(self._lib.sgmhip_scene_clear(self._h))

    def rectify_pair(self, idx_left, idx_right, inv_h1, inv_h2, size, srgb2lin):
        """Warp images idx_left / idx_right of the resident scene by the inverse homographies inv_h1 / inv_h2 into size = (w, h), with their linear gray
        images and validity masks (sgmhip_rectify_pair: rectify.warp_perspective_u8 + sgm_pipeline.to_gray_linear, bit for bit).  The results stay on
        the device for `tsgm_match_rectified` / `rectified`."""
        a = np.ascontiguousarray(inv_h1, np.float64); b = np.ascontiguousarray(inv_h2, np.float64); t = np.ascontiguousarray(srgb2lin, np.float32)
        assert a.shape == (3, 3) and b.shape == (3, 3) and t.shape == (256,)
        w, h = int(size[0]), int(size[1])
        self._chk(self._lib.sgmhip_rectify_pair(self._h, idx_left, idx_right, a, b, w, h, t))
        self._rect_shape = (h, w)

    def rectified(self, side, bgr=True, gray=True, mask=True):
        """-> (bgr, gray, mask) of the resident rectified image of `side` (0 left, 1 right); None for what was not asked."""
        if self._rect_shape is None:
            self._chk(self._lib.sgmhip_rectified_get(self._h, side, None, None, None))      # the library's own error
        h, w = self._rect_shape or (0, 0)
        b = np.zeros((h, w, 3), np.uint8) if bgr else None; g = np.zeros((h, w), np.float32) if gray else None; m = np.zeros((h, w), np.uint8) if mask else None
        self._chk(self._lib.sgmhip_rectified_get(self._h, side, b, g, m))
        return b, g, m

    def tsgm_match_rectified(self, min_resolution=320, init_left_disparity=None, n_speckle_size=100, subpixel_mode=SUBPIXEL_LC_BLEND, subpixel_steps=4, seeded=False):
        """`tsgm_match` on the resident rectified pair of the last `rectify_pair`.  -> (disparity, cost, levels) on the valid grid.
        `seeded`: the initial left disparity is the resident one of the last `seed_disparity` (sgmhip_tsgm_match_rectified_seeded) and `init_left_disparity` must be None."""
        h, w = self._rect_shape or (6, 6)              # (without a pair the library refuses the call)
        d = np.zeros((h - 6, w - 6), np.int16); c = np.zeros((h - 6, w - 6), np.uint16); lv = C.c_int(0)
        if seeded:
            if init_left_disparity is not None:
                raise ValueError("seeded=True reads the resident seed disparity; init_left_disparity must be None")
            self._chk(self._lib.sgmhip_tsgm_match_rectified_seeded(self._h, min_resolution, n_speckle_size, subpixel_mode, subpixel_steps, self.P1, self.P2s, d, c, C.byref(lv)))
            self._shape = d.shape
            return d, c, int(lv.value)
        init = None if init_left_disparity is None else np.ascontiguousarray(init_left_disparity, np.int16)
        self._chk(self._lib.sgmhip_tsgm_match_rectified(self._h, min_resolution, init, n_speckle_size, subpixel_mode, subpixel_steps, self.P1, self.P2s, d, c, C.byref(lv)))
        self._shape = d.shape
        return d, c, int(lv.value)

    # -- the loop's seed made and kept on the device (include/sgmhip_seed.h) -------------------
    def seed_raster(self, w, h, proj, z, faces, download=True):
        """The depth-only `views.triangulate_points_depth_map` from its mesh on the device (sgmhip_seed_raster): the faces rasterised in the order given into a
        (h, w) depth map that stays resident as the seed.  -> the map, or None without `download`."""
        P = np.ascontiguousarray(proj, np.float32).reshape(-1, 2); Z = np.ascontiguousarray(z, np.float32).ravel()
        F = np.asarray(faces).reshape(-1, 3)
        if len(Z) != len(P):
            raise ValueError("one depth per projected vertex")
        if len(F) and (F.min() < 0 or F.max() > 0xFFFFFFFF):
            raise ValueError("face indices must be vertex indices")
        F = np.ascontiguousarray(F, np.uint32)
        ok = int(w) > 0 and int(h) > 0 and int(w) * int(h) <= 0x7FFFFFFF     # (a refused size reaches the library, which says why)
        out = np.zeros((int(h), int(w)) if ok else (1, 1), np.float32) if download else None
        self._chk(self._lib.sgmhip_seed_raster(self._h, int(w), int(h), P, Z, len(P), F, len(F), out))
        return out

    def seed_disparity(self, invH, invQ, subpixelSteps, size, download=True):
        """`Depth2DisparityMap` of the resident seed (sgmhip_seed_disparity); the (h, w) result stays resident as the initial left disparity of
        `tsgm_match_rectified(seeded=True)`.  -> the map, or None without `download`."""
        w, h = size
        ih = np.ascontiguousarray(invH, np.float64); iq = np.ascontiguousarray(invQ, np.float64)
        out = np.zeros((int(h), int(w)) if w > 0 and h > 0 else (1, 1), np.int16) if download else None
        self._chk(self._lib.sgmhip_seed_disparity(self._h, ih, iq, int(subpixelSteps), int(w), int(h), out))
        return out

    def seed_clear(self):
        self._chk(self._lib.sgmhip_seed_clear(self._h))

    def rectify_stats(self):
        """-> (HIP-event milliseconds of the rectification kernel, its launches) since the last stats_reset(True)."""
        ms = C.c_double(0); n = C.c_uint64(0)
        self._chk(self._lib.sgmhip_rectify_stats_get(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def fuse_disparities(self, pairs, size, minViews=2):
        """SemiGlobalMatcher::Fuse in one resident call.  pairs: dicts with disparity, cost, Q, subpixel_steps (the .dimap content); size = (w, h) of
        the reference image.  -> (depthMap, confMap, number of pairs that produced depths)."""
        n = len(pairs); dw, dh = size
        ds = [np.ascontiguousarray(p["disparity"], np.int16) for p in pairs]; cs = [np.ascontiguousarray(p["cost"], np.uint16) for p in pairs]
        dp = (C.POINTER(C.c_int16) * max(n, 1))(*[a.ctypes.data_as(C.POINTER(C.c_int16)) for a in ds])
        cp = (C.POINTER(C.c_uint16) * max(n, 1))(*[a.ctypes.data_as(C.POINTER(C.c_uint16)) for a in cs])
        ws = (C.c_int * max(n, 1))(*[a.shape[1] for a in ds]); hs = (C.c_int * max(n, 1))(*[a.shape[0] for a in ds])
        qs = np.ascontiguousarray(np.stack([np.asarray(p["Q"], np.float64).reshape(16) for p in pairs]) if n else np.zeros((1, 16)), np.float64)
        st = (C.c_int * max(n, 1))(*[int(p["subpixel_steps"]) for p in pairs])
        dep = np.zeros((dh, dw), np.float32); cf = np.zeros((dh, dw), np.float32); used = C.c_int(0)
        self._chk(self._lib.sgmhip_fuse_disparities(self._h, n, dp, cp, ws, hs, qs, st, dw, dh, minViews, dep, cf, C.byref(used)))
        return dep, cf, int(used.value)

    def FilterSpeckles(self, disparity, maxSpeckleSize=100, maxDiff=5):
        a = np.ascontiguousarray(disparity, np.int16).copy()
        self._chk(self._lib.sgmhip_filter_speckles(self._h, a, a.shape[1], a.shape[0], maxSpeckleSize, maxDiff))
        return a

    def sync(self):
        self._chk(self._lib.sgmhip_sync(self._h))

    def stats_reset(self, enable=True):
        self._chk(self._lib.sgmhip_stats_reset(self._h, bool(enable)))

    def stats_get(self) -> SGMHipStats:
        s = SGMHipStats(); self._chk(self._lib.sgmhip_stats_get(self._h, C.byref(s))); return s

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sgmhip_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
