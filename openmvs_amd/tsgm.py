"""The tSGM coarse-to-fine loop of `SemiGlobalMatcher::Match(scene, ...)` for one rectified image pair
(reference `libs/MVS/SemiGlobalMatcher.cpp:577-706`), on top of the C-ABI steps of include/sgmhip.h.

What is here is the loop body between rectification and export: per pyramid level the two `Match` calls (right->left with ranges from
the flipped previous disparities, then left->right), the consistency checks, the first-level speckle filter and mask extraction, the mask
up-scaling, and the final sub-pixel refinement.  What is not: `Image::StereoRectifyImages` (OpenCV `stereoRectify` + remap) and the initial
disparity map from the sparse points (`TriangulatePoints2DepthMap` with corners + `Depth2DisparityMap`) -- the caller passes rectified images,
their masks, and optionally that initial half-resolution disparity map (without it the first level searches the default range).

The loop is written against a small backend interface so that the very same code runs on the device (`SemiGlobalMatcherHIP`, plus a float
INTER_AREA resampler) and, in the tests, on the CPU oracle.
"""
from __future__ import annotations

import numpy as np

NO_DISP = 32767
HW = 3                       # halfWindowSizeX / Y


def compute_scale(width: int, height: int, min_resolution: int) -> int:
    """The pyramid depth of :577-583: returns k with scale = 1 / 2^k (k = 0: plain SGM)."""
    if not min_resolution:
        return 0
    size0 = max(width, height)
    level = 8                                    # computeMaxResolution(w, h, level = 8, minResolution), libs/Common/Types.inl:2459-2477
    if (size0 >> level) < min_resolution:
        level = 0
        while (size0 >> (level + 1)) >= min_resolution:
            level += 1
    return max(1, level)                         # scale = 1 / max(2, 2^level)


def resize_area_u8(img: np.ndarray, f: int) -> np.ndarray:
    """cv::resize(img, Size(), 1/f, 1/f, INTER_AREA) for an 8-bit image whose size is a multiple of f: OpenCV's integer-factor path -- for
    f = 2 the rounded mean (a+b+c+d+2)>>2 of ResizeAreaFastVec, otherwise saturate_cast<uchar>(sum * (1/f^2)) (round half to even)."""
    if f == 1:
        return img
    H, W = img.shape[:2]
    if W % f or H % f:
        raise NotImplementedError("tsgm: image size %dx%d is not a multiple of %d" % (W, H, f))
    s = img.reshape(H // f, f, W // f, f, -1).astype(np.int32).sum(axis=(1, 3))
    out = ((s + 2) >> 2) if f == 2 else np.rint(s.astype(np.float32) * np.float32(1.0 / (f * f)))
    return out.astype(np.uint8).reshape((H // f, W // f) + img.shape[2:])


def resize_nearest_u8(img: np.ndarray, w: int, h: int) -> np.ndarray:
    """cv::resize(mask, size, INTER_NEAREST): sx = min(floor(dx * ifx), sw - 1) with ifx = 1 / (dw / sw) in double (resizeNN; csrc/pm_math.h pm_nn_index)."""
    H, W = img.shape
    ys = np.minimum(np.floor(np.arange(h) * (1.0 / (h / float(H)))).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(w) * (1.0 / (w / float(W)))).astype(np.int64), W - 1)
    return img[ys][:, xs]


MAX_UNIFORM_DISP = 1024      # SGMHIP_MAX_UNIFORM_DISP (include/sgmhip.h)


def plain_range(seed) -> tuple:
    """The global disparity range of plain SGM (:644-661; the numpy twin of sgmhip_plain_range): min and max over the seed, NO_DISP entries included, then
    numDisp = (max - min) + 16, disp = min + max, [disp - numDisp, disp + numDisp) -- every intermediate a Disparity (int16) that wraps as one."""
    a = np.asarray(seed, np.int16)
    if a.size == 0:
        raise ValueError("plain_range: the seed map is empty")
    i16 = lambda v: int(np.array(v, np.int64).astype(np.int16))
    mn, mx = int(a.min()), int(a.max())
    num = i16(i16(mx - mn) + 16)
    disp = i16(mn + mx)
    return i16(disp - num), i16(disp + num)


def _plain_match(be, left_bgr, left_gray, right_bgr, right_gray, init_left_disparity, n_speckle_size, subpixel_mode, subpixel_steps):
    """Plain SGM (minResolution = 0, :585-590, 643-706): one level at full resolution, every pixel with the global range of the half-resolution seed.  Match(right,
    left) takes that range as it is, Match(left, right) its negation -- the reference's assignment, the opposite of the tSGM branch.  The reference also crops the
    masks and extracts them again after the filtering (:612-617, 705-706) and never reads them: they are not computed here."""
    h, w = left_gray.shape
    sh = (int(np.rint(h * 0.5)) - 2 * HW, int(np.rint(w * 0.5)) - 2 * HW)                  # Image8U::computeResize(size, 0.5), :611-625
    if h <= 2 * HW or w <= 2 * HW or sh[0] <= 0 or sh[1] <= 0:
        raise ValueError("plain SGM: the half-resolution seed grid of a %d x %d image is empty" % (w, h))
    if init_left_disparity is not None:
        seed = np.ascontiguousarray(init_left_disparity, np.int16)
        if seed.shape != sh:
            raise ValueError("initial disparity map must be %dx%d" % (sh[1], sh[0]))
    else:
        seed = np.full(sh, NO_DISP, np.int16)
    mn, mx = plain_range(seed)
    D = mx - mn
    if D <= 0 or D > MAX_UNIFORM_DISP or mn < -32767:
        raise ValueError("plain SGM: the seed's disparities span %d .. %d (min, max), which gives the range [%d, %d), D = %d: it must hold 1 .. %d disparities"
                         % (int(seed.min()), int(seed.max()), mn, mx, D, MAX_UNIFORM_DISP))

    def match(bgr, ga, gb, a, b):
        if hasattr(be, "set_problem_uniform"):
            be.set_problem_uniform(bgr, ga, gb, a, b)
        else:
            n = (h - 2 * HW) * (w - 2 * HW)
            px = np.zeros(n, [("idx", np.uint64), ("minDisp", np.int16), ("maxDisp", np.int16), ("pad_", np.int32)])     # SGMHipPixelData
            px["idx"] = np.arange(n, dtype=np.uint64) * np.uint64(b - a); px["minDisp"] = a; px["maxDisp"] = b
            be.set_problem(bgr, ga, gb, px, n * (b - a), b - a)
        be.Match()
        return be.results()

    right_disp, _ = match(right_bgr, right_gray, left_gray, mn, mx)                           # :667-676
    left_disp, _ = match(left_bgr, left_gray, right_gray, -mx, -mn)                           # :678-685
    left_disp = be.ConsistencyCrossCheck(left_disp, right_disp)                                # :698-706
    right_disp = be.ConsistencyCrossCheck(right_disp, left_disp)
    left_disp = be.FilterSpeckles(left_disp, n_speckle_size, 5)
    right_disp = be.FilterSpeckles(right_disp, n_speckle_size, 5)
    be.set_disparity(left_disp)
    be.RefineDisparityMap(subpixel_mode, subpixel_steps)
    refined, cost = be.results()
    return refined, cost, 1


def tsgm_match(be, left_bgr, left_gray, right_bgr, right_gray, left_mask, right_mask, min_resolution=320, init_left_disparity=None,
               n_speckle_size=100, subpixel_mode=6, subpixel_steps=4):
    """Runs the loop; returns (left disparity map at full resolution, refined to `subpixel_steps`, its cost map, the number of levels).

    `be` provides: resize_area_f32(img, f); set_problem / Match / results (as SemiGlobalMatcherHIP); ConsistencyCrossCheck, FilterSpeckles,
    ExtractMask, UpscaleMask, FlipDirection, Disparity2RangeMap, RefineDisparityMap."""
    H, W = left_gray.shape
    k = compute_scale(W, H, min_resolution)
    if k == 0:
        return _plain_match(be, left_bgr, left_gray, right_bgr, right_gray, init_left_disparity, n_speckle_size, subpixel_mode, subpixel_steps)
    left_disp = right_disp = None
    cost = None
    levels = 0
    for lvl in range(k, -1, -1):
        f = 1 << lvl
        lb, rb = resize_area_u8(left_bgr, f), resize_area_u8(right_bgr, f)
        lg = left_gray if f == 1 else be.resize_area_f32(left_gray, f)
        rg = right_gray if f == 1 else be.resize_area_f32(right_gray, f)
        h, w = lg.shape
        vw, vh = w - 2 * HW, h - 2 * HW
        first = left_disp is None
        if first:
            hw2, hh2 = int(np.rint(w * 0.5)), int(np.rint(h * 0.5))                      # Image8U::computeResize(size, 0.5)
            if init_left_disparity is not None:
                left_disp = np.ascontiguousarray(init_left_disparity, np.int16)
                if left_disp.shape != (hh2 - 2 * HW, hw2 - 2 * HW):
                    raise ValueError("initial disparity map must be %dx%d" % (hw2 - 2 * HW, hh2 - 2 * HW))
            else:
                left_disp = np.full((hh2 - 2 * HW, hw2 - 2 * HW), NO_DISP, np.int16)
            lm = resize_nearest_u8(left_mask, w, h)[HW:HW + vh, HW:HW + vw].copy()        # :612-617
            rm = resize_nearest_u8(right_mask, w, h)[HW:HW + vh, HW:HW + vw].copy()
        else:
            lm = be.UpscaleMask(lm, (vw, vh)); rm = be.UpscaleMask(rm, (vw, vh))          # :619-621
        a, b = (11, 33) if first else (5, 7)
        right_disp = be.FlipDirection(left_disp)                                           # :626-627
        px, n, mx = be.Disparity2RangeMap(right_disp, rm, a, b)
        be.set_problem(rb, rg, lg, px, n, mx); be.Match()                                  # Match(rightDataLevel, leftDataLevel, ...), :654
        right_disp, _ = be.results()
        px, n, mx = be.Disparity2RangeMap(left_disp, lm, a, b)                             # :657
        be.set_problem(lb, lg, rg, px, n, mx); be.Match()                                  # :667
        left_disp, cost = be.results()
        if first:                                                                          # :680-690
            left_disp = be.ConsistencyCrossCheck(left_disp, right_disp)
            right_disp = be.ConsistencyCrossCheck(right_disp, left_disp)
            left_disp = be.FilterSpeckles(left_disp, n_speckle_size, 5)
            right_disp = be.FilterSpeckles(right_disp, n_speckle_size, 5)
            lm = be.ExtractMask(left_disp, lm); rm = be.ExtractMask(right_disp, rm)
        else:
            left_disp = be.ConsistencyCrossCheck(left_disp, right_disp)                    # :693
        levels += 1
    # RefineDisparityMap works on the resident sums of the last Match with the cross-checked map (:699): push the checked map back first
    be.set_disparity(left_disp)
    be.RefineDisparityMap(subpixel_mode, subpixel_steps)
    refined, cost = be.results()
    return refined, cost, levels
