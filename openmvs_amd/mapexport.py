"""The reference's image and per-view PLY outputs, stated in numpy: the statements the device (csrc/pm_export.hip, include/pmhip_export.h) is equal to, bit for bit, as
`views.estimate_normal_map` is for the normal maps.  They are literal restatements of the cited lines, every float step in float32 and every double step in float64; they
are not pinned to compiled reference text.  Where the reference's result is not defined by the language, the engine's definition (include/pmhip_export.h)
is stated here too.  Also the PNG / PFM writers of those outputs, behind an `image_saver(path, array)` hook."""
from __future__ import annotations

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
FZERO_TOLERANCE = np.float32(0.0001)                     # libs/Common/Types.h:579
F = np.float32


def _min(a, b):
    """std::min(a, b) = b < a ? b : a (MINF, libs/Common/Types.h:312): a NaN decides by its position."""
    return np.where(np.less(b, a), b, a).astype(np.float32)


def _max(a, b):
    """std::max(a, b) = a < b ? b : a (MAXF, Types.h:315)."""
    return np.where(np.less(a, b), b, a).astype(np.float32)


def round2int(x):
    """ROUND2INT = (int)floor(x + .5f) (Types.h:949-955) as `pmfu_round2int` states it: whatever is not inside int -- NaN included -- is INT_MIN."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(x, np.float32) + F(0.5))
        ok = (f >= F(-2147483648.0)) & (f < F(2147483648.0))
        return np.where(ok, np.where(ok, f, 0).astype(np.int64), -2147483648)


def to_u8(x):
    """(uint8_t)CLAMP(ROUND2INT(x), 0, 255) (`pmfu_toU8`)."""
    return np.clip(round2int(x), 0, 255).astype(np.uint8)


def x84_threshold(values, mul=5.2):
    """ComputeX84Threshold<float,float> (libs/Common/Util.inl:1001-1024) with GetMinMax (libs/Common/List.h:700) over the values > 0 (zeros, negatives, -0 and NaN do
    not count, as DepthMap2Image and ExportConfidenceMap collect them): (median, mul * MAD, min, max) as float32, or None without a valid value.  The median is the
    element at index n/2 of the sorted values (std::nth_element), the MAD the element at the same index of |v - median| in float.  inf - inf (a median of +inf) is a
    NaN that ranks above +inf (engine-defined)."""
    v = np.asarray(values, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        v = v[v > 0]
    if not len(v):
        return None
    k = len(v) // 2
    median = np.partition(v, k)[k]
    with np.errstate(invalid="ignore"):
        a = np.abs(v - median).astype(np.float32)
    bits = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))          # non-negative floats order like their patterns
    mad = np.partition(bits, k)[k:k + 1].astype(np.uint32).view(np.float32)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return median, F(mul) * mad, v.min(), v.max()


def _base(val):
    """`Base` of Pixel8U::gray2color (libs/Common/Types.inl:2229-2241), ALT = float (Types.h:1844); a NaN fails every test and is 0."""
    val = np.asarray(val, np.float32)
    with np.errstate(invalid="ignore"):
        t = F(2) * val - F(1)
        up = (t - F(-0.75)) * (F(1) - F(0)) / (F(-0.25) - F(-0.75)) + F(0)           # Interpolate(val, y0, x0, y1, x1) = (val - x0) * (y1 - y0) / (x1 - x0) + y0
        down = (t - F(0.25)) * (F(0) - F(1)) / (F(0.75) - F(0.25)) + F(1)
        return np.where(val <= F(0.125), F(0), np.where(val <= F(0.375), up, np.where(val <= F(0.625), F(1), np.where(val <= F(0.87), down, F(0))))).astype(np.float32)


def depth_range(depth):
    """The range DepthMap2Image finds (libs/MVS/DepthMap.cpp:1666-1679): (FLT_MAX, 0) without a valid depth."""
    th = x84_threshold(depth)
    if th is None:
        return FLT_MAX, F(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return _max(th[0] - th[1], th[2])[()], _min(th[0] + th[1], th[3])[()]


def depth_map_to_image(depth, min_depth=None, max_depth=None):
    """DepthMap2Image (DepthMap.cpp:1662-1690) -> ((h, w, 3) uint8, red first; (minDepth, maxDepth) in use).  Without a range (the reference's FLT_MAX, 0) it is found by
    `depth_range`.  Per valid pixel gray2color(CLAMP((maxDepth - depth) * sclDepth, 0, 1)) (Types.inl:2222-2247) through set(float, float, float) (Types.h:1991);
    invalid pixels are black.  minDepth == maxDepth: IEEE arithmetic as it falls (include/pmhip_export.h)."""
    d = np.asarray(depth, np.float32)
    if min_depth is None or max_depth is None or (F(min_depth) == FLT_MAX and F(max_depth) == 0):
        mn, mx = depth_range(d)
    else:
        mn, mx = F(min_depth), F(max_depth)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        scl = F(1) / (mx - mn)
        gray = _min(_max((mx - d) * scl, F(0)), F(1))
        rgb = np.stack([to_u8(_base(gray + F(0.25)) * F(255)), to_u8(_base(gray) * F(255)), to_u8(_base(gray - F(0.25)) * F(255))], axis=-1)
        rgb[~(d > 0)] = 0
    return rgb, (mn, mx)


def normal_map_to_image(normal):
    """The pixel rule of ExportNormalMap (DepthMap.cpp:1700-1715): black where every component is within FZERO_TOLERANCE of 0 (ISZERO, Types.h:1222, Types.inl:540),
    else CLAMP(ROUND2INT(...), 0, 255) of (1 - nx) * 127.5, (1 - ny) * 127.5, -nz * 255."""
    n = np.asarray(normal, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        zero = (np.abs(n) < FZERO_TOLERANCE).all(axis=-1)
        rgb = np.stack([to_u8((F(1) - n[..., 0]) * F(127.5)), to_u8((F(1) - n[..., 1]) * F(127.5)), to_u8(-n[..., 2] * F(255))], axis=-1)
    rgb[zero] = 0
    return rgb


def conf_map_to_image(conf):
    """ExportConfidenceMap (DepthMap.cpp:1721-1749) -> ((h, w) uint8, (minConf, maxConf)), or None without a confidence > 0 (the reference returns false).  The cast
    truncates; a NaN (0 / 0 when maxConf == minConf) is 0 (engine-defined)."""
    c = np.asarray(conf, np.float32)
    th = x84_threshold(c)
    if th is None:
        return None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mn, mx = F(th[0] - th[1]), F(th[0] + th[1])
        if mn < F(0.1):
            mn = F(0.1)
        if mx < F(0.1):
            mx = F(30)
        delta = F(mx - mn)
        s = _min(_max((c - mn) * F(255) / delta, F(0)), F(255))
        img = np.where(np.isnan(s), 0, np.where(np.isnan(s), 0, s).astype(np.int64)).astype(np.uint8)
        img[~(c > 0)] = 0
    return img, (mn, mx)


VIEW_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])                                            # DepthMap.cpp:1759-1762, 15 bytes
VIEW_VERTEX_N = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])   # :1812-1816, 27 bytes


def view_point_cloud(K, R, C, depth, normal=None, bgr=None):
    """MVS::ExportPointCloud (DepthMap.cpp:1753-1870): the records of the valid pixels (depth > 0) in row-major order, `VIEW_VERTEX_N` with a normal map and
    `VIEW_VERTEX` without.  X = (float) TransformPointI2W(Point3(i, j, depth)) in double (Camera.h:339-356), N = R^T n, colour = the image at the same pixel (B, G, R in,
    r g b out) or white.  The image has the map's size here, so the ROUND2INT(scaleImage * i) lookup of the branch without normals (:1790, :1799) is the identity."""
    K = np.asarray(K, np.float64).reshape(3, 3); R = np.asarray(R, np.float64).reshape(3, 3); C = np.asarray(C, np.float64).reshape(3)
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        j, i = np.nonzero(d > 0)
    z = d[j, i].astype(np.float64)
    c0 = (i.astype(np.float64) - K[0, 2]) * z / K[0, 0]; c1 = (j.astype(np.float64) - K[1, 2]) * z / K[1, 1]
    out = np.zeros(len(z), VIEW_VERTEX if normal is None else VIEW_VERTEX_N)
    for k, name in enumerate("xyz"):                                                  # R.t() * X + C: sums from 0, left to right (cv::Matx)
        out[name] = (((0.0 + R[0, k] * c0) + R[1, k] * c1) + R[2, k] * z + C[k]).astype(np.float32)
    if normal is not None:
        n = np.asarray(normal, np.float32)[j, i].astype(np.float64)
        for k, name in enumerate(("nx", "ny", "nz")):
            out[name] = (((0.0 + R[0, k] * n[:, 0]) + R[1, k] * n[:, 1]) + R[2, k] * n[:, 2]).astype(np.float32)
    col = np.full((len(z), 3), 255, np.uint8) if bgr is None else np.asarray(bgr, np.uint8)[j, i]
    out["r"], out["g"], out["b"] = col[:, 2], col[:, 1], col[:, 0]
    return out


def footprint_world(K, R, C, X):
    """Camera::GetFootprintWorld(TPoint3<double>) (libs/MVS/Camera.h:458-471), literally: camX = R (X - C), x = (camX.x / camX.z, camX.y / camX.z), and
    camX.z / sqrt(f^2 + normSq(TransformPointI2V(x))) with TransformPointI2V(x) = x - principal point (Camera.h:324-328) applied to the normalised point."""
    K = np.asarray(K, np.float64).reshape(3, 3); R = np.asarray(R, np.float64).reshape(3, 3); C = np.asarray(C, np.float64).reshape(3)
    d = np.asarray(X, np.float64).reshape(-1, 3) - C
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cam = [((0.0 + R[r, 0] * d[:, 0]) + R[r, 1] * d[:, 1]) + R[r, 2] * d[:, 2] for r in range(3)]
        vx = cam[0] / cam[2] - K[0, 2]; vy = cam[1] / cam[2] - K[1, 2]
        return cam[2] / np.sqrt(K[0, 0] * K[0, 0] + (vx * vx + vy * vy))


def point_scales(points, view_start, views, weights, K, R, C, scale_mult=1.0):
    """The per-point rule of PointCloud::SaveWithScale (libs/MVS/PointCloud.cpp:504-531) -> (scale, confidence), float32 per point.  `weights` None: the smallest
    footprint over the point's views and the number of views; else the scale whose scale / weight is smallest (the first on a tie: the test is a strict >) and that
    weight.  The scale is multiplied by `scale_mult` at the end.  The ASSERT(scale > 0) is not restated: a view behind the point gives a negative scale."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    vs = np.asarray(view_start, np.int64); vv = np.asarray(views, np.int64)
    n = len(P)
    cnt = vs[1:] - vs[:-1]
    owner = np.repeat(np.arange(n), cnt)
    sc = np.zeros(len(vv), np.float32)
    for v in np.unique(vv):
        m = vv == v
        sc[m] = footprint_world(K[v], R[v], C[v], P[owner[m]].astype(np.float64)).astype(np.float32)
    scale = np.full(n, FLT_MAX, np.float32)
    conf = cnt.astype(np.float32) if weights is None else np.zeros(n, np.float32)
    best = np.full(n, FLT_MAX, np.float32)
    w = None if weights is None else np.asarray(weights, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(int(cnt.max()) if n else 0):                                  # the r-th view of every point that has one, in list order
            has = np.nonzero(cnt > r)[0]
            s = sc[vs[has] + r]
            if w is None:
                take = scale[has] > s
                scale[has[take]] = s[take]
                continue
            cw = w[vs[has] + r]
            ratio = (s / cw).astype(np.float32)
            take = best[has] > ratio
            best[has[take]] = ratio[take]; scale[has[take]] = s[take]; conf[has[take]] = cw[take]
        return (scale * F(scale_mult)).astype(np.float32), conf


# ---- writers ---------------------------------------------------------------------------------------------------------------------------------------------------------
def save_image(path, array):
    """The default `image_saver`: an (h, w) or (h, w, 3) uint8 array (red first) as the file type of the name, through PIL."""
    from PIL import Image
    a = np.ascontiguousarray(array, np.uint8)
    Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(path)


def save_pfm(path, array):
    """TImage<float>::Save of a .pfm (one channel, little-endian scale -1, rows bottom to top)."""
    a = np.asarray(array, np.float32)
    with open(path, "wb") as f:
        f.write(("Pf\n%d %d\n%f\n" % (a.shape[1], a.shape[0], -1.0)).encode("ascii"))
        f.write(np.ascontiguousarray(a[::-1], "<f4").tobytes())
