"""Shared cases of the image and PLY outputs (csrc/pm_export.hip, include/pmhip_export.h), run on the emulator by tests/test_emu_map_export.py and on the device by
tests/test_zz_gpu_map_export.py: every device result equals its numpy statement in openmvs_amd/mapexport.py bit for bit -- uint8 images equal, records byte-equal,
floats compared as uint32.  The work quanta come from `engine.export_stats()`; nothing here repeats them.  Cases whose result the reference leaves undefined are pinned
on their own, against the value include/pmhip_export.h defines."""
import ctypes as C
import os

import numpy as np

from openmvs_amd import mapexport as mx

f32 = np.float32
FLT_MAX = np.finfo(f32).max
K0 = np.array([[90.0, 0, 31.5], [0, 88.0, 8.25], [0, 0, 1]])
R0 = np.array([[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]])
C0 = np.array([0.3, -0.2, 0.1])


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.nonzero(bits(got) != bits(want))
    assert not len(bad[0]), "%s: %d of %d values differ, first at %s: %r, expected %r" % (what, len(bad[0]), got.size, tuple(int(b[0]) for b in bad), got[bad][0], want[bad][0])


def same_image(got, want, what):
    assert got.dtype == np.uint8 and want.dtype == np.uint8 and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.nonzero(got != want)
    assert not len(bad[0]), "%s: %d of %d bytes differ, first at %s: %d, expected %d" % (what, len(bad[0]), got.size, tuple(int(b[0]) for b in bad), got[bad][0], want[bad][0])


# ---- selection ---------------------------------------------------------------------------------------------------------------------------------------------------------
def interleave(valid, seed=0):
    """The valid values, in their order, with zeros, negatives, -0.0 and NaN between them: count != area."""
    rng = np.random.default_rng(seed)
    n = len(valid)
    junk = np.array([0.0, -1.5, -0.0, np.nan, -np.inf], f32)
    gaps = rng.integers(0, 3, n + 1)
    out = []
    for k in range(n):
        out.extend(junk[rng.integers(0, len(junk), gaps[k])]); out.append(valid[k])
    out.extend(junk[rng.integers(0, len(junk), gaps[n] + 1)])
    a = np.array(out, f32)
    with np.errstate(invalid="ignore"):
        assert (a > 0).sum() == n and a.size > n
    return a


def check_selection(e, flat, what, layouts=((1, -1),)):
    """pmhip_x84_threshold and, through pmhip_depth_image, DepthMap2Image's range of the flat array laid out as the listed (h, w) shapes (-1: the whole length)."""
    want = mx.x84_threshold(flat)
    with np.errstate(invalid="ignore"):
        v = flat[flat > 0]
    k = len(v) // 2
    med = np.partition(v, k)[k]
    assert bits(want[0]) == bits(med) and want[2] == v.min() and want[3] == v.max(), what
    if np.isfinite(med):
        assert bits(want[1]) == bits(f32(5.2) * np.partition(np.abs(v - med), k)[k]), what
    got = e.x84_threshold(flat)
    same_bits(np.array(got), np.array(want), "x84 threshold of " + what)
    for h, w in layouts:
        m = flat.reshape(h, w)
        img, rng = e.depth_image(m)
        timg, trng = mx.depth_map_to_image(m)
        same_bits(np.array(rng), np.array(trng), "depth range of %s as %s" % (what, m.shape))
        same_image(img, timg, "depth image of %s as %s" % (what, m.shape))
    return want


def quantum_counts(e):
    q = e.export_stats()["quantum"]
    return [q - 1, q, q + 1]


def count_case(e, n, seed=1):
    """n valid values in a map with as many invalid ones again, as 1 x area, area x 1 and -- when the area has a divisor -- a rectangle."""
    rng = np.random.default_rng(seed + n)
    flat = interleave(rng.uniform(0.5, 9.0, n).astype(f32), seed + n)
    layouts = [(1, -1), (-1, 1)] + [(d, -1) for d in (7, 5, 3, 2) if flat.size % d == 0][:1]
    check_selection(e, flat, "%d valid values" % n, layouts)


def past_the_grid_cap(e):
    """More valid values than one trip of the capped grid takes: the only case with a second grid-stride trip, and the values the second trip reads decide the result."""
    s = e.export_stats()
    one_trip = s["quantum"] * s["grid_cap"]
    rng = np.random.default_rng(5)
    n = one_trip + s["quantum"] + 1
    v = rng.uniform(1.0, 2.0, n).astype(f32)
    v[one_trip:] = rng.uniform(50.0, 60.0, n - one_trip).astype(f32)          # the maximum lies in the second trip
    flat = np.concatenate([np.zeros(3, f32), v, np.array([np.nan, -1.0], f32)])
    assert flat.size > one_trip and flat.size % 2 == 0
    want = check_selection(e, flat, "%d valid values, past one trip of the grid" % n, ((2, -1),))
    assert want[3] >= 50


def pattern_cases(e):
    rng = np.random.default_rng(7)
    n = 257
    k = n // 2
    check_selection(e, interleave(np.full(n, 3.25, f32), 1), "all values equal")                   # MAD = 0
    assert mx.x84_threshold(np.full(n, 3.25, f32))[1] == 0
    for below in (k - 1, k, k + 1):                                                                  # two distinct values around the cut
        v = np.r_[np.full(below, 2.0, f32), np.full(n - below, 5.0, f32)]
        rng.shuffle(v)
        want = check_selection(e, interleave(v, below), "%d values below the cut of %d" % (below, k))
        assert want[0] == (5.0 if below <= k else 2.0)
    low = (np.uint32(0x40490F00) + rng.integers(0, 256, n).astype(np.uint32)).view(f32)              # every digit but the lowest shared
    check_selection(e, interleave(low, 2), "values that differ in the lowest digit only")
    tops = np.arange(0, 0x7F, dtype=np.uint32)
    high = np.r_[(tops << np.uint32(24)) | np.uint32(1), np.array([0x7F7FFFFF, 0x7F800000], np.uint32)].view(f32)   # smallest denormal ... FLT_MAX, +inf
    assert high[0] == np.nextafter(f32(0), f32(1)) and high[-2] == FLT_MAX and np.isinf(high[-1])
    rng.shuffle(high)
    want = check_selection(e, interleave(high, 3), "values that differ in the highest digit only")
    assert np.isfinite(want[0]) and want[2] == np.nextafter(f32(0), f32(1)) and np.isinf(want[3])
    dup = np.r_[rng.uniform(1, 2, 40), np.full(180, 2.5), rng.uniform(3, 4, 37)].astype(f32)
    rng.shuffle(dup)
    assert check_selection(e, interleave(dup, 4), "many duplicates of the median")[0] == 2.5
    asc = np.sort(rng.uniform(0.1, 100.0, 300).astype(f32))
    check_selection(e, interleave(asc, 5), "ascending values")
    check_selection(e, interleave(asc[::-1].copy(), 6), "descending values")


def infinite_median_is_pinned(e):
    """Engine-defined (include/pmhip_export.h): a median of +inf makes |v - median| a NaN for the infinite values, which ranks above +inf."""
    flat = np.array([1.0, np.inf, 0.0, np.inf, np.inf], f32)
    got = e.x84_threshold(flat)
    assert np.isinf(got[0]) and np.isnan(got[1]) and got[2] == 1.0 and np.isinf(got[3])
    flat = np.array([1.0, 2.0, np.inf, np.inf, np.inf, np.inf, np.inf], f32)          # |v - inf|: two +inf, five NaN -- index 3 is a NaN, index 1 would be +inf
    assert np.isnan(e.x84_threshold(flat)[1]) and np.isnan(mx.x84_threshold(flat)[1])
    flat = np.array([1.0, 2.0, 3.0, np.inf, np.inf, np.inf, 4.0], f32)                # index 3 of (1 2 3 4 inf inf inf) is 4: finite median, |v - 4| = 3 2 1 0 inf inf inf -> 3
    got = e.x84_threshold(flat)
    assert got[0] == 4.0 and got[1] == f32(5.2) * f32(3.0)


def no_valid_value(e, error):
    try:
        e.x84_threshold(np.array([0.0, -1.0, np.nan, -0.0], f32))
    except error as ex:
        assert "pmhip error -1" in str(ex) and "no value > 0" in str(ex), str(ex)
    else:
        raise AssertionError("an array without a valid value was accepted")
    assert e.x84_threshold(np.array([2.0], f32)) == (2.0, 0.0, 2.0, 2.0)


# ---- the colour map ------------------------------------------------------------------------------------------------------------------------------------------------------
COLOUR_SIZES = ((1, 1), (1, 65), (7, 37))                                                      # (h, w)


def colour_map_case(e, h, w):
    """A given range 0 .. 8 and the depths 1 ... 8: the grays are exact eighths, which meet 0.125, 0.375, 0.625 and the value beside 0.87 on all three channel offsets."""
    d = (np.arange(h * w) % 9).astype(f32).reshape(h, w)                                        # 0 (invalid), 1 ... 8
    if h * w == 1:
        d[:] = 3
    img, rng = e.depth_image(d, 0.0, 8.0)
    want, _ = mx.depth_map_to_image(d, 0.0, 8.0)
    same_image(img, want, "colour map %d x %d" % (w, h))
    assert tuple(rng) == (0.0, 8.0) and not img[d == 0].any()
    if h * w >= 9:
        # gray = (8 - d) / 8; the channels by hand at the breakpoints: gray 0.125 -> Base(0.375) = 1, Base(0.125) = 0, Base(-0.125) = 0
        assert tuple(img[d == 7][0]) == (255, 0, 0) and tuple(img[d == 5][0]) == (255, 255, 0) and tuple(img[d == 3][0]) == (0, 255, 255) and tuple(img[d == 8][0]) == (128, 0, 0)
        assert tuple(img[d == 1][0]) == (0, 0, 255)                                             # gray 0.875: Base(0.875) = 0 (> 0.87), Base(0.625) = 1


def no_valid_pixel(e):
    for d in (np.zeros((5, 13), f32), np.array([[-1.0, np.nan, -0.0, 0.0]], f32)):
        img, rng = e.depth_image(d)
        assert not img.any() and rng[0] == FLT_MAX and rng[1] == 0
        want, trng = mx.depth_map_to_image(d)
        assert not want.any() and trng[0] == FLT_MAX and trng[1] == 0


def equal_range_is_pinned(e):
    """Engine-defined (include/pmhip_export.h): minDepth == maxDepth makes sclDepth infinite; a depth equal to the range is 0 * inf = NaN and black, a nearer one gray 1,
    a farther one gray 0."""
    d = np.zeros((3, 5), f32); d[1, 2] = 2.5
    img, rng = e.depth_image(d)
    assert not img.any() and tuple(rng) == (2.5, 2.5)
    d = np.array([[3.0, 4.0, 5.0, 0.0]], f32)
    img, rng = e.depth_image(d, 4.0, 4.0)
    assert tuple(rng) == (4.0, 4.0) and img.tolist() == [[[0, 0, 128], [0, 0, 0], [128, 0, 0], [0, 0, 0]]], img.tolist()
    same_image(img, mx.depth_map_to_image(d, 4.0, 4.0)[0], "equal range")


# ---- scenes for the resident maps ------------------------------------------------------------------------------------------------------------------------------------------
def make_scene(e, sizes, n_levels=0):
    """A scene of len(sizes) views, the first one's size being the scene's; cameras K0 (principal point moved with the size), R0, C0 + i."""
    w, h = sizes[0]
    e.scene_create(max(len(sizes), 2), w, h, n_levels)
    cams = []
    for i, (sw, sh) in enumerate(sizes):
        K = K0.copy(); K[0, 2] = (sw - 1) / 2.0 + 0.25 * i; K[1, 2] = (sh - 1) / 2.0
        Ci = C0 + np.array([0.4 * i, 0.0, 0.0])
        (e.scene_set_view_sized if (sw, sh) != (w, h) else e.scene_set_view)(i, np.zeros((sh, sw), f32), K, R0, Ci, 0.1, 100.0, [j for j in range(len(sizes)) if j != i][:1])
        cams.append((K, R0, Ci))
    return cams


def install(e, i, depth, normal=None, conf=None):
    e.scene_set_maps(i, depth, np.zeros(depth.shape + (3,), f32) if normal is None else normal)
    if conf is not None:
        e.scene_set_conf(i, conf)


def normal_image_cases(e):
    tol = mx.FZERO_TOLERANCE
    lo, hi = np.nextafter(tol, f32(0)), tol                                                  # just inside (a zero) and just outside the tolerance
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0),
            (0, 0.6, -0.8),                                                                   # (1 - 0) * 127.5 is the .5 tie: 128
            (0.6, 0.0, 0.8),                                                                  # nz > 0 clamps to 0
            (lo, lo, lo), (-lo, lo, -lo), (hi, lo, lo), (lo, hi, lo), (lo, lo, hi), (lo, lo, -hi), (-hi, -hi, -hi),
            (-2.0, 3.0, -1.5), (0.3, -0.4, -0.866)]
    w, h = 11, 9
    make_scene(e, [(w, h), (7, 5)])
    rng = np.random.default_rng(31)
    for i, (sw, sh) in enumerate(((w, h), (7, 5))):
        n = rng.standard_normal((sh, sw, 3)).astype(f32)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        flat = n.reshape(-1, 3); flat[:len(rows)] = np.array(rows, f32)[:len(flat)]
        install(e, i, np.ones((sh, sw), f32), n)
        got = e.scene_normal_image(i)
        same_image(got, mx.normal_map_to_image(n), "normal image of view %d" % i)
        g = got.reshape(-1, 3)
        assert g[0].tolist() == [0, 128, 0] and g[5].tolist() == [128, 128, 255] and g[6].tolist() == [0, 0, 0] and g[7].tolist() == [128, 51, 204] and g[8, 2] == 0
        assert g[9].tolist() == [0, 0, 0] and g[10].tolist() == [0, 0, 0] and g[11].any() and g[15].any()
    n = np.zeros((h, w, 3), f32); n[0, 0] = (np.nan, 0.5, -0.5); n[0, 1] = (np.inf, -np.inf, np.nan)     # engine-defined: ROUND2INT of a NaN or beyond int is INT_MIN, clamped to 0
    install(e, 0, np.ones((h, w), f32), n)
    got = e.scene_normal_image(0)
    assert got[0, 0].tolist() == [0, 64, 128] and got[0, 1].tolist() == [0, 0, 0]
    same_image(got, mx.normal_map_to_image(n), "non-finite normals")


def conf_image_cases(e):
    w, h = 13, 9
    make_scene(e, [(w, h), (5, 7)])
    rng = np.random.default_rng(32)
    d = np.ones((h, w), f32)

    def run(i, c, what):
        install(e, i, np.ones(c.shape, f32), None, c)
        got = e.scene_conf_image(i)
        want = mx.conf_map_to_image(c)
        same_image(got[0], want[0], what)
        same_bits(np.array(got[1]), np.array(want[1]), "range of " + what)
        return got

    c = rng.uniform(0.3, 0.7, (h, w)).astype(f32); c[rng.random((h, w)) < 0.2] = 0
    assert run(0, c, "minConf below the floor")[1][0] == f32(0.1)
    c = rng.uniform(0.01, 0.02, (7, 5)).astype(f32)
    assert tuple(run(1, c, "maxConf below the floor")[1]) == (f32(0.1), f32(30))
    # a value exactly maxConf and the truncating cast.  Thirty each of 1, 2, 3 with x = 2 + 5.2 * 1 and five more values inside the range: index n/2 of the sorted values
    # is a 2 and of the deviations a 1 wherever the six fall, so minConf = 0.1 (the floor), maxConf = x, and the five are placed at scaled values k + 0.999
    x = f32(2) + f32(5.2) * f32(1)
    ks = np.array([0, 1, 100, 200, 253], np.float64)
    vals = (np.float64(f32(0.1)) + (ks + 0.999) * (np.float64(x) - np.float64(f32(0.1))) / 255.0).astype(f32)
    c = np.zeros(h * w, f32)
    c[:96] = np.r_[np.repeat(np.array([1, 2, 3], f32), 30), x, vals]
    rng.shuffle(c)
    got = run(0, c.reshape(h, w), "a value exactly maxConf, scaled values of k + 0.999")
    assert tuple(got[1]) == (f32(0.1), x) and got[0].ravel()[c == x][0] >= 254
    assert [int(got[0].ravel()[c == v][0]) for v in vals] == [0, 1, 100, 200, 253]
    install(e, 0, d, None, np.zeros((h, w), f32))
    assert e.scene_conf_image(0) is None and mx.conf_map_to_image(np.zeros((h, w), f32)) is None
    c = np.full((h, w), -1.0, f32); c[0, 0] = np.nan
    install(e, 0, d, None, c)
    assert e.scene_conf_image(0) is None


def equal_confidence_is_pinned(e):
    """Engine-defined (include/pmhip_export.h): maxConf == minConf and a confidence equal to both is 0 / 0 = NaN, whose cast is 0."""
    w, h = 13, 9
    make_scene(e, [(w, h), (5, 7)])
    c = np.full((h, w), 1.0, f32); c[0, 0] = 0; c[0, 1] = 2.0; c[0, 2] = 0.5
    install(e, 0, np.ones((h, w), f32), None, c)
    img, rng = e.scene_conf_image(0)
    assert tuple(rng) == (1.0, 1.0) and img[0, 0] == 0 and img[0, 1] == 255 and img[0, 2] == 0 and not img[1:].any()
    same_image(img, mx.conf_map_to_image(c)[0], "equal confidences")


# ---- the cloud of a view -----------------------------------------------------------------------------------------------------------------------------------------------
CLOUD_WIDTHS = (63, 64, 65)


def view_cloud_case(e, w, error):
    """Width w, 17 rows (the valid count straddles one scan tile at every width), a second view of its own size: with and without normals and colour, every row pattern."""
    h = 17
    tile = e.export_stats()["scan_tile"]
    cams = make_scene(e, [(w, h), (37, 11), (w, h)])
    rng = np.random.default_rng(40 + w)
    for i, (sw, sh) in enumerate(((w, h), (37, 11), (w, h))):
        d = rng.uniform(1.0, 6.0, (sh, sw)).astype(f32)
        d[rng.random((sh, sw)) < 0.2] = 0
        d[2] = 0                                                                               # a row with no valid pixel
        d[3] = rng.uniform(1.0, 6.0, sw)                                                       # a row with every pixel valid
        d[4] = 0; d[4, -1] = 2.0                                                               # only the last pixel
        d[5, ::2] = -1.0; d[6, 0] = np.nan
        n = rng.standard_normal((sh, sw, 3)).astype(f32)
        bgr = rng.integers(0, 256, (sh, sw, 3)).astype(np.uint8)
        install(e, i, d, n)
        if i != 2:
            e.scene_set_color(i, bgr)
        if i == 0:
            n0, bgr0 = n, bgr
        for with_n in (True, False):
            want = mx.view_point_cloud(*cams[i], d, n if with_n else None, None if i == 2 else bgr)
            got = e.scene_view_cloud(i, with_n)
            assert got.dtype.itemsize == (27 if with_n else 15) and got.tobytes() == want.tobytes(), "view %d (%d x %d), normals %s: records differ" % (i, sw, sh, with_n)
            assert e.scene_view_cloud(i, with_n, capacity=len(want)).tobytes() == want.tobytes()        # capacity == count
        if i == 2:
            assert (got["r"] == 255).all() and (got["g"] == 255).all() and (got["b"] == 255).all()
    # all pixels valid, then only the last one, then exactly one tile and one more
    for d in (np.full((h, w), 3.0, f32), np.r_[np.zeros(h * w - 1, f32), f32(2)].reshape(h, w), np.r_[np.ones(tile, f32), np.zeros(h * w - tile - 1, f32), f32(1)].reshape(h, w)):
        install(e, 0, d, n0)
        for with_n in (True, False):
            want = mx.view_point_cloud(*cams[0], d, n0 if with_n else None, bgr0)
            assert len(want) == int((d > 0).sum()) and e.scene_view_cloud(0, with_n).tobytes() == want.tobytes(), "%d valid pixels, normals %s" % (len(want), with_n)
    # capacity == count - 1: refused, the needed count is returned, nothing is written
    need = int((d > 0).sum())
    rec = np.full(need * 27, 0xEE, np.uint8); cnt = C.c_uint64(0)
    rc = e._lib.pmhip_scene_view_cloud(e._h, 0, 1, rec, need - 1, C.byref(cnt))
    assert rc == -1 and cnt.value == need and (rec == 0xEE).all() and b"capacity" in e._lib.pmhip_last_error(e._h)
    try:
        e.scene_view_cloud(0, True, capacity=need - 1)
    except error as ex:
        assert "pmhip error -1" in str(ex)
    else:
        raise AssertionError("a capacity below the count was accepted")
    assert len(e.scene_view_cloud(0, True)) == need


def empty_view_cloud(e, tmp_dir):
    from openmvs_amd import plyio
    w, h = 21, 9
    make_scene(e, [(w, h), (5, 7)])
    install(e, 0, np.zeros((h, w), f32))
    for with_n in (True, False):
        got = e.scene_view_cloud(0, with_n)
        assert len(got) == 0
        assert plyio.save_view_cloud(os.path.join(str(tmp_dir), "empty.ply"), got, with_n) is False and not os.path.exists(os.path.join(str(tmp_dir), "empty.ply"))


# ---- scales ------------------------------------------------------------------------------------------------------------------------------------------------------------
def scale_cases(e):
    """1, 2 and 17 views per point (the cloud's count is a uint8, not PM_MAX_SRC), with and without weights, a weight of 0, a camera behind the point, a scaleMult that is
    no power of two."""
    nv = 18
    w, h = 33, 17
    e.scene_create(nv, w, h, 0)
    rng = np.random.default_rng(50)
    Ks, Rs, Cs = [], [], []
    for i in range(nv):
        a = 0.05 * i
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        K = np.array([[100.0 + 7 * i, 0, 16.0 + 0.5 * i], [0, 95.0 + 3 * i, 8.0], [0, 0, 1]])
        Cc = np.array([0.3 * i - 2.0, 0.1 * i, -0.2 * i])
        if i == nv - 1:
            Cc = np.array([0.0, 0.0, 40.0])                                                   # every point lies behind this camera
        e.scene_set_view(i, np.zeros((h, w), f32), K, R, Cc, 0.1, 100.0, [(i + 1) % nv])
        Ks.append(K); Rs.append(R); Cs.append(Cc)
    P = 300
    pts = np.c_[rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(6, 12, P)].astype(f32)
    cnt = np.r_[np.full(100, 1), np.full(100, 2), np.full(100, 17)]
    rng.shuffle(cnt)
    vs = np.r_[0, np.cumsum(cnt)].astype(np.uint32)
    views = np.concatenate([np.sort(rng.choice(nv - 1, c, replace=False)) for c in cnt]).astype(np.uint32)
    views[vs[7]] = nv - 1                                                                      # one point seen from behind
    wts = rng.uniform(0.1, 50.0, len(views)).astype(f32)
    wts[vs[11]] = 0                                                                            # a weight of 0 (scale / 0 = inf never wins)
    for weights in (None, wts):
        e.scene_cloud_set(pts, vs, views, weights)
        for mult in (1.0, 1.7):
            got = e.scene_cloud_scale(mult)
            want = mx.point_scales(pts, vs, views, weights, Ks, Rs, Cs, mult)
            same_bits(got[0], want[0], "scales, weights %s, scaleMult %g" % (weights is not None, mult))
            same_bits(got[1], want[1], "confidences, weights %s, scaleMult %g" % (weights is not None, mult))
        if weights is None:
            assert np.array_equal(got[1], cnt.astype(f32)) and got[0][7] < 0, "the negative scale of the camera behind the point is recorded"
    assert (got[0] > 0).sum() > P - 5


def scale_tie_case(e):
    """A tie in scale / weight: on the optical axis of two cameras with focal lengths 512 and 256 the scales are z / 512 and z / 256 exactly; with weights 0.5 and 1 the
    ratios are equal, and the first view of the list wins (the test is a strict >)."""
    e.scene_create(2, 33, 17, 0)
    Ks = [np.array([[f, 0, 0.0], [0, f, 0.0], [0, 0, 1]]) for f in (512.0, 256.0)]
    for i in range(2):
        e.scene_set_view(i, np.zeros((17, 33), f32), Ks[i], np.eye(3), np.zeros(3), 0.1, 100.0, [1 - i])
    pts = np.array([[0, 0, 8.0], [0, 0, 8.0]], f32)
    vs = np.array([0, 2, 4], np.uint32)
    views = np.array([0, 1, 1, 0], np.uint32); wts = np.array([0.5, 1.0, 1.0, 0.5], f32)
    e.scene_cloud_set(pts, vs, views, wts)
    scale, conf = e.scene_cloud_scale(1.0)
    assert scale.tolist() == [8.0 / 512, 8.0 / 256] and conf.tolist() == [0.5, 1.0]
    want = mx.point_scales(pts, vs, views, wts, Ks, [np.eye(3)] * 2, [np.zeros(3)] * 2, 1.0)
    same_bits(scale, want[0], "tie"); same_bits(conf, want[1], "tie")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def error_cases(e, error):
    w, h = 21, 9
    make_scene(e, [(w, h), (5, 7)])
    d = np.full((h, w), 2.0, f32)
    install(e, 0, d, None, np.full((h, w), 0.5, f32))
    calls = (("scene_depth_image", lambda i: e.scene_depth_image(i)), ("scene_normal_image", lambda i: e.scene_normal_image(i)), ("scene_conf_image", lambda i: e.scene_conf_image(i)),
             ("scene_view_cloud", lambda i: e.scene_view_cloud(i, True)))
    for name, call in calls:
        for idx, code, word in ((2, -1, "not a view"), (-1, -1, "not a view"), (1, -4, "no depth map")):
            try:
                call(idx)
            except error as ex:
                assert "pmhip error %d" % code in str(ex) and word in str(ex) and "pmhip_" + name in str(ex), str(ex)
            else:
                raise AssertionError("%s(%d) was accepted" % (name, idx))
        call(0)                                                                                # the engine stays usable
    lib, hnd = e._lib, e._h
    assert lib.pmhip_scene_depth_image(hnd, 0, 0.0, 1.0, None, None) == -1 and lib.pmhip_scene_normal_image(hnd, 0, None) == -1
    assert lib.pmhip_scene_conf_image(hnd, 0, None, None, None) == -1 and lib.pmhip_scene_view_cloud(hnd, 0, 1, None, 0, None) == -1
    assert lib.pmhip_x84_threshold(hnd, None, 4, 5.2, np.zeros(4, f32)) == -1 and lib.pmhip_depth_image(hnd, d, 0, 3, 0.0, 1.0, np.zeros(3, np.uint8), None) == -1
    assert lib.pmhip_export_get_stats(hnd, None) == -1
    same_image(e.scene_depth_image(0, 0.0, 8.0)[0], mx.depth_map_to_image(d, 0.0, 8.0)[0], "after the refusals")
    s = e.export_stats()
    assert s["launches"] == 1 and s["quantum"] > 0 and s["grid_cap"] > 0


def scale_needs_a_cloud_and_cameras(e, error):
    e.scene_create(2, 21, 9, 0)
    e.scene_set_view(0, np.zeros((9, 21), f32), K0, R0, C0, 0.1, 100.0, [1])
    e.scene_cloud_set(np.array([[0, 0, 5.0]], f32), np.array([0, 1], np.uint32), np.array([1], np.uint32))
    try:
        e.scene_cloud_scale(1.0)
    except error as ex:
        assert "pmhip error -4" in str(ex) and "without a camera" in str(ex), str(ex)
    else:
        raise AssertionError("a view without a camera was accepted")
    e.scene_cloud_set(np.array([[0, 0, 5.0]], f32), np.array([0, 1], np.uint32), np.array([0], np.uint32))
    scale, conf = e.scene_cloud_scale(2.0)
    want = mx.point_scales(np.array([[0, 0, 5.0]], f32), [0, 1], [0], None, [K0], [R0], [C0], 2.0)
    same_bits(scale, want[0], "one point"); assert conf.tolist() == [1.0]


# ---- routes --------------------------------------------------------------------------------------------------------------------------------------------------------------
def route_options(light=True):
    from openmvs_amd import optdense
    opt = optdense.defaults()
    opt.nResolutionLevel = 3; opt.nMinResolution = 40; opt.nNumViews = 2; opt.nEstimateNormals = 2; opt.nEstimationGeometricIters = 0; opt.nSpeckleSize = 20
    if light:                                                                                  # the emulator: one level, one sweep -- the estimation is not what the case is about
        opt.nSubResolutionLevels = 0; opt.nEstimationIters = 1
    return opt


def dense_reconstruction_case(e, mvs, tmp_dir, light=True):
    """`densify.dense_reconstruction(export_level=5, ply_out=...)` on the pipeline-test scene at 80 x 60: the file set of verbosity 5, every image the twin of the resident
    maps, the per-view and final PLY files what the writers make of the resident data."""
    from PIL import Image
    from openmvs_amd import densify, plyio
    out = os.path.join(str(tmp_dir), "out")
    ply = os.path.join(out, "scene_dense")
    seen = {}
    real = densify.export_view_files

    def spy(engine, scene, ids, out_dir, level=3, tag="", image_saver=None):
        for v in ids:                                                                          # the resident maps at the moment of each export
            seen[(int(v), tag)] = engine.scene_get_maps(v)
        return real(engine, scene, ids, out_dir, level, tag, image_saver)

    densify.export_view_files = spy
    try:
        sv, cloud = densify.dense_reconstruction(e, mvs, None, route_options(light), seed=3, export_level=5, export_dir=out, ply_out=ply)
    finally:
        densify.export_view_files = real
    assert sv.ids == [0, 1, 2, 3] and cloud["nPoints"] > 0
    names = sorted(os.listdir(out))
    want_names = ["scene_dense.ply"]
    for v in sv.ids:
        d, n, c = seen[(v, "")]
        fd = seen[(v, "filtered")][0]
        want_names += ["depth%04d.%s" % (v, s) for s in ("raw.png", "png", "conf.png", "conf.pfm", "normal.png")]
        want_names += ["depth%04d.ply" % v] * bool((d > 0).any()) + ["depth%04d.filtered.png" % v] + ["depth%04d.filtered.ply" % v] * bool((fd > 0).any())
        assert (d > 0).any() and (c > 0).any()

        def png(s):
            return np.asarray(Image.open(os.path.join(out, "depth%04d.%s" % (v, s))))

        same_image(png("raw.png"), mx.depth_map_to_image(seen[(v, "raw")][0])[0], "depth%04d.raw.png" % v)
        same_image(png("png"), mx.depth_map_to_image(d)[0], "depth%04d.png" % v)
        same_image(png("conf.png"), mx.conf_map_to_image(c)[0], "depth%04d.conf.png" % v)
        same_image(png("normal.png"), mx.normal_map_to_image(n), "depth%04d.normal.png" % v)
        same_image(png("filtered.png"), mx.depth_map_to_image(fd)[0], "depth%04d.filtered.png" % v)
        raw = open(os.path.join(out, "depth%04d.conf.pfm" % v), "rb").read()
        head = b"Pf\n%d %d\n-1.000000\n" % (c.shape[1], c.shape[0])
        assert raw.startswith(head)
        same_bits(np.frombuffer(raw[len(head):], "<f4").reshape(c.shape)[::-1], c, "depth%04d.conf.pfm" % v)
        rec = mx.view_point_cloud(sv.K[v], sv.R[v], sv.C[v], d, n, sv.bgr[v])
        body = open(os.path.join(out, "depth%04d.ply" % v), "rb").read()
        assert body.endswith(rec.tobytes()) and (b"element vertex %d\n" % len(rec)) in body[:200] and b"property float32 nx\n" in body[:300], "depth%04d.ply" % v
        final = e.scene_get_maps(v)
        same_bits(final[0], fd, "the last export saw the final depth map of view %d" % v)
    assert names == sorted(want_names), (names, sorted(want_names))
    back = plyio.load_point_cloud(ply + ".ply")
    res = e.scene_cloud_get()
    assert res["nPoints"] == cloud["nPoints"]
    same_bits(np.c_[back["x"], back["y"], back["z"]], res["points"], "scene_dense.ply points")
    same_bits(np.c_[back["nx"], back["ny"], back["nz"]], res["normals"], "scene_dense.ply normals")
    assert np.array_equal(np.c_[back["blue"], back["green"], back["red"]], res["colors"])
    cnt = np.diff(res["viewStart"].astype(np.int64))
    assert np.array_equal(back["view_indices"][0], cnt) and np.array_equal(back["view_indices"][1], res["views"])
    assert np.array_equal(back["view_weights"][0], cnt)
    same_bits(back["view_weights"][1], res["weights"], "scene_dense.ply weights")
    return sv, cloud


def mesh_png_case(e, mvs, tmp_dir):
    """`export_mesh_depth_maps(..., "x.png", engine=e)`: one PNG per image, the twin of `views.project_mesh`'s depth map.  The image is the engine's work: without an
    engine, and for a name that is no image's, the call raises as before."""
    from PIL import Image
    from openmvs_amd import densify, views
    from tests import mesh_project_cases as mcases
    V, F = mcases.scene_mesh(mvs)
    sv = densify.load_scene(mvs, opt=route_options())
    files = densify.export_mesh_depth_maps(sv, (V, F), os.path.join(str(tmp_dir), "dev.png"), engine=e)
    assert [os.path.basename(f) for f in files] == ["dev%04d.png" % i for i in range(4)]
    for i, f in enumerate(files):
        w, h = sv.sizes[i]
        d = views.project_mesh(sv.K[i], sv.R[i], sv.C[i], w, h, V, F)[0]
        assert (d > 0).mean() > 0.2
        same_image(np.asarray(Image.open(f)), mx.depth_map_to_image(d)[0], f)
    saved = []
    densify.export_mesh_depth_maps(sv, (V, F), os.path.join(str(tmp_dir), "hook.PNG"), engine=e, image_saver=lambda path, a: saved.append((os.path.basename(path), a)))
    assert [n for n, _ in saved] == ["hook%04d.PNG" % i for i in range(4)] and all(np.array_equal(a, np.asarray(Image.open(f))) for (_, a), f in zip(saved, files))
    for name, eng in (("host.png", None), ("x.bak", e), ("x", e)):
        try:
            densify.export_mesh_depth_maps(sv, (V, F), os.path.join(str(tmp_dir), name), engine=eng)
        except ValueError as ex:
            assert "extension" in str(ex)
        else:
            raise AssertionError("%s was accepted" % name)
    assert not [f for f in os.listdir(str(tmp_dir)) if f.startswith(("host", "x"))]
