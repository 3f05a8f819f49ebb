"""The cases of the device rectification (sgmhip_rectify_pair and the calls around it), shared by the device suite (tests/test_zz_gpu_sgm_rectify.py)
and the emulator suite (tests/test_emu_sgm_rectify.py).

The reference is the host code the kernel replaces -- `rectify.warp_perspective_u8` followed by `sgm_pipeline.to_gray_linear` -- so equality is exact
(`np.array_equal`, gray compared as uint32 views): there is no tolerance.  Sources are seeded random 8-bit images, so every bit of every tap matters.
Every homography keeps Z > 0 over the whole destination (asserted in `_case`; Z is linear in (x, y), so the four corners decide).  A reference is
computed once per case and shared (`reference`); nothing changes it."""
import functools
import os

import numpy as np

from openmvs_amd import rectify, sgm_pipeline

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "data", "scene")


def _T(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def _S(s):
    return np.diag([s, s, 1.0])


def _R(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _P(a, b):
    return np.array([[1, 0, 0], [0, 1, 0], [a, b, 1]], np.float64)


def source_positions(H, size):
    """(X, Y, Z) of `warp_perspective_u8` for every destination pixel: its own expressions."""
    w, h = size
    Hi = np.linalg.inv(H)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    Z = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
    return (Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]) / Z, (Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]) / Z, Z


def _case(name, seed, size_l, size_r, H1, H2, size):
    """size_*: (w, h) of the two sources; H*: source -> destination, as `warp_perspective_u8` takes them; size: (w, h) of the destination."""
    rng = np.random.default_rng(seed)
    src = [rng.integers(0, 256, (s[1], s[0], 3), dtype=np.uint8) for s in (size_l, size_r)]
    Hs = [np.ascontiguousarray(H1, np.float64), np.ascontiguousarray(H2, np.float64)]
    for H in Hs:
        Hi = np.linalg.inv(H)
        for x, y in ((0, 0), (size[0] - 1, 0), (0, size[1] - 1), (size[0] - 1, size[1] - 1)):
            assert Hi[2, 0] * x + Hi[2, 1] * y + Hi[2, 2] > 0, name
    return dict(name=name, src=src, H=Hs, size=size)


def _outside(c, side):
    X, Y, _ = source_positions(c["H"][side], c["size"])
    H0, W0 = c["src"][side].shape[:2]
    return (X <= -1).any(), (X >= W0).any(), (Y <= -1).any(), (Y >= H0).any()


def _build():
    cs = []
    cs.append(_case("identity", 1, (64, 48), (64, 48), np.eye(3), np.eye(3), (64, 48)))
    # X = x - 0.5: every weight is 1/2, sums of four taps end in .25 / .5 / .75 (the ties of floor(v + 0.5)); X = x + 3.25 runs past W0
    cs.append(_case("translation", 2, (77, 45), (77, 45), _T(0.5, 0.5), _T(-3.25, 2.75), (77, 45)))
    # whole-pixel shifts put destination pixels exactly on X = -1, Y = -1, X = W0 and Y = H0: the borders of the tap test and of the mask
    cs.append(_case("translation_whole_pixels", 3, (77, 45), (77, 45), _T(2, 1), _T(-2, -1), (77, 45)))
    c = _case("rotation_perspective_shift", 4, (61, 47), (90, 40),
              _T(38, 22) @ _R(2.0) @ _P(1e-5, -1.2e-5) @ _T(-30.3, -23.6), _T(38.4, 22.1) @ _R(-2.0) @ _P(-0.9e-5, 1.1e-5) @ _T(-52.7, -19.2), (77, 45))
    o = [_outside(c, 0), _outside(c, 1)]
    assert all(o[0][k] or o[1][k] for k in range(4)) and sum(o[0]) >= 2 and sum(o[1]) >= 2, o       # every side is left on at least one source
    cs.append(c)
    c = _case("magnify_minify", 5, (80, 45), (200, 110), _T(0.4, -0.3) @ _S(1.7), _T(6.2, 2.0) @ _S(0.6), (130, 70))
    assert all(_outside(c, 1))                                     # x 0.6: the destination covers more than the source, on all four sides
    cs.append(c)
    cs.append(_case("wide_2050x3", 6, (2052, 4), (1500, 5), _T(-0.3, -0.4), _T(3.5, -0.7) @ _S(1.37) @ _R(0.05), (2050, 3)))     # > 2048 columns, w % 4 == 2
    cs.append(_case("tall_3x300", 7, (4, 301), (5, 260), _T(-0.6, -0.2), _T(-0.8, 2.3) @ _S(1.15) @ _R(-0.1), (3, 300)))
    cs.append(_case("source_1x1", 8, (1, 1), (1, 1), _T(1.5, 1.25), _T(2.0, 1.0) @ _S(1.6), (5, 4)))
    return cs


CASES = _build()
NAMES = [c["name"] for c in CASES]
_REF = {}


def reference(c):
    """[(bgr, gray, mask) of the left image, ... of the right image] by the host code; computed once per case."""
    if c["name"] not in _REF:
        out = []
        for side in (0, 1):
            bgr, mask = rectify.warp_perspective_u8(c["src"][side], c["H"][side], c["size"])
            gray = sgm_pipeline.to_gray_linear(bgr)
            for a in (bgr, gray, mask):
                a.setflags(write=False)
            out.append((bgr, gray, mask))
        _REF[c["name"]] = out
    return _REF[c["name"]]


def same_bits(m, c):
    """Rectify case `c` on matcher `m` and compare the three maps of both sides with the host code, bit for bit."""
    ref = reference(c)
    m.scene_set_images(c["src"])
    m.rectify_pair(0, 1, np.linalg.inv(c["H"][0]), np.linalg.inv(c["H"][1]), c["size"], sgm_pipeline._srgb_table())
    w, h = c["size"]
    for side in (0, 1):
        bgr, gray, mask = m.rectified(side)
        rb, rg, rm = ref[side]
        assert bgr.shape == (h, w, 3) and gray.shape == (h, w) and mask.shape == (h, w) and rg.dtype == np.float32
        assert np.array_equal(bgr, rb), (c["name"], side, "bgr", int((bgr != rb).any(-1).sum()))
        assert np.array_equal(mask, rm), (c["name"], side, "mask", int((mask != rm).sum()))
        assert np.array_equal(gray.view(np.uint32), rg.view(np.uint32)), (c["name"], side, "gray", int((gray.view(np.uint32) != rg.view(np.uint32)).sum()))
    if c["name"] == "identity":
        for side in (0, 1):
            bgr, _, mask = m.rectified(side, gray=False)
            assert np.array_equal(bgr, c["src"][side]) and (mask == 255).all()
    if c["name"] == "source_1x1":
        assert ref[0][0].any() and ref[1][0].any() and not ref[0][2].all()          # the one pixel is seen, and not everywhere
    # partial downloads: any pointer may be NULL
    b, g, k = m.rectified(1, bgr=False, mask=False)
    assert b is None and k is None and np.array_equal(g.view(np.uint32), ref[1][1].view(np.uint32))


def errors_leave_the_engine_usable(m, error):
    """An unset index, an index beyond the table, a match before any rectification, a size that is no multiple of 2^levels: each is an exception with
    a message, and the engine works afterwards.  m: an engine that has not rectified a pair yet."""
    c = CASES[NAMES.index("translation")]
    table = sgm_pipeline._srgb_table()
    inv = [np.linalg.inv(H) for H in c["H"]]
    m.scene_set_images([c["src"][0], None, c["src"][1]])
    with_message = lambda e, *words: all(wd in str(e.value) for wd in words) and len(str(e.value)) > 20
    import pytest
    with pytest.raises(error) as e:
        m.tsgm_match_rectified(min_resolution=32)
    assert with_message(e, "no rectified pair")
    with pytest.raises(error) as e:
        m.rectified(0)
    assert with_message(e, "no rectified pair")
    with pytest.raises(error) as e:
        m.rectify_pair(0, 1, inv[0], inv[1], c["size"], table)
    assert with_message(e, "1", "never set")
    with pytest.raises(error) as e:
        m.rectify_pair(0, 3, inv[0], inv[1], c["size"], table)
    assert with_message(e, "3", "outside the scene table")
    with pytest.raises(error) as e:
        m.rectify_pair(-1, 2, inv[0], inv[1], c["size"], table)
    assert with_message(e, "outside the scene table")
    for size in ((0, 45), (77, -1)):
        with pytest.raises(error) as e:
            m.rectify_pair(0, 2, inv[0], inv[1], size, table)
        assert with_message(e, "positive")
    with pytest.raises(error) as e:                                    # none of the refused calls left a pair behind
        m.tsgm_match_rectified(min_resolution=32)
    assert with_message(e, "no rectified pair")
    m.rectify_pair(0, 2, inv[0], inv[1], c["size"], table)             # 77 x 45: one halving at minResolution 32, and neither extent is even
    with pytest.raises(error) as e:
        m.tsgm_match_rectified(min_resolution=32)
    assert with_message(e, "multiple of 2^levels")
    # ... and the engine is usable: the pair is still resident, and a fitting crop of it matches like the uploaded images do
    ref = reference(c)
    assert np.array_equal(m.rectified(1)[0], ref[1][0])
    m.rectify_pair(0, 2, inv[0], inv[1], (76, 44), table)
    d, k, levels = m.tsgm_match_rectified(min_resolution=32)
    crop = lambda a: np.ascontiguousarray(a[:44, :76])
    d2, k2, levels2 = m.tsgm_match(crop(ref[0][0]), crop(ref[1][0]), crop(ref[0][1]), crop(ref[1][1]), crop(ref[0][2]), crop(ref[1][2]), min_resolution=32)
    assert levels == levels2 == 2 and d.shape == (38, 70) and np.array_equal(d, d2) and np.array_equal(k, k2)
    m.scene_clear()
    with pytest.raises(error) as e:
        m.rectify_pair(0, 2, inv[0], inv[1], c["size"], table)
    assert with_message(e, "outside the scene table")


# ---- the pipeline on tests/data/scene -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_scene(level):
    """tests/data/scene at 1 / 2^level of its resolution -> (scene, cameras, BGR images, per-image visibility of the sparse points)."""
    from openmvs_amd import densify, mvsi, optdense, views
    mvs = os.path.join(SCENE, "scene.mvs")
    sc = mvsi.load(mvs)
    if level == 0:                                                 # the files as they are (640 x 479), as tests/test_sgm_real.py reads them
        from PIL import Image
        cams = views.Cameras(sc)
        bgr = [np.ascontiguousarray(np.asarray(Image.open(os.path.join(SCENE, im.name)).convert("RGB"))[..., ::-1]) for im in sc.images]
    else:
        opt = optdense.defaults()
        opt.nResolutionLevel = level; opt.nMinResolution = 80
        sv = densify.load_scene(mvs, opt=opt)
        cams = views.Cameras(sc, sv.sizes[:len(sc.images)])
        bgr = sv.bgr
    own = np.repeat(np.arange(len(sc.vertices)), np.diff(sc.vertex_view_start)); ids = sc.vertex_views["image_id"]
    seen = []
    for i in range(len(sc.images)):
        s = np.zeros(len(sc.vertices), bool); s[own[ids == i]] = True; seen.append(s)
    return sc, cams, bgr, seen


def real_pair_case(A=0, B=2):
    """The test scene's images at their full size (640 x 479) under the rectifying homographies of a real pair (`rectify.stereo_rectify_geometry`)."""
    sc, cams, bgr, seen = load_scene(0)
    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    X = sc.vertices[seen[A] & seen[B]]
    g = rectify.stereo_rectify_geometry((bgr[A].shape[1], bgr[A].shape[0]), *cam(A), (bgr[B].shape[1], bgr[B].shape[0]), *cam(B),
                                        sgm_pipeline.world_to_image3(*cam(A), X), sgm_pipeline.world_to_image3(*cam(B), X))
    assert g is not None and bgr[A].shape == (479, 640, 3) and min(g["size"]) > 300
    c = dict(name="real_pair_%d_%d" % (A, B), src=[bgr[A], bgr[B]], H=[np.ascontiguousarray(g["H1"]), np.ascontiguousarray(g["H2"])], size=g["size"])
    for H in c["H"]:
        assert source_positions(H, c["size"])[2].min() > 0
    return c


def match_pair_routes_agree(matcher, level, min_resolution, A=0, B=2):
    """`match_pair` of pair (A, B) by the device route (resident images, sgmhip_rectify_pair, sgmhip_tsgm_match_rectified) and by the host route."""
    sc, cams, bgr, seen = load_scene(level)
    cam = lambda i: (cams.K[i], cams.R[i], cams.C[i])
    X = sc.vertices[seen[A] & seen[B]]
    host = sgm_pipeline.match_pair(sgm_pipeline.DeviceBackend(matcher, None, rectify_on_device=False), bgr[A], cam(A), bgr[B], cam(B), X, min_resolution=min_resolution)
    be = sgm_pipeline.DeviceBackend(matcher, None)
    be.scene_set_images(bgr)
    ignored = sgm_pipeline.match_pair(be, bgr[A], cam(A), bgr[B], cam(B), X, min_resolution=min_resolution)      # no indices: the host route, whatever the backend can do
    dev = sgm_pipeline.match_pair(be, bgr[A], cam(A), bgr[B], cam(B), X, min_resolution=min_resolution, image_ids=(A, B))
    assert (dev["disparity"] != 32767).mean() > 0.3
    for other in (host, ignored):
        for k in ("disparity", "cost", "H", "Q"):
            assert np.array_equal(dev[k], other[k]), k
        assert dev["image_size"] == other["image_size"] and dev["subpixel_steps"] == other["subpixel_steps"]
    be.scene_clear()
    return dev


def dense_reconstruction_routes_agree(matcher, tmp_path):
    """`dense_reconstruction(..., -1)` at the quarter-size options of test_sgm_modes_of_dense_reconstruction with the rectification on the device and on the
    host: the same files with the same bytes, and every image uploaded exactly once."""
    from openmvs_amd import optdense
    opt = optdense.defaults()
    opt.nResolutionLevel = 2; opt.nMinResolution = 80; opt.nNumViews = 2; opt.nEstimateNormals = 2; opt.fViewMinScore = 0.0
    mvs = os.path.join(SCENE, "scene.mvs")
    dirs = {}
    for on_device in (True, False):
        d = str(tmp_path / ("device" if on_device else "host"))
        before = matcher.image_uploads
        done = sgm_pipeline.dense_reconstruction(sgm_pipeline.DeviceBackend(matcher, None, rectify_on_device=on_device), mvs, d, -1, opt, min_resolution=40)
        assert 4 <= len(done) <= 6 and sorted(os.listdir(d)) == sorted(sgm_pipeline.pair_file_name(a, b) for a, b in done)
        assert matcher.image_uploads - before == (4 if on_device else 0)            # four images, each sent once for all its pairs
        dirs[on_device] = d
    names = sorted(os.listdir(dirs[True]))
    assert names == sorted(os.listdir(dirs[False]))
    for n in names:
        with open(os.path.join(dirs[True], n), "rb") as a, open(os.path.join(dirs[False], n), "rb") as b:
            assert a.read() == b.read(), n
    before = matcher.image_uploads
    assert sgm_pipeline.dense_reconstruction(sgm_pipeline.DeviceBackend(matcher, None), mvs, dirs[True], -1, opt, min_resolution=40) == []
    assert matcher.image_uploads == before                                         # nothing to match: nothing uploaded
