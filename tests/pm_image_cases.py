"""Cases of the engine's image store (csrc/pm_image.hip, csrc/pm_host_image.hip; include/pmhip.h section 2b), shared by the emulator suite (tests/test_emu_pm_image.py)
and the device suite (tests/test_zz_gpu_pm_image.py).  The reference is the host code the store replaces -- densify._resize_area_u8, views.to_gray,
densify.scale_image, and the host route of densify.load_scene -- and every comparison is exact."""
import functools
import os

import numpy as np
import pytest

from openmvs_amd import densify, optdense, patchmatch, views

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


# ---- the working size ---------------------------------------------------------------------------------------------------------------------------------
def working_sizes_equal_the_host_rule():
    def host(W, H, level, lo, hi):
        res, _ = views.compute_max_resolution(W, H, level, lo, hi)
        return views.resized_size(W, H, res)
    assert patchmatch.working_size(640, 479, 1, 160, 3200) == host(640, 479, 1, 160, 3200) == (320, 240)
    assert patchmatch.working_size(6000, 4000, 1, 640, 2560) == host(6000, 4000, 1, 640, 2560) == (2560, 1707)
    n = 0
    for W, H in ((640, 479), (479, 640), (6000, 4000), (4000, 3000), (3000, 2000), (1, 1), (7, 5), (1921, 1081), (333, 1000), (5, 5), (4001, 3001)):
        for level in (0, 1, 2, 3, 6, 40):
            for lo in (0, 40, 160, 640, 5000):
                for hi in (0, 100, 1280, 2560, 3200):
                    assert patchmatch.working_size(W, H, level, lo, hi) == host(W, H, level, lo, hi), (W, H, level, lo, hi)
                    n += 1
    assert n == 11 * 6 * 5 * 5


def scaled_sizes_equal_need_scale_image():
    f32 = np.float32
    for W, H in ((13, 9), (67, 131), (640, 479)):
        for s in (f32(0.85), f32(1.15), f32(1.0), f32(0.9), f32(1.1)):
            assert not densify.need_scale_image(s) and patchmatch.scaled_size(W, H, s) is None, s
        for s in (0.84, 1.16, 0.5, 0.25, f32(1.0 / 3.0), 0.8, 0.6, 1.2, 1.7):
            s = float(f32(s))
            assert densify.need_scale_image(s) and patchmatch.scaled_size(W, H, s) == (int(np.rint(W * s)), int(np.rint(H * s))), s


# ---- resize + gray ------------------------------------------------------------------------------------------------------------------------------------
def _ties_image():
    """16 x 8, 4 x 4 blocks whose sums are 8, 24 (channel 0), 24, 8 (channel 1) and 40, 56 (channel 2): sum / 16 = 0.5, 1.5, 2.5, 3.5 -- round half to even gives 0, 2, 2, 4."""
    img = np.zeros((8, 16, 3), np.uint8)
    for by in range(2):
        for bx in range(4):
            odd = (bx + by) & 1
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            blk[:2, :, 0] = 3 if odd else 1          # eight pixels: 24 / 8
            blk[:2, :, 1] = 1 if odd else 3
            blk[1:3, :, 2] = 7 if odd else 5         # 56 / 40
    return img


def _all_bytes_image():
    """256 x 3: every byte value in each channel, in three different pairings."""
    i = np.arange(256)
    img = np.zeros((3, 256, 3), np.uint8)
    for r in range(3):
        img[r, :, 0] = (i + 85 * r) % 256
        img[r, :, 1] = (i * 7 + 13 + 31 * r) % 256
        img[r, :, 2] = 255 - (i * 3 + r) % 256
    assert all(len(set(img[:, :, c].ravel().tolist())) == 256 for c in range(3))
    return img


def _random_u8(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


#            name                source (W, H)   destination   channel orders
RESIZE = [("halving",            (8, 6),         (4, 3),       (1, 0)),
          ("integer_3_2",        (12, 10),       (4, 5),       (1, 0)),
          ("ties_to_even",       (16, 8),        (4, 2),       (1,)),
          ("general_7x5",        (7, 5),         (3, 2),       (1, 0)),
          ("general_just_above", (13, 9),        (12, 8),      (1,)),
          ("general_131x67",     (131, 67),      (57, 29),     (1,)),
          ("one_row",            (300, 3),       (127, 1),     (1,)),
          ("one_column",         (3, 300),       (1, 127),     (1,)),
          ("scene_640x479",      (640, 479),     (320, 240),   (1,)),
          ("no_resize",          (9, 9),         (9, 9),       (1, 0)),
          ("all_bytes",          (256, 3),       (256, 3),     (1,))]
RESIZE_NAMES = [c[0] for c in RESIZE]
FULL_SIZE = [("full_4000x3000_halved", (4000, 3000), (2000, 1500), (1,)), ("full_3000x2000_general", (3000, 2000), (1280, 853), (1,))]      # device only


def _source(name, size, seed):
    if name == "ties_to_even":
        return _ties_image()
    if name == "all_bytes":
        return _all_bytes_image()
    return _random_u8(size[0], size[1], seed)


def host_prepare(img, w, h, channel_order):
    """(gray, bgr) of the host route: Image::ResizeImage, then toGray and the B, G, R image."""
    rgb = img if channel_order == 1 else np.ascontiguousarray(img[..., ::-1])
    if (w, h) != (rgb.shape[1], rgb.shape[0]):
        rgb = densify._resize_area_u8(rgb, w, h)
    return views.to_gray(rgb), np.ascontiguousarray(rgb[..., ::-1])


def resize_equals_the_host_code(e, case, key=3):
    name, size, (w, h), orders = case
    img = _source(name, size, seed=RESIZE_NAMES.index(name) if name in RESIZE_NAMES else 99)
    assert img.shape == (size[1], size[0], 3)
    for order in orders:
        gray, bgr = host_prepare(img, w, h, order)
        e.image_prepare(key, img, w, h, channel_order=order)
        g, b = e.image_get(key)
        assert g.shape == (h, w) and b.shape == (h, w, 3)
        assert np.array_equal(b, bgr), (name, order, "bgr", int((b != bgr).sum()))
        assert np.array_equal(g.view(np.uint32), gray.view(np.uint32)), (name, order, "gray", int((g != gray).sum()))
    if name == "ties_to_even":
        assert sorted(set(b.ravel().tolist())) == [0, 2, 4]
    e.image_drop(key)


# ---- ScaleImage ---------------------------------------------------------------------------------------------------------------------------------------
SCALES = [0.5, 0.25, float(np.float32(1.0 / 3.0)), 0.8, 0.6, 1.2, 1.7, 0.84, 1.16]
SCALE_SOURCES = [(13, 9), (67, 131)]


def scale_image_equals_the_host_code(e, size, error):
    W, H = size
    rgb = _random_u8(W, H, seed=W)
    e.image_prepare(0, rgb, W, H)
    gray = e.image_get(0)[0]
    assert np.array_equal(gray, views.to_gray(rgb))
    for s in SCALES:
        ref = densify.scale_image(gray, s)
        assert ref is not None
        w, h = e.image_scale(1, 0, s)
        got, none = e.image_get(1)
        assert none is None and (w, h) == (ref.shape[1], ref.shape[0]) == got.shape[::-1], (s, w, h, ref.shape)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (size, s, int((got != ref).sum()), float(np.abs(got - ref).max()))
    third = float(np.float32(1.0 / 3.0))
    assert abs(1.0 / third - 3) > np.finfo(np.float64).eps                       # float(1/3): the table path, not the block path
    for s in (np.float32(0.85), np.float32(1.15)):                                # NeedScaleImage is false: not resampled
        assert densify.scale_image(gray, s) is None
        with pytest.raises(error) as x:
            e.image_scale(1, 0, s)
        assert "15 %" in str(x.value)
    assert np.array_equal(e.image_get(0)[0], gray)                                # the source is untouched, the engine usable
    e.image_drop(-1)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------------
def errors_leave_the_engine_usable(e, error):
    """Every refusal of include/pmhip.h section 2b, each followed by a call that succeeds on the same engine.  (`a source without gray` is checked in the library, but no
    call of the ABI makes such an entry: every entry has a gray image.)"""
    from openmvs_amd import synth
    img = _random_u8(12, 10, seed=5)
    ok = lambda: resize_equals_the_host_code(e, RESIZE[0], key=7)

    def refused(call, words):
        with pytest.raises(error) as x:
            call()
        assert words in str(x.value), str(x.value)
        ok()
    refused(lambda: e.image_prepare(0, img, 13, 10), "shrinking only")          # enlarging
    refused(lambda: e.image_prepare(0, img, 12, 11), "shrinking only")
    refused(lambda: e.image_prepare(0, img, 0, 5), "at least 1 x 1")
    refused(lambda: e.image_prepare(0, img, 6, -1), "at least 1 x 1")
    refused(lambda: e.image_get(5), "unknown key")
    refused(lambda: e.image_scale(1, 5, 0.5), "unknown source key")
    refused(lambda: e.image_drop(5), "unknown key")
    e.image_prepare(0, img, 12, 10)
    refused(lambda: e.image_scale(1, 0, 1.1), "15 %")
    refused(lambda: e.image_scale(1, 0, 0.9), "15 %")
    refused(lambda: e.image_scale(1, 0, 0.01), "leaves no image")
    # a scene: views adopt entries by key; an unknown key and an entry below the engine's minimum size are refused
    sc = synth.make_scene(3, 48, 40, n_src=2)
    e.scene_create(3, 48, 40, 1)
    cam = lambda i: (sc.K[i], sc.R[i], sc.C[i], float(sc.dmin[i]), float(sc.dmax[i]), sc.neighbors[i])
    refused(lambda: e.scene_set_view_stored(0, 5, *cam(0)), "unknown key")
    e.image_prepare(2, img, 2, 2)
    refused(lambda: e.scene_set_view_stored(0, 2, *cam(0)), "at least 3 x 3")
    refused(lambda: e.scene_set_view_stored(9, 0, *cam(0)), "no such view")
    e.scene_set_view_stored(0, 0, *cam(0))                                       # 12 x 10 in a 48 x 40 scene: a view with its own size
    assert e.view_size(0) == (12, 10)
    before = e.image_bytes()
    assert before > 0 and e.scene_bytes() > 0
    e.scene_create(3, 48, 40, 1)                                                 # the store survives a new scene ...
    assert e.image_bytes() == before and np.array_equal(e.image_get(0)[1], host_prepare(img, 12, 10, 1)[1])
    e.Release()                                                                  # ... and goes with pmhip_release
    assert e.image_bytes() == 0
    refused(lambda: e.image_get(0), "unknown key")
    e.image_drop(-1)
    assert e.image_bytes() == 0


# ---- the scene front end ------------------------------------------------------------------------------------------------------------------------------
def _opt(level, min_resolution):
    opt = optdense.defaults()
    opt.nResolutionLevel = level; opt.nMinResolution = min_resolution; opt.nNumViews = 8; opt.nEstimateNormals = 2; opt.nSpeckleSize = 20
    return opt


def _pil(p):
    from PIL import Image
    with Image.open(p) as im:
        return np.asarray(im.convert("RGB"))


def shrunk_loader(p):
    """Image 1 at 0.6 of its size through a plain index shrink: its neighbours see it at another scale (ViewData::ScaleImage on both sides)."""
    rgb = _pil(p)
    if os.path.basename(p) != "00001.jpg":
        return rgb
    H, W = rgb.shape[:2]
    ys = (np.arange(int(H * 0.6)) / 0.6).astype(np.int64); xs = (np.arange(int(W * 0.6)) / 0.6).astype(np.int64)
    return np.ascontiguousarray(rgb[ys][:, xs])


@functools.lru_cache(maxsize=None)
def host_scene(level, min_resolution, mixed):
    """The host route's SceneViews, computed once and shared (read only)."""
    return densify.load_scene(SCENE, opt=_opt(level, min_resolution), image_loader=shrunk_loader if mixed else None)


def scene_image(e, slot, device):
    """The gray image the scene holds for a slot (pmhip_scene_copy, what = 0)."""
    import torch
    w, h = e.view_size(slot)
    t = torch.empty((h, w), dtype=torch.float32, device=device)
    e.scene_copy(0, slot, 1, t.data_ptr(), False)
    e.sync()
    return t.cpu().numpy()


def same_views(a, b):
    assert a.ids == b.ids and a.sizes == b.sizes and (a.width, a.height) == (b.width, b.height) and a.alias_of == b.alias_of and a.names == b.names
    assert len(a.gray) == len(b.gray) == len(a.bgr) + len(a.alias_of) == len(b.bgr) + len(b.alias_of)
    for k in ("K", "R", "C", "dmin", "dmax", "neighbors", "estimate_neighbors"):
        assert len(getattr(a, k)) == len(getattr(b, k)) and all(np.array_equal(x, y) for x, y in zip(getattr(a, k), getattr(b, k))), k
    assert a.init_depth.keys() == b.init_depth.keys() and all(np.array_equal(a.init_depth[i], b.init_depth[i]) and np.array_equal(a.init_normal[i], b.init_normal[i]) for i in a.init_depth)


def scene_routes_hold_the_same_images(new_engine, device, level, min_resolution, size, mixed=False, estimate=False):
    """`load_scene` + `scene_load` by both routes: the same slots, sizes and cameras, the same stored and resident images; with `estimate` also the same final depth maps."""
    host = host_scene(level, min_resolution, mixed)
    assert (host.width, host.height) == size
    e = new_engine()
    try:
        dev = densify.load_scene(SCENE, opt=_opt(level, min_resolution), image_loader=shrunk_loader if mixed else None, engine=e)
        same_views(dev, host)
        n = len(host.gray)
        assert all(g is None for g in dev.gray) and all(b is None for b in dev.bgr) and dev.stored == {i: i for i in range(n)} and not host.stored
        assert e.image_stats()["prepared"] == 4 and e.image_stats()["scaled"] == len(host.alias_of)             # one upload per image
        if mixed:
            up = sorted(a for a, j in host.alias_of.items() if j == 1); down = sorted(a for a, j in host.alias_of.items() if j != 1)
            assert len(up) == 3 and len(down) == 3 and sorted(host.alias_of[a] for a in down) == [0, 2, 3]
            assert all(host.sizes[a][0] > host.sizes[1][0] * 1.5 for a in up) and all(host.sizes[a][0] < host.sizes[0][0] * 0.65 for a in down)
            assert host.sizes[1] != size and host.sizes[0] == size
        else:
            assert not host.alias_of
        for i in range(n):
            g, b = e.image_get(dev.stored[i])
            assert np.array_equal(g.view(np.uint32), host.gray[i].view(np.uint32)), ("stored gray", i)
            assert (b is None and i >= len(host.bgr)) or np.array_equal(b, host.bgr[i]), ("stored colour", i)
        e.scene_load(dev, n_levels=1)
        assert e.image_bytes() == 0 and all(e.view_size(i) == tuple(host.sizes[i]) for i in range(n))          # the entries are gone, and the staging with the last of them
        resident = [scene_image(e, i, device) for i in range(n)]
        for i in range(n):
            assert np.array_equal(resident[i].view(np.uint32), host.gray[i].view(np.uint32)), ("resident gray", i)
        if not estimate:
            return
        opt = _opt(level, min_resolution)
        opt.nSubResolutionLevels = 1; opt.nEstimationGeometricIters = 1; opt.nEstimationIters = 2
        # (no per-map or cross-view filters: at 80 x 60 they leave next to nothing of this scene, and the comparison would be one of empty maps)
        run = lambda eng, sv: densify.compute_depth_maps(eng, sv.ids, opt.params(3), n_optimize=0, init_depth=sv.init_depth, init_normal=sv.init_normal, scene=sv)
        run(e, dev)
        got = {v: e.scene_get_maps(v) for v in dev.ids}
        cloud = densify.fuse_depth_maps(e, dev, opt, bgr=dev.bgr)
    finally:
        e.close()
    e = new_engine()
    try:
        e.scene_load(host, n_levels=1)
        run(e, host)
        for v in host.ids:
            for x, y, what in zip(got[v], e.scene_get_maps(v), ("depth", "normal", "confidence")):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (v, what)
        ref = densify.fuse_depth_maps(e, host, opt, bgr=host.bgr)
        for k in ("points", "views", "weights", "colors", "normals"):
            assert np.array_equal(cloud[k], ref[k]), k
        assert all((got[v][0] > 0).mean() > 0.5 for v in host.ids), [float((got[v][0] > 0).mean()) for v in host.ids]
        assert ref["nPoints"] > 0
    finally:
        e.close()


def dense_reconstruction_routes_agree(new_engine, tmp_path, level, min_resolution):
    """`dense_reconstruction` with the same seed by both routes: the archives are the same bytes."""
    out = {}
    for on_device in (False, True):
        e = new_engine()
        try:
            out[on_device] = str(tmp_path / ("device.mvs" if on_device else "host.mvs"))
            sv, cloud = densify.dense_reconstruction(e, SCENE, out[on_device], _opt(level, min_resolution), seed=3, prepare_on_device=on_device)
            assert cloud["nPoints"] > 0 and cloud["colors"] is not None
            assert all((g is None) == on_device for g in sv.gray) and all((b is None) == on_device for b in sv.bgr)
            assert e.image_stats()["prepared"] == (4 if on_device else 0) and e.image_bytes() == 0
        finally:
            e.close()
    with open(out[True], "rb") as a, open(out[False], "rb") as b:
        assert a.read() == b.read()
