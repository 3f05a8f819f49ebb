"""One SGM pair from the images to the disparity map, by the host route and by the device route of `sgm_pipeline.match_pair` (needs the GPU):

    python tools/sgm_pair_bench.py [--width 1920 --height 1080] [--source synth|scene --scale 3] [--reps 5] [--min-resolution 320] [--log profiles/sgm_pair_bench.log]

host route:   rectify.stereo_rectify_images (two numpy warps and masks) + to_gray_linear twice on the host, then sgmhip_tsgm_match, which uploads the six images;
device route: the two images resident (uploaded once per scene, timed apart), rectify.stereo_rectify_geometry on the host, sgmhip_rectify_pair, then
              sgmhip_tsgm_match_rectified.
Both run in this one process, alternating, after a warm-up of each; the results are compared (they are equal).  Times are host wall clock around calls that end in
a device synchronise; the rectification kernel is also timed by HIP events in a pass of its own (sgmhip_rectify_stats_get).  Bytes the kernel must move, per image:
8 B written per destination pixel (3 BGR + 4 gray + 1 mask) plus the bytes of the source rectangle the destination covers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmvs_amd import rectify, sgm, sgm_pipeline, tsgm  # noqa: E402


def synth_pair(w, h):
    """Two neighbouring views of the seeded synthetic scene and world points both see (a grid of view 0's ground-truth depths)."""
    from openmvs_amd import synth
    sc = synth.make_scene(2, w, h, n_src=1)
    K, R, C = sc.K[0], sc.R[0], sc.C[0]
    us, vs = np.meshgrid(np.arange(20, w - 20, 40, dtype=np.float64), np.arange(20, h - 20, 40, dtype=np.float64))
    d = sc.gt_depth[0][vs.astype(int), us.astype(int)].astype(np.float64)
    rays = np.stack([(us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1], np.ones_like(us)], -1) * d[..., None]
    X = (rays.reshape(-1, 3) @ R + C)[d.ravel() > 0]
    p2 = sgm_pipeline.world_to_image3(sc.K[1], sc.R[1], sc.C[1], X)
    X = X[(p2[:, 2] > 0) & (p2[:, 0] >= 0) & (p2[:, 1] >= 0) & (p2[:, 0] < w) & (p2[:, 1] < h)]
    return [np.ascontiguousarray(sc.bgr[i]) for i in (0, 1)], [(sc.K[i], sc.R[i], sc.C[i]) for i in (0, 1)], X


def scene_pair(scale, A=0, B=2):
    """Images A and B of tests/data/scene enlarged `scale` times, with the scene's own sparse points."""
    from PIL import Image
    from openmvs_amd import mvsi
    base = os.path.join(ROOT, "tests", "data", "scene")
    sc = mvsi.load(os.path.join(base, "scene.mvs"))
    bgr, cams = [], []
    for i in (A, B):
        with Image.open(os.path.join(base, sc.images[i].name)) as im:
            im = im.convert("RGB"); im = im.resize((im.width * scale, im.height * scale), Image.BICUBIC)
            bgr.append(np.ascontiguousarray(np.asarray(im)[..., ::-1]))
        cams.append(sc.camera(i, (bgr[-1].shape[1], bgr[-1].shape[0]))[:3])
    own = np.repeat(np.arange(len(sc.vertices)), np.diff(sc.vertex_view_start)); ids = sc.vertex_views["image_id"]
    seen = [np.isin(np.arange(len(sc.vertices)), own[ids == i]) for i in (A, B)]
    return bgr, cams, sc.vertices[seen[0] & seen[1]]


def source_bytes(Hf, size, src_shape):
    """3 B per pixel of the source rectangle that the destination's positions (and their second taps) cover."""
    w, h = size
    Hi = np.linalg.inv(Hf)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    Z = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
    X = (Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]) / Z; Y = (Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]) / Z
    H0, W0 = src_shape[:2]
    ok = (X > -1) & (Y > -1) & (X < W0) & (Y < H0)
    if not ok.any():
        return 0
    x0, x1 = max(int(np.floor(X[ok].min())), 0), min(int(np.floor(X[ok].max())) + 1, W0 - 1)
    y0, y1 = max(int(np.floor(Y[ok].min())), 0), min(int(np.floor(Y[ok].max())) + 1, H0 - 1)
    return (x1 - x0 + 1) * (y1 - y0 + 1) * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", choices=["synth", "scene"], default="synth")
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale", type=int, default=3, help="--source scene: enlargement of the 640 x 479 images")
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--min-resolution", type=int, default=320)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    a = ap.parse_args()
    bgr, cams, X = synth_pair(a.width, a.height) if a.source == "synth" else scene_pair(a.scale)
    m = sgm.SemiGlobalMatcherHIP(0)
    table = sgm_pipeline._srgb_table()
    sizes = [(b.shape[1], b.shape[0]) for b in bgr]
    p1 = sgm_pipeline.world_to_image3(*cams[0], X); p2 = sgm_pipeline.world_to_image3(*cams[1], X)
    now = time.perf_counter

    def crop_of(size):
        f = 1 << tsgm.compute_scale(size[0], size[1], a.min_resolution)
        return size[0] // f * f, size[1] // f * f

    def host():
        t0 = now()
        r = rectify.stereo_rectify_images(bgr[0], *cams[0], bgr[1], *cams[1], p1, p2)
        w, h = crop_of(r["size"])
        lb, rb = r["rect1"][:h, :w].copy(), r["rect2"][:h, :w].copy()
        lg, rg = sgm_pipeline.to_gray_linear(lb), sgm_pipeline.to_gray_linear(rb)
        lm, rm = r["mask1"][:h, :w].copy(), r["mask2"][:h, :w].copy()
        t1 = now()
        d, c, lv = m.tsgm_match(lb, rb, lg, rg, lm, rm, min_resolution=a.min_resolution)
        t2 = now()
        return t1 - t0, t2 - t1, d, c, (w, h), lv

    def device():
        t0 = now()
        g = rectify.stereo_rectify_geometry(sizes[0], *cams[0], sizes[1], *cams[1], p1, p2)
        w, h = crop_of(g["size"])
        m.rectify_pair(0, 1, np.linalg.inv(g["H1"]), np.linalg.inv(g["H2"]), (w, h), table)
        t1 = now()
        d, c, lv = m.tsgm_match_rectified(min_resolution=a.min_resolution)
        t2 = now()
        return t1 - t0, t2 - t1, d, c, (w, h), lv

    t0 = now(); m.scene_set_images(bgr); t_upload = now() - t0
    wh, wd = host(), device()                                     # warm-up of both routes: code objects, buffers
    assert np.array_equal(wh[2], wd[2]) and np.array_equal(wh[3], wd[3]), "the two routes disagree"
    size, levels = wd[4], wd[5]
    runs = {"host": [], "device": []}
    for _ in range(max(a.reps, 5)):
        for name, fn in (("host", host), ("device", device)):
            r = fn()
            assert np.array_equal(r[2], wd[2])
            runs[name].append((r[0], r[1]))
    g = rectify.stereo_rectify_geometry(sizes[0], *cams[0], sizes[1], *cams[1], p1, p2)
    inv = [np.linalg.inv(g["H1"]), np.linalg.inv(g["H2"])]
    m.stats_reset(True)
    for _ in range(max(a.reps, 5)):
        m.rectify_pair(0, 1, inv[0], inv[1], size, table)
    ev_ms, ev_n = m.rectify_stats()
    m.stats_reset(False)
    nbytes = sum(8 * size[0] * size[1] + source_bytes(H, size, b.shape) for H, b in zip((g["H1"], g["H2"]), bgr))

    out = []
    out.append("sgm_pair_bench: source %s, images %s, rectified %d x %d (cropped to the loop's multiple), %d levels, minResolution %d, valid disparities %.3f" %
               (a.source, " / ".join("%dx%d" % s for s in sizes), size[0], size[1], levels, a.min_resolution, float((wd[2] != sgm.NO_DISP).mean())))
    out.append("one-time upload of the two images to the resident scene: %.2f ms (host route: six images per pair inside the loop call)" % (t_upload * 1e3))
    out.append("%-7s %4s %14s %14s %14s %10s" % ("route", "rep", "rectify [ms]", "loop [ms]", "pair [ms]", "rectify %"))
    res = {}
    for name in ("host", "device"):
        for k, (tr, tl) in enumerate(runs[name]):
            out.append("%-7s %4d %14.3f %14.3f %14.3f %10.2f" % (name, k, tr * 1e3, tl * 1e3, (tr + tl) * 1e3, 100 * tr / (tr + tl)))
        tr = float(np.median([r[0] for r in runs[name]])); tl = float(np.median([r[1] for r in runs[name]])); tp = float(np.median([r[0] + r[1] for r in runs[name]]))
        out.append("%-7s %4s %14.3f %14.3f %14.3f %10.2f" % (name, "med", tr * 1e3, tl * 1e3, tp * 1e3, 100 * tr / (tr + tl)))
        res[name] = dict(rectify_ms=tr * 1e3, loop_ms=tl * 1e3, pair_ms=tp * 1e3, rectify_share=tr / (tr + tl))
    k_ms = ev_ms / max(ev_n, 1)
    out.append("rectification kernel by HIP events: %.4f ms per pair (mean of %d launches, both images in one launch); %.1f MB to move -> %.1f GB/s" %
               (k_ms, ev_n, nbytes / 1e6, nbytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else float("nan")))
    res.update(kernel_ms=k_ms, kernel_bytes=int(nbytes), kernel_GBps=nbytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None, upload_ms=t_upload * 1e3,
               rectified=list(size), levels=levels, source=a.source, images=[list(s) for s in sizes])
    out.append(json.dumps(res))
    text = "\n".join(out)
    print(text)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(text + "\n")
    m.close()
    assert res["device"]["pair_ms"] <= res["host"]["pair_ms"], "the device route is slower than the host route"


if __name__ == "__main__":
    main()
