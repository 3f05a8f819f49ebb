"""Preparing a scene's views from decoded 8-bit images, by the host route and by the device route of `densify.load_scene` (needs the GPU):

    python tools/scene_load_bench.py [--reps 5] [--log profiles/scene_load_bench.log]

host route:   Image::ResizeImage, toGray and the B, G, R image in numpy (`densify._resize_area_u8`, `views.to_gray`), per image;
device route: every decoded image goes to the engine's image store once (`PatchMatchHIP.image_prepare`: upload, then one kernel of csrc/pm_image.hip).
Both run in this one process on the cameras and sparse points of tests/data/scene with seeded synthetic images of the case's size in place of the files (decoding
is not measured: the loader hands out arrays made beforehand), alternating, after a warm-up of each; the images the two routes produce are compared once (equal).
Two cases: 4000 x 3000 halved (the default --resolution-level 1), and 3000 x 2000 -> 1280 x 853 (the general area path).
Wall times are the host clock around `load_scene`, which ends in a device synchronise on the device route, divided by the number of images; everything else
`load_scene` does (view selection, seed maps) is in both.  The kernel is timed by HIP events and the upload on the host clock inside the library
(`PatchMatchHIP.image_stats`).  Bytes the kernel must move per image: 3 W0 H0 read + (3 + 4) w h written; its share of peak is that over the kernel time over the
HBM3E peak of the MI355X (8.0 TB/s by specification; about 6.3 TB/s is what a plain copy reaches)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmvs_amd import densify, mvsi, optdense  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "data", "scene", "scene.mvs")
HBM_PEAK = 8.0e12          # bytes / s, specification
CASES = [dict(name="4000x3000 halved", size=(4000, 3000), level=1, max_resolution=3200, working=(2000, 1500)),
         dict(name="3000x2000 -> 1280x853", size=(3000, 2000), level=1, max_resolution=1280, working=(1280, 853))]


def synthetic_images(names, size, seed):
    """One seeded (H, W, 3) uint8 image per file name: smooth structure plus noise, so that neither route sees a constant."""
    W, H = size
    out = {}
    for k, n in enumerate(names):
        rng = np.random.default_rng(seed + k)
        coarse = rng.integers(0, 256, (H // 50 + 2, W // 50 + 2, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(coarse, 50, 0), 50, 1)[:H, :W].astype(np.int16) + rng.integers(-20, 21, (H, W, 3), dtype=np.int16)
        out[os.path.basename(n)] = np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))
    return out


def run_case(e, c, reps, out):
    names = [im.name for im in mvsi.load(SCENE).images]
    imgs = synthetic_images(names, c["size"], seed=c["size"][0])
    loader = lambda p: imgs[os.path.basename(p)]
    opt = optdense.defaults()
    opt.nResolutionLevel = c["level"]; opt.nMinResolution = 640; opt.nMaxResolution = c["max_resolution"]; opt.nNumViews = 8
    n = len(names)
    now = time.perf_counter

    def host():
        t0 = now(); sv = densify.load_scene(SCENE, opt=opt, image_loader=loader); return now() - t0, sv

    def device():
        e.image_drop(-1)
        t0 = now(); sv = densify.load_scene(SCENE, opt=opt, image_loader=loader, engine=e); e.sync(); return now() - t0, sv

    (_, hs), (_, ds) = host(), device()                           # warm-up of both routes, and the comparison
    assert hs.sizes == ds.sizes and all(s == c["working"] for s in hs.sizes[:n]) and not hs.alias_of, (hs.sizes, c["working"])
    for i in range(n):
        g, b = e.image_get(ds.stored[i])
        assert np.array_equal(g.view(np.uint32), hs.gray[i].view(np.uint32)) and np.array_equal(b, hs.bgr[i]), "the two routes disagree on image %d" % i
    del hs
    runs = {"host": [], "device": []}
    e.image_stats(reset=True)
    for _ in range(max(reps, 5)):
        for name, fn in (("host", host), ("device", device)):
            runs[name].append(fn()[0] / n)
    st = e.image_stats(reset=True)
    W0, H0 = c["size"]; w, h = c["working"]
    nbytes = 3 * W0 * H0 + 7 * w * h
    k_ms = st["kernel_ms"] / st["prepared"]; up_ms = st["upload_ms"] / st["prepared"]
    out.append("case %s: %d images of %d x %d -> %d x %d" % (c["name"], n, W0, H0, w, h))
    out.append("%-7s %4s %18s" % ("route", "rep", "per image [ms]"))
    res = dict(case=c["name"])
    for name in ("host", "device"):
        for k, t in enumerate(runs[name]):
            out.append("%-7s %4d %18.3f" % (name, k, t * 1e3))
        res[name + "_ms_per_image"] = float(np.median(runs[name])) * 1e3
        out.append("%-7s %4s %18.3f" % (name, "med", res[name + "_ms_per_image"]))
    rate = nbytes / (k_ms * 1e-3) if k_ms > 0 else float("nan")
    out.append("kernel by HIP events: %.4f ms per image (mean of %d launches); %.1f MB to move -> %.1f GB/s = %.1f %% of the 8.0 TB/s HBM peak" %
               (k_ms, st["prepared"], nbytes / 1e6, rate / 1e9, 100 * rate / HBM_PEAK))
    out.append("upload of the decoded image (pageable host memory, waited for): %.3f ms per image, %.1f MB -> %.1f GB/s" %
               (up_ms, 3 * W0 * H0 / 1e6, 3 * W0 * H0 / (up_ms * 1e-3) / 1e9 if up_ms > 0 else float("nan")))
    res.update(kernel_ms=k_ms, kernel_bytes=nbytes, kernel_GBps=rate / 1e9, kernel_share_of_hbm_peak=rate / HBM_PEAK, upload_ms=up_ms, launches=st["prepared"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    a = ap.parse_args()
    e = PatchMatchHIP(0)
    out = ["scene_load_bench: densify.load_scene on the cameras of tests/data/scene, seeded synthetic images, host route (numpy) against device route (image store)"]
    results = [run_case(e, c, a.reps, out) for c in CASES]
    e.close()
    out.append(json.dumps(results))
    text = "\n".join(out)
    print(text)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(text + "\n")
    for r in results:
        assert r["device_ms_per_image"] <= r["host_ms_per_image"], "the device route is slower than the host route (%s)" % r["case"]


if __name__ == "__main__":
    main()
