"""Timing of the image and PLY outputs (csrc/pm_export.hip) on one MI355X against the host route a caller had before them: `scene_get_maps` (24 MB per 1920x1080 view
over PCIe) plus the numpy statements of openmvs_amd/mapexport.py.  The scene is the 9 x 1920x1080 one of tools/cloud_finish_bench.py (seeded maps, fused on the device).
Per output, after a warm-up, the median of --reps runs:
  device   wall time of the binding's call, which ends in a stream synchronise and includes the download of the image or the records; next to it the time between
           the HIP events that bracket the call's kernels and its download (pmhip_export_get_stats), and the kernels launched
  host     wall time of scene_get_maps + the numpy twin (for the scales: `point_scales` on the cloud already on the host)
Five rows: depth image, confidence image, normal image, view cloud (with normals), cloud scales.  Every device result is compared with the twin bit for bit.  The tool
asserts nothing about speed: it reports which rows, if any, the device route loses.  Writes the log named by --log.
    python tools/map_export_bench.py [--reps 5] [--log profiles/map_export_bench.log] [--size 1920x1080]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openmvs_amd import mapexport as mx  # noqa: E402
from openmvs_amd import synth  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP  # noqa: E402
from tests import fuse_cases as fc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "map_export_bench.log"))
ap.add_argument("--size", default="1920x1080", help="WxH of the views (the figures of DESIGN 4.12 are at the default)")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    fn()                                                                       # warm-up: code objects, working buffers
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


V = 9
W, H = (int(v) for v in a.size.split("x"))
t = time.time()
sc = synth.make_scene(V, W, H, n_src=8, device="cuda" if torch.cuda.is_available() else "cpu")
maps = fc.make_maps(sc, seed=7)
e = PatchMatchHIP(0)
e.scene_load(sc, n_levels=0)
for v in range(V):
    e.scene_set_maps(v, maps[0][v], maps[1][v]); e.scene_set_conf(v, maps[2][v]); e.scene_set_color(v, sc.bgr[v])
say("map_export_bench: %s, %d views %dx%d, %d repetitions after a warm-up (setup %.1f s)" % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU: a rehearsal, the times mean nothing", V, W, H, a.reps, time.time() - t))
view = 0
bgr = np.ascontiguousarray(sc.bgr[view])
rows = []


def row(name, device, host, same):
    d_ms, got = timed(device, a.reps)
    s = e.export_stats()
    h_ms, want = timed(host, max(1, min(a.reps, 3)))
    ok = bool(same(got, want))
    rows.append(dict(output=name, device_ms=round(d_ms, 3), device_kernels_us=s["device_us"], launches=s["launches"], host_ms=round(h_ms, 1), bit_identical=ok,
                     device_not_slower=bool(d_ms <= h_ms)))
    say("%-16s device %9.3f ms (events %7d us, %2d launches)   host %9.1f ms   bit-identical %s" % (name, d_ms, s["device_us"], s["launches"], h_ms, ok))


row("depth image", lambda: e.scene_depth_image(view)[0], lambda: mx.depth_map_to_image(e.scene_get_maps(view)[0])[0], np.array_equal)
row("confidence image", lambda: e.scene_conf_image(view)[0], lambda: mx.conf_map_to_image(e.scene_get_maps(view)[2])[0], np.array_equal)
row("normal image", lambda: e.scene_normal_image(view), lambda: mx.normal_map_to_image(e.scene_get_maps(view)[1]), np.array_equal)


def host_cloud():
    d, n, _ = e.scene_get_maps(view)
    return mx.view_point_cloud(sc.K[view], sc.R[view], sc.C[view], d, n, bgr)


n_valid = int((maps[0][view] > 0).sum())
row("view cloud", lambda: e.scene_view_cloud(view, True, capacity=n_valid), host_cloud, lambda g, w: g.tobytes() == w.tobytes())
order = sorted(range(V), key=lambda i: (-len(sc.neighbors[i]), i))
cloud = e.scene_fuse(order, bEstimateColor=False, bEstimateNormal=False)
say("fused cloud: %d points, %d views listed" % (cloud["nPoints"], len(cloud["views"])))
row("cloud scales", lambda: e.scene_cloud_scale(1.7),
    lambda: mx.point_scales(cloud["points"], cloud["viewStart"], cloud["views"], cloud["weights"], sc.K, sc.R, sc.C, 1.7),
    lambda g, w: np.array_equal(g[0].view(np.uint32), w[0].view(np.uint32)) and np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)))
e.close()
slower = [r["output"] for r in rows if not r["device_not_slower"]]
say("device route slower than the host route for: %s" % (", ".join(slower) if slower else "none"))
for r in rows:
    say(json.dumps(r))
os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
with open(a.log, "w") as f:
    f.write("\n".join(lines) + "\n")
for r in rows:
    assert r["bit_identical"], "%s: the device result differs from the twin's" % r["output"]
