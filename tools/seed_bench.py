"""Timing of the seed rasteriser (csrc/seed_raster.hip) on one MI355X against the host route it replaces, in one process.

  full HD      1920x1080, depth and normals, the points of image 0 of tests/data/scene projected at that size, faces rasterised (bInitSparse = 0) and 2x2 splats
  corners      1024x768, depth only, the same points with the four image corners (the SGM path's seed)

  host route   the C++ front end makes the maps (mvsf_init_depth_map_dense / mvsf_init_depth_map / mvsf_triangulate_depth_map) and `scene_set_maps` uploads them
  device route the C++ front end makes the mesh (mvsf_point_mesh) and `scene_seed_view` rasterises it into the resident maps; the rasteriser alone is also timed
  python walk  `views.triangulate_points_depth_map`, the pure-Python face walk the SGM path ran per pair, timed ONCE at 160x120 and labelled so

After a warm-up of both routes, `--reps` (at least 5) repetitions alternate between the two; the figure of a route is the median of its wall times per view.  The
kernel time is that of the clears and kernels by HIP events (pmhip_seed_get_stats).  The bytes the kernels must move per pixel: two passes over the key map (4 B
written by the clear, 4 B read by the resolve pass), the depth (4 B) and, with normals, the normal (12 B); that figure over the kernel time is set against the
8.0 TB/s HBM peak.  The device depth maps are compared with the host route's bit for bit (the normal maps to 1e-6: mvsf_point_mesh sums the vertex normals in the
Python front end's order, mvsf_init_depth_map face by face).  The only assertion on a time: the device route is not slower per view than the host route of the same
run.  Writes profiles/seed_raster_bench.log.
    python tools/seed_bench.py [--log profiles/seed_raster_bench.log] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from openmvs_amd import mvsfront, mvsi, views  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP, SEED_FACES, SEED_POINTS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "seed_raster_bench.log"))
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
assert a.reps >= 5
SCENE = os.path.join(ROOT, "tests", "data", "scene", "scene.mvs")
HBM_PEAK = 8.0e12          # bytes / s, specification
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


try:
    import torch  # noqa: E402  (the device's name)
    DEVICE = torch.cuda.get_device_name(0)
except Exception:
    DEVICE = "unnamed device"
cf, py = mvsfront.SceneFront(SCENE), mvsi.load(SCENE)
e = PatchMatchHIP(0)
say("seed_bench: %s; image 0 of tests/data/scene; warm-up, then %d alternating repetitions per route, medians; one process" % (DEVICE, a.reps))
results = {}
ok = True


def bench(name, size, mode, corners, with_normals):
    global ok
    w, h = size
    cams = views.Cameras(py, [size] * len(py.images))
    _, pts, avg = views.select_views(py, cams, 0, views.DenseOptions())
    pts = np.ascontiguousarray(pts, np.uint32)
    e.scene_create(2, w, h, 0)

    def host():
        t0 = time.perf_counter()
        if corners:
            d, n = cf.triangulate_depth_map(0, pts, size, avg, sparse=mode == SEED_POINTS)[0], None
        else:
            d, n = cf.init_depth_map(0, pts, size, dense=mode == SEED_FACES)[:2]
        t1 = time.perf_counter()
        e.scene_set_maps(0, d, n)
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, d, n

    def device():
        t0 = time.perf_counter()
        proj, z, nrm, faces, _, _ = cf.point_mesh(0, pts, size, avg if corners else None, normals=with_normals)
        t1 = time.perf_counter()
        e.scene_seed_view(0, mode, proj, z, nrm, faces)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, e.seed_stats()

    _, _, hd, hn = host(); device()                                              # warm-up: code objects, buffers
    gd, gn, _ = e.scene_get_maps(0)
    same_depth = bool(np.array_equal(gd.view(np.uint32), hd.view(np.uint32)))
    normals_close = True if hn is None else bool(np.abs(gn - hn).max() < 1e-6)
    H, D = [], []
    for _ in range(a.reps):
        H.append(host()[:2]); D.append(device())
    med = statistics.median
    host_ms, host_cpu = med(v[0] for v in H), med(v[1] for v in H)
    dev_ms, mesh_ms, seed_ms = med(v[0] for v in D), med(v[1] for v in D), med(v[2] for v in D)
    k_ms = med(v[3]["device_us"] for v in D) / 1e3
    st = D[-1][3]
    per_px = 4 + 4 + 4 + (12 if with_normals else 0)
    nbytes = per_px * w * h
    rate = nbytes / (k_ms * 1e-3) if k_ms > 0 else 0.0
    say("%s, %dx%d, %s, %d vertices: host route %.3f ms per view (maps on the host %.3f ms, the rest upload); device route %.3f ms per view (mesh on the host %.3f ms, "
        "scene_seed_view %.3f ms, of which kernels and clears by HIP events %.4f ms; %d faces on the workgroup route, %d B of mesh uploaded against %d B of maps)"
        % (name, w, h, "faces" if mode == SEED_FACES else "2x2 splats", len(pts) + (4 if corners else 0),
           host_ms, host_cpu, dev_ms, mesh_ms, seed_ms, k_ms, st["large_faces"], st["mesh_bytes"], (16 if with_normals else 4) * w * h))
    say("    kernels must move %d B per pixel (key clear 4, key read 4, depth 4%s) = %.1f MB -> %.1f GB/s = %.2f %% of the 8.0 TB/s HBM peak; %.1f %% of the pixels covered; "
        "depth bit-identical to the host route: %s; normals within 1e-6: %s" % (per_px, ", normal 12" if with_normals else "", nbytes / 1e6, rate / 1e9, 100 * rate / HBM_PEAK,
                                                                              100 * float((gd > 0).mean()), same_depth, normals_close))
    results[name + ("_faces" if mode == SEED_FACES else "_points")] = dict(
        size="%dx%d" % size, host_ms_per_view=round(host_ms, 4), host_maps_ms=round(host_cpu, 4), device_ms_per_view=round(dev_ms, 4), mesh_ms=round(mesh_ms, 4),
        seed_view_ms=round(seed_ms, 4), kernel_ms=round(k_ms, 5), bytes_per_pixel=per_px, kernel_GBps=round(rate / 1e9, 1), share_of_hbm_peak=round(rate / HBM_PEAK, 5),
        large_faces=st["large_faces"], mesh_bytes=st["mesh_bytes"], depth_bit_identical=same_depth, normals_close=normals_close,
        host_runs=[round(v[0], 3) for v in H], device_runs=[round(v[0], 3) for v in D])
    ok = ok and same_depth and normals_close
    return host_ms, dev_ms


timed = [bench("full_hd", (1920, 1080), SEED_FACES, False, True), bench("full_hd", (1920, 1080), SEED_POINTS, False, True),
         bench("corners", (1024, 768), SEED_FACES, True, False)]

# the Python walk the SGM path ran for every pair: once, at a small size
size = (160, 120)
cams = views.Cameras(py, [size] * len(py.images))
_, pts, avg = views.select_views(py, cams, 0, views.DenseOptions())
t0 = time.perf_counter()
views.triangulate_points_depth_map(cams.K[0], cams.P[0], py.vertices[pts], *size, avg_depth=avg)
walk_ms = (time.perf_counter() - t0) * 1e3
say("python walk (views.triangulate_points_depth_map with corners), ONCE at %dx%d, NOT at the sizes above: %.0f ms" % (size[0], size[1], walk_ms))
results["python_walk"] = dict(size="%dx%d" % size, ms=round(walk_ms, 1), runs=1)
e.close(); cf.close()
say(json.dumps(results))
os.makedirs(os.path.dirname(a.log), exist_ok=True)
with open(a.log, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the device maps differ from the host route's"
for host_ms, dev_ms in timed:
    assert dev_ms <= host_ms, "the device route (%.3f ms per view) is slower than the host route (%.3f ms)" % (dev_ms, host_ms)
