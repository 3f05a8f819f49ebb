"""Timing of pmhip_scene_cloud_finish (csrc/pm_cloud.hip) on one MI355X: the fused cloud of BASELINE config 5's scale (5 x 3840x2160) and of
9 x 1920x1080, cropped to a box that keeps ~90 %, coloured and given PCA normals (k = 16).  Prints the engine's step times (crop, grid build,
k-NN + PCA, colours; each ended by a stream synchronisation, no download), points per second, and the same-box CPU yardstick: scipy's
cKDTree(...).query(k=16, workers=16) plus the numpy PCA over the same neighbour sets.  One JSON line per cloud at the end.
    python tools/cloud_finish_bench.py [--reps 3] [--no-cpu] [--only 4k|1080p] [--filter TH]
--filter TH adds Scene::PointCloudFilter(TH) (pmhip_scene_cloud_filter, csrc/pm_cloud_filter.hip) on the finished cloud: its step times (binning, cone pass,
removal), the cones, the candidates classified per cone and the fusion's own wall time next to it.
Kernel figures: run it under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/cloud_finish_bench.py --no-cpu`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from openmvs_amd import synth  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP  # noqa: E402
from tests import fuse_cases as fc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-cpu", action="store_true")
ap.add_argument("--only", default="")
ap.add_argument("--filter", type=int, default=None, metavar="TH")
a = ap.parse_args()

CASES = [("4k", 5, 3840, 2160, 4), ("1080p", 9, 1920, 1080, 8)]


def cpu_yardstick(pts, k=16, workers=16):
    from scipy.spatial import cKDTree
    X = pts.astype(np.float64)
    t0 = time.time()
    tree = cKDTree(X)
    t1 = time.time()
    normals = np.empty((len(X), 3), np.float32)
    tq = tp = 0.0
    for s in range(0, len(X), 1 << 20):
        q0 = time.time()
        _, idx = tree.query(X[s:s + (1 << 20)], k=k, workers=workers)
        q1 = time.time()
        nb = X[idx]
        d = nb - nb.mean(axis=1, keepdims=True)
        _, vec = np.linalg.eigh(np.einsum("qki,qkj->qij", d, d))
        normals[s:s + len(idx)] = vec[:, :, 0]
        tp += time.time() - q1; tq += q1 - q0
    return dict(build_s=t1 - t0, query_s=tq, pca_s=tp, total_s=t1 - t0 + tq + tp)


results = []
for name, V, W, H, nsrc in CASES:
    if a.only and a.only != name:
        continue
    t = time.time()
    sc = synth.make_scene(V, W, H, n_src=nsrc, device="cuda")
    maps = fc.make_maps(sc, seed=7)
    e = PatchMatchHIP(0)
    e.scene_load(sc, n_levels=0)
    for v in range(V):
        e.scene_set_maps(v, maps[0][v], maps[1][v]); e.scene_set_conf(v, maps[2][v]); e.scene_set_color(v, sc.bgr[v])
    order = sorted(range(V), key=lambda i: (-len(sc.neighbors[i]), i))
    fused = e.scene_fuse(order, bEstimateColor=False, bEstimateNormal=False)
    pts = fused["points"]
    lo, hi = np.percentile(pts, 2, axis=0), np.percentile(pts, 98, axis=0)
    obb = (np.eye(3, dtype=np.float32), ((lo + hi) * 0.5).astype(np.float32), ((hi - lo) * 0.5).astype(np.float32))
    print("%s: %d views %dx%d fused into %d points (setup %.1f s)" % (name, V, W, H, fused["nPoints"], time.time() - t), flush=True)
    best = None
    for r in range(a.reps + 1):                          # the first run allocates the working buffers
        e.scene_fuse(order, bEstimateColor=False, bEstimateNormal=False)
        t0 = time.time()
        out = e.scene_cloud_finish(crop_obb=obb, estimate_colors=True, estimate_normals=True)
        wall = time.time() - t0
        tm = out["times"]
        print("  run %d: %s ms, %d points kept, wall incl. download %.1f ms" % (r, {k: round(v, 2) for k, v in tm.items()}, out["nPoints"], wall * 1e3), flush=True)
        if r and (best is None or sum(tm.values()) < sum(best.values())):
            best = dict(tm)
    total = sum(best.values())
    res = dict(cloud=name, fused_points=int(fused["nPoints"]), kept_points=int(out["nPoints"]), ms=best, total_ms=round(total, 2),
               normals_ms=round(best["grid"] + best["knn_pca"], 2), points_per_s=round(out["nPoints"] / (total / 1e3)))
    if not a.no_cpu:
        y = cpu_yardstick(out["points"])
        res["cpu_yardstick_s"] = {k: round(v, 3) for k, v in y.items()}
        res["speedup_normals_vs_cpu"] = round(y["total_s"] * 1e3 / res["normals_ms"], 1)
        print("  CPU yardstick (cKDTree workers=16 + numpy PCA): %s s" % res["cpu_yardstick_s"], flush=True)
    if a.filter is not None:
        fbest = None
        for r in range(a.reps + 1):
            t0 = time.time()
            e.scene_fuse(order, bEstimateColor=False, bEstimateNormal=False)
            fuse_ms = (time.time() - t0) * 1e3                   # (with the download of the fused cloud)
            e.scene_cloud_finish(crop_obb=obb, estimate_colors=True, estimate_normals=True)
            t0 = time.time()
            out = e.scene_cloud_filter(th_remove=a.filter)
            wall = time.time() - t0
            tm = out["times"]
            print("  filter run %d: %s ms, %d -> %d points, %d cones, %.0f candidates per cone, wall incl. download %.1f ms (fusion %.1f ms)" %
                  (r, {k: round(v, 2) for k, v in tm.items()}, len(out["visibility"]), out["nPoints"], out["n_cones"], out["n_candidates"] / max(out["n_cones"], 1), wall * 1e3, fuse_ms), flush=True)
            if r and (fbest is None or sum(tm.values()) < sum(fbest[0].values())):
                fbest = (dict(tm), fuse_ms)
        tm, fuse_ms = fbest
        vis = out["visibility"]
        res["filter"] = dict(th=a.filter, ms={k: round(v, 2) for k, v in tm.items()}, total_ms=round(sum(tm.values()), 2), points=int(len(vis)), kept=int(out["nPoints"]),
                             cones=out["n_cones"], candidates=out["n_candidates"], candidates_per_cone=round(out["n_candidates"] / max(out["n_cones"], 1), 1),
                             ns_per_cone=round(tm["cones"] * 1e6 / max(out["n_cones"], 1), 2), ps_per_classification=round(tm["cones"] * 1e9 / max(out["n_candidates"], 1), 2),
                             nonzero=int((vis != 0).sum()), fuse_wall_ms=round(fuse_ms, 1))
    results.append(res)
    e.close()
for r in results:
    print(json.dumps(r))
