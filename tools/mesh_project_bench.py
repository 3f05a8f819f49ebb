"""Timing of Mesh::Project on one MI355X (csrc/pm_mesh.hip) on a synthetic displaced grid of about 2 M faces, against the host twin in the same run.

  render 1     one 1920x1080 view, depth and normals: device time of the clears and kernels (HIP events inside the call, pmhip_mesh_get_stats) and the wall time of the
               whole blocking call with its final sync and the download of the maps
  render 32    a 32-view batch at 1920x1080 in one call, the same two figures, per view
  visibility   pmhip_mesh_visibility: 100 views of at most 320 pixels (320x180), depth-only renders and the vertex test; only the bitset comes back
  host         `views.project_mesh` (numpy) on one view.  It is run on a quarter of the faces at a quarter of the pixels (the same pixels per face) and its time is
               multiplied by four: the figure is SCALED, and the log says so.  The reference's own loop is scalar C++ over every face, once per image.
  threshold    the small / large box threshold swept on three meshes -- the 2 M-face one (boxes of a few pixels), one of ~46 k faces (boxes of ~100 pixels) and one
               of ~4.6 k faces (boxes of ~900 pixels) -- 8 views each, device time, best of 3, the settings alternating

Every timed shape is warmed up first; every figure is the best of 3 in one process; the device maps of the first view are compared with the twin's on the reduced
mesh bit for bit.  Nothing is asserted against a number chosen in advance.  Writes profiles/mesh_project_bench.log.
    python tools/mesh_project_bench.py [--log profiles/mesh_project_bench.log] [--faces 2000000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from openmvs_amd import views  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mesh_project_bench.log"))
ap.add_argument("--faces", type=int, default=2000000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--vis-views", type=int, default=100)
a = ap.parse_args()
f32 = np.float32
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def grid(n_faces, aspect=16 / 9):
    """A displaced grid of about n_faces faces that fills the frame of a camera 3 units in front of it, turned towards it."""
    ny = max(int(round(np.sqrt(n_faces / 2 / aspect))), 1); nx = max(int(round(ny * aspect)), 1)
    xs, ys = np.meshgrid(np.linspace(-1.6, 1.6, nx + 1), np.linspace(-0.9, 0.9, ny + 1))
    z = 0.12 * np.sin(xs * 5.1 + 0.3) * np.cos(ys * 6.3) + 0.03 * np.sin(xs * 41.0) * np.sin(ys * 37.0)
    V = np.stack([xs, ys, z], -1).reshape(-1, 3).astype(f32)
    i = (np.arange(ny, dtype=np.int64)[:, None] * (nx + 1) + np.arange(nx, dtype=np.int64)[None, :]).ravel()
    F = np.concatenate([np.stack([i, i + nx + 1, i + 1], 1), np.stack([i + nx + 2, i + 1, i + nx + 1], 1)]).astype(np.uint32)
    return V, F


def cameras(n, w, h):
    """n cameras on an arc in front of the grid, all looking at its centre; the grid stays inside the frame with its border of 3."""
    K, R, C = [], [], []
    for k in range(n):
        ang = ((k % 8) - 3.5) * 0.04; tilt = ((k // 8) - 1.5) * 0.03
        cy, sy, cx, sx = np.cos(ang), np.sin(ang), np.cos(tilt), np.sin(tilt)
        Rk = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        K.append(np.array([[0.95 * w, 0, (w - 1) / 2], [0, 0.95 * w, (h - 1) / 2], [0, 0, 1]])); R.append(Rk); C.append(-Rk.T @ np.array([0.0, 0.0, 3.4]))
    return np.array(K), np.array(R), np.array(C)


def best_of_3(call):
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        st = call()
        out.append(((time.perf_counter() - t0) * 1e3, st["device_us"] / 1e3))
    return min(v[0] for v in out), min(v[1] for v in out), [round(v[0], 2) for v in out], [round(v[1], 3) for v in out]


import torch  # noqa: E402  (the device's name)
e = PatchMatchHIP(0)
w, h = a.width, a.height
V, F = grid(a.faces)
say("mesh_project_bench: %s; displaced grid of %d vertices, %d faces; best of 3 after a warm-up, one process" % (torch.cuda.get_device_name(0), len(V), len(F)))
t0 = time.perf_counter()
e.mesh_set(V, F)
say("mesh_set (host vertex normals in face order, upload): %.1f ms" % ((time.perf_counter() - t0) * 1e3))
results = {"faces": int(len(F)), "vertices": int(len(V)), "size": "%dx%d" % (w, h)}


def render(n):
    K, R, C = cameras(n, w, h)
    def call():
        e.mesh_project(K, R, C, [(w, h)] * n, normals=True)
        return e.mesh_tuning()
    st = call()                                                                # warm-up: code objects, buffers
    wall, dev, walls, devs = best_of_3(call)
    got = e.mesh_project(K[:1], R[:1], C[:1], [(w, h)], normals=False)[0][0]
    say("render %d view(s) %dx%d with normals: device %.3f ms per view (%s ms per call), call + sync + download %.2f ms per view (%s ms per call); %d batch(es), "
        "%d faces on the workgroup route, %.1f %% of the pixels covered" % (n, w, h, dev / n, devs, wall / n, walls, st["batches"], st["large_faces"], 100 * float((got > 0).mean())))
    return dict(views=n, device_ms_per_view=round(dev / n, 4), call_ms_per_view=round(wall / n, 3), device_ms=devs, call_ms=walls, batches=st["batches"], covered=round(float((got > 0).mean()), 4))


results["render_1"] = render(1)
results["render_batch"] = render(a.views)

# visibility: the reference's 320-pixel render for every image and the vertex test
vw, vh = 320, int(round(320 * h / w))
K, R, C = cameras(a.vis_views, vw, vh)


def vis_call():
    global vis
    vis = e.mesh_visibility(K, R, C, [(vw, vh)] * a.vis_views, len(V))
    return e.mesh_tuning()


st = vis_call()
wall, dev, walls, devs = best_of_3(vis_call)
say("visibility %d views %dx%d: device %.3f ms per view (%s ms per call), call + sync + bitset download %.2f ms per view; %d batch(es); %.1f %% of the (vertex, view) pairs visible"
    % (a.vis_views, vw, vh, dev / a.vis_views, devs, wall / a.vis_views, st["batches"], 100 * float(vis.mean())))
results["visibility"] = dict(views=a.vis_views, size="%dx%d" % (vw, vh), device_ms_per_view=round(dev / a.vis_views, 4), call_ms_per_view=round(wall / a.vis_views, 3), visible=round(float(vis.mean()), 4))

# the host twin on a quarter of the faces at a quarter of the pixels, scaled by four; the device on the same input for the comparison of the maps
Vq, Fq = grid(a.faces // 4)
Kq, Rq, Cq = cameras(1, w // 2, h // 2)
Nq = views.compute_normal_vertices(Vq, Fq)
t0 = time.perf_counter()
dq, nq = views.project_mesh(Kq[0], Rq[0], Cq[0], w // 2, h // 2, Vq, Fq, Nq)
host_ms = (time.perf_counter() - t0) * 1e3
e.mesh_set(Vq, Fq)
gd, gn = e.mesh_project(Kq, Rq, Cq, [(w // 2, h // 2)])[0]
same = bool(np.array_equal(gd.view(np.uint32), dq.view(np.uint32)) and np.array_equal(gn.view(np.uint32), nq.view(np.uint32)))
say("host twin (numpy) on %d faces at %dx%d: %.0f ms; SCALED by 4 to the full mesh and size: %.0f ms per view (not measured at full size); device maps bit-identical to it: %s"
    % (len(Fq), w // 2, h // 2, host_ms, 4 * host_ms, same))
results["host"] = dict(faces=int(len(Fq)), size="%dx%d" % (w // 2, h // 2), ms=round(host_ms, 1), scaled_ms_per_view=round(4 * host_ms, 1), scaled=True, bit_identical=same)

# the threshold sweep: device time of 8 views, the settings alternating, best of 3
sweep = {}
BOXES = (16, 64, 256, 1024, 4096)
for name, nf in (("fine", a.faces), ("medium", 46000), ("coarse", 4600)):
    Vs, Fs = grid(nf)
    e.mesh_set(Vs, Fs)
    K, R, C = cameras(8, w, h)
    times = {b: [] for b in BOXES}
    large = {}
    for rep in range(4):                                                       # the first round warms up
        for b in BOXES:
            e.mesh_tuning(box_pixels=b)
            e.mesh_project(K, R, C, [(w, h)] * 8, normals=False)
            st = e.mesh_tuning()
            large[b] = st["large_faces"]
            if rep:
                times[b].append(st["device_us"] / 1e3 / 8)
    sweep[name] = {b: dict(device_ms_per_view=round(min(times[b]), 4), runs=[round(v, 4) for v in times[b]], large_faces=large[b]) for b in BOXES}
    say("threshold sweep, %s mesh (%d faces, 8 views %dx%d, depth only), device ms per view [faces on the workgroup route]: %s"
        % (name, len(Fs), w, h, ", ".join("%d: %.4f [%d]" % (b, sweep[name][b]["device_ms_per_view"], large[b]) for b in BOXES)))
e.mesh_tuning(box_pixels=-1)
results["threshold_sweep"] = sweep
results["default_box_pixels"] = e.mesh_tuning()["box_pixels"]
e.close()
say(json.dumps(results))
os.makedirs(os.path.dirname(a.log), exist_ok=True)
with open(a.log, "w") as f:
    f.write("\n".join(lines) + "\n")
assert same, "the device maps differ from the host twin's"
