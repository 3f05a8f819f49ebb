"""Timing of MVS::EstimateNormalMap on one MI355X (csrc/pm_normal.hip: pm_normal_map_kernel) against the two host versions, at 1920x1080 and 3840x2160 on seeded depth
maps with about 10 % holes.  Per size, after a warm-up:
  kernel    the launch bracketed by HIP events on the engine's stream (pmhip_scene_estimate_normals only enqueues it), against the bytes it must move -- 4 read and 12
            written per pixel -- over the 8.0 TB/s HBM peak
  call      wall time of scene_estimate_normals + sync on the resident map (no upload, no download)
  host C++  mvsfront.estimate_normal_map (mvsf_estimate_normal_map), after one untimed call
  numpy     views.estimate_normal_map
The device result is compared with the C++ one bit for bit, and the tool asserts that the device call is not slower than the C++ host function in this run -- nothing
against a number chosen in advance.  Writes profiles/normal_map_bench.log.
    python tools/normal_map_bench.py [--reps 5] [--log profiles/normal_map_bench.log]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openmvs_amd import mvsfront, views  # noqa: E402
from openmvs_amd.patchmatch import PatchMatchHIP  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "normal_map_bench.log"))
a = ap.parse_args()
assert a.reps >= 5, "at least 5 repetitions"

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def depth_map(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = (4.0 + 0.002 * x + 0.001 * y + 0.05 * np.sin(x / 40.0) * np.cos(y / 60.0)).astype(np.float32)
    d *= (1.0 + 2e-3 * rng.standard_normal((h, w))).astype(np.float32)
    d[rng.random((h, w)) < 0.10] = 0
    return d


e = PatchMatchHIP(0)
stream = torch.cuda.ExternalStream(e.stream())
say("normal_map_bench: %s, %d repetitions after a warm-up" % (torch.cuda.get_device_name(0), a.reps))
results = []
for w, h in ((1920, 1080), (3840, 2160)):
    K = np.array([[0.9 * w, 0, w / 2 - 0.5], [0, 0.9 * w, h / 2 - 0.5], [0, 0, 1]])
    d = depth_map(w, h, w)
    e.scene_create(2, w, h, 0)
    for i in range(2):
        e.scene_set_view(i, np.zeros((h, w), np.float32), K, np.eye(3), np.zeros(3), 0.1, 100.0, [1 - i])
    e.scene_set_maps(0, d, None)
    e.scene_estimate_normals([0]); e.sync()                                  # warm-up: the first launch loads the code object
    kernel_ms, call_ms = [], []
    for _ in range(a.reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        e.scene_estimate_normals([0])
        ev1.record(stream)
        e.sync()
        kernel_ms.append(ev0.elapsed_time(ev1))
        t0 = time.perf_counter()
        e.scene_estimate_normals([0]); e.sync()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    got = e.scene_get_maps(0)[1]
    mvsfront.estimate_normal_map(K, d)                                       # untimed: the library's first call
    cpp_ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        want = mvsfront.estimate_normal_map(K, d)
        cpp_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref = views.estimate_normal_map(K, d)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(ref.view(np.uint32), want.view(np.uint32)))
    px = w * h
    k_med = float(np.median(kernel_ms))
    r = dict(size="%dx%d" % (w, h), pixels=px, holes=round(float((d == 0).mean()), 3), kernel_ms=[round(v, 4) for v in kernel_ms], kernel_ms_median=round(k_med, 4),
             bytes=16 * px, gbytes_per_s=round(16 * px / (k_med * 1e-3) / 1e9, 1), share_of_hbm_peak=round(16 * px / (k_med * 1e-3) / HBM_PEAK, 4),
             call_ms=[round(v, 3) for v in call_ms], call_ms_median=round(float(np.median(call_ms)), 3),
             host_cpp_ms=[round(v, 1) for v in cpp_ms], host_cpp_ms_median=round(float(np.median(cpp_ms)), 1), host_numpy_ms=round(numpy_ms, 1), bit_identical=same)
    say("%s: kernel %.4f ms (%.1f GB/s of the 16 B/pixel it must move, %.1f %% of the HBM peak), call + sync %.3f ms, host C++ %.1f ms, numpy %.1f ms, bit-identical %s"
        % (r["size"], k_med, r["gbytes_per_s"], 100 * r["share_of_hbm_peak"], r["call_ms_median"], r["host_cpp_ms_median"], numpy_ms, same))
    results.append(r)
e.close()
for r in results:
    say(json.dumps(r))
os.makedirs(os.path.dirname(a.log), exist_ok=True)
with open(a.log, "w") as f:
    f.write("\n".join(lines) + "\n")
for r in results:
    assert r["bit_identical"], "%s: the device result differs from the host's" % r["size"]
    assert r["call_ms_median"] <= r["host_cpp_ms_median"], "%s: the device call (%.3f ms) is slower than the C++ host function (%.1f ms)" % (r["size"], r["call_ms_median"], r["host_cpp_ms_median"])
