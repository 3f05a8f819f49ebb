"""include/DenseDepthMapsHIP.hpp as a host that resumes depth maps from files: SetDepthMap installs every view's depth and confidence, some without normals, and
EstimateMissingNormals makes those on the device (pmhip_scene_estimate_normals) -- bit for bit `views.estimate_normal_map`; stored normals stay as they are; then
pmhip_estimate_normal_map on host buffers.  The program links the emulated library in the CPU suite and the device library in the GPU suite."""
import os
import subprocess

import numpy as np
import pytest

from openmvs_amd import patchmatch, views
from tests import normal_map_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp, lib, hip):
    exe = os.path.join(tmp, "normal_map_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "normal_map_driver.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + os.path.dirname(lib)] + (["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []))
    return exe


def _run(tmp_path, exe):
    rng = np.random.default_rng(23)
    w, h = 70, 23
    sizes = [(w, h), (41, 37), (w, h)]                         # the middle view carries its own size and K
    has_normal = [False, False, True]
    R = np.eye(3); C = np.zeros(3)
    inp, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    maps = []
    with open(inp, "wb") as f:
        f.write(np.array([3, w, h], np.int32).tobytes())
        for i, (vw, vh) in enumerate(sizes):
            d = cases.surface(rng, vh, vw, holes=0.1); c = rng.random((vh, vw)).astype(f32)
            n = np.full((vh, vw, 3), cases.SENTINEL, f32) if has_normal[i] else None
            f.write(np.array([vw, vh, int(has_normal[i])], np.int32).tobytes())
            f.write(np.concatenate([cases.KS[i].ravel(), R.ravel(), C.ravel()]).astype(np.float64).tobytes())
            f.write(d.tobytes()); f.write(c.tobytes())
            if n is not None:
                f.write(n.tobytes())
            maps.append((d, n, c))
    subprocess.check_call([exe, str(inp), str(out)])
    raw = np.frombuffer(open(out, "rb").read(), f32)
    at = 0
    for i, (d, n, c) in enumerate(maps):
        P = d.size
        cases.same_bits(raw[at:at + P].reshape(d.shape), d, "depth %d" % i)
        cases.same_bits(raw[at + P:at + 4 * P].reshape(d.shape + (3,)), cases.host(cases.KS[i], d, "view %d" % i) if n is None else n, "normals %d" % i)
        cases.same_bits(raw[at + 4 * P:at + 5 * P].reshape(d.shape), c, "confidence %d" % i)
        at += 5 * P
    d0 = maps[0][0]
    cases.same_bits(raw[at:].reshape(d0.shape + (3,)), views.estimate_normal_map(cases.KS[0], d0), "pmhip_estimate_normal_map")


def test_normal_map_driver_under_the_emulator(tmp_path):
    from tests import emu
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as lib:
        _run(tmp_path, _build(str(tmp_path), lib, hip=False))


@pytest.mark.gpu
def test_normal_map_driver_on_the_device(tmp_path):
    from openmvs_amd import build
    _run(tmp_path, _build(str(tmp_path), build.build_lib("libpmhip.so"), hip=True))
