"""include/DenseDepthMapsHIP.hpp as a host that exports a scan's depth maps: SetMesh makes the mesh resident, ProjectMesh renders it into listed views of the loaded
scene at their own sizes (pmhip_mesh_project) -- bit for bit `views.project_mesh` -- with and without normals, ReleaseMesh frees it.  The program links the emulated
library in the CPU suite and the device library in the GPU suite."""
import os
import subprocess

import numpy as np
import pytest

from openmvs_amd import patchmatch, views
from tests import mesh_project_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp, lib, hip):
    exe = os.path.join(tmp, "mesh_project_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mesh_project_driver.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + os.path.dirname(lib)] + (["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []))
    return exe


def _run(tmp_path, exe):
    V, F = cases.grid_mesh(24, 12, -1.3, 1.3, -0.7, 0.7, 0.0, 0.2, 7)
    cams = [cases.generic_cam(65, 33, 11), cases.generic_cam(33, 17, 13), cases.generic_cam(65, 33, 16, dist=1.2)]      # the middle view carries its own size
    inp, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(cams), 65, 33, len(V), len(F)], np.int32).tobytes())
        for K, R, C, w, h in cams:
            f.write(np.array([w, h], np.int32).tobytes())
            f.write(np.concatenate([K.ravel(), R.ravel(), C.ravel()]).astype(np.float64).tobytes())
        f.write(V.tobytes()); f.write(F.tobytes())
    subprocess.check_call([exe, str(inp), str(out)])
    raw = np.frombuffer(open(out, "rb").read(), f32)
    N = views.compute_normal_vertices(V, F)
    want = [views.project_mesh(K, R, C, w, h, V, F, N) for K, R, C, w, h in cams]
    assert sum((d > 0).sum() for d, _ in want) > 1000
    at = 0
    for i, (d, n) in enumerate(want):
        cases.same_bits(raw[at:at + d.size].reshape(d.shape), d, "depth %d" % i); at += d.size
        cases.same_bits(raw[at:at + n.size].reshape(n.shape), n, "normals %d" % i); at += n.size
    for i, (d, n) in enumerate(want):
        cases.same_bits(raw[at:at + d.size].reshape(d.shape), d, "depth %d of the depth-only call" % i); at += d.size
    assert at == len(raw)


def test_mesh_project_driver_under_the_emulator(tmp_path):
    from tests import emu
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as lib:
        _run(tmp_path, _build(str(tmp_path), lib, hip=False))


@pytest.mark.gpu
def test_mesh_project_driver_on_the_device(tmp_path):
    from openmvs_amd import build
    _run(tmp_path, _build(str(tmp_path), build.build_lib("libpmhip.so"), hip=True))
