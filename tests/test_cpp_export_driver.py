"""include/DenseDepthMapsHIP.hpp as a host that writes the reference's outputs: a three-view scene, one view of its own size, gets its maps through SetDepthMap;
DepthImage, ConfImage and ViewCloud for every view and SavePointCloud (with scales, with view lists, by view count) are compared with the numpy statements of
openmvs_amd/mapexport.py and the writers of openmvs_amd/plyio.py, byte for byte.  The program links the emulated library in the CPU suite and the device library in the
GPU suite."""
import os
import subprocess

import numpy as np
import pytest

from openmvs_amd import mapexport as mx
from openmvs_amd import patchmatch, plyio
from tests import map_export_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp, lib, hip):
    exe = os.path.join(tmp, "export_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "export_driver.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + os.path.dirname(lib)] + (["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []))
    return exe


def _run(tmp_path, exe):
    rng = np.random.default_rng(61)
    w, h = 70, 23
    sizes = [(w, h), (41, 37), (w, h)]                         # the middle view carries its own size
    colour = [True, True, False]
    inp, out = tmp_path / "scene.bin", tmp_path / "out"
    out.mkdir()
    maps, cams = [], []
    with open(inp, "wb") as f:
        f.write(np.array([3, w, h], np.int32).tobytes())
        for i, (vw, vh) in enumerate(sizes):
            d = rng.uniform(1.0, 6.0, (vh, vw)).astype(f32); d[rng.random((vh, vw)) < 0.2] = 0
            c = rng.uniform(0.05, 0.9, (vh, vw)).astype(f32); c[d == 0] = 0
            n = rng.standard_normal((vh, vw, 3)).astype(f32)
            bgr = rng.integers(0, 256, (vh, vw, 3)).astype(np.uint8) if colour[i] else None
            K = cases.K0.copy(); K[0, 2] = (vw - 1) / 2.0; K[1, 2] = (vh - 1) / 2.0
            Ci = cases.C0 + np.array([0.4 * i, 0.0, 0.0])
            f.write(np.array([vw, vh, int(colour[i])], np.int32).tobytes())
            f.write(np.concatenate([K.ravel(), cases.R0.ravel(), Ci.ravel()]).astype(np.float64).tobytes())
            f.write(d.tobytes()); f.write(c.tobytes()); f.write(n.tobytes())
            if bgr is not None:
                f.write(bgr.tobytes())
            maps.append((d, c, n, bgr)); cams.append((K, cases.R0, Ci))
        P = 40
        pts = np.c_[rng.uniform(-2, 2, P), rng.uniform(-1, 1, P), rng.uniform(5, 9, P)].astype(f32)
        cnt = rng.integers(1, 4, P)
        vs = np.r_[0, np.cumsum(cnt)].astype(np.uint32)
        vv = np.concatenate([np.sort(rng.choice(3, k, replace=False)) for k in cnt]).astype(np.uint32)
        wts = rng.uniform(0.5, 20.0, len(vv)).astype(f32)
        f.write(np.array([P, len(vv)], np.int32).tobytes()); f.write(f32(1.7).tobytes())
        f.write(pts.tobytes()); f.write(vs.tobytes()); f.write(vv.tobytes()); f.write(wts.tobytes())
    subprocess.check_call([exe, str(inp), str(out)])
    for i, (d, c, n, bgr) in enumerate(maps):
        rgb = np.frombuffer(open(out / ("depth%d.rgb" % i), "rb").read(), np.uint8).reshape(d.shape + (3,))
        cases.same_image(rgb, mx.depth_map_to_image(d)[0], "DepthImage(%d)" % i)
        gray = np.frombuffer(open(out / ("conf%d.gray" % i), "rb").read(), np.uint8).reshape(d.shape)
        cases.same_image(gray, mx.conf_map_to_image(c)[0], "ConfImage(%d)" % i)
        with_n = i != 1
        want = str(tmp_path / "want.ply")
        assert plyio.save_view_cloud(want, mx.view_point_cloud(*cams[i], d, n if with_n else None, bgr), with_n)
        assert open(out / ("view%d.ply" % i), "rb").read() == open(want, "rb").read(), "ViewCloud(%d)" % i
    cloud = dict(nPoints=P, points=pts, viewStart=vs, views=vv, weights=wts, colors=None, normals=None)
    K, R, C = ([c[k] for c in cams] for k in range(3))
    want = str(tmp_path / "want.ply")
    for name, kw in (("cloud_scale.ply", dict(scales=mx.point_scales(pts, vs, vv, wts, K, R, C, 1.7))), ("cloud_views.ply", {}), ("cloud_2views.ply", dict(min_views=2))):
        assert plyio.save_point_cloud(want, cloud, **kw)
        assert open(out / name, "rb").read() == open(want, "rb").read(), name
    assert not (out / "cloud_none.ply").exists()


def test_export_driver_under_the_emulator(tmp_path):
    from tests import emu
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so") as lib:
        _run(tmp_path, _build(str(tmp_path), lib, hip=False))


@pytest.mark.gpu
def test_export_driver_on_the_device(tmp_path):
    from openmvs_amd import build
    _run(tmp_path, _build(str(tmp_path), build.build_lib("libpmhip.so"), hip=True))
