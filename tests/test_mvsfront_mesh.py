"""mvsf_point_mesh (include/mvsfront_mesh.h): the C++ front end returns the mesh `views.point_mesh` builds -- projections, depths, vertex normals and faces compared as
arrays, bit for bit, nothing rasterised -- with and without the image corners, at two sizes; the counts come back when the capacities are 0; and the existing
functions, rebuilt on the shared vertex-normal code, rasterise that mesh as before."""
import ctypes as C
import os

import numpy as np
import pytest

from openmvs_amd import mvsfront, mvsi, views

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes():
    cf = mvsfront.SceneFront(SCENE)
    yield cf, mvsi.load(SCENE)
    cf.close()


@pytest.mark.parametrize("size", [(640, 479), (320, 240), (80, 60)])
@pytest.mark.parametrize("corners", [False, True], ids=["plain", "corners"])
def test_point_mesh_is_the_mesh_of_views_point_mesh(scenes, size, corners):
    cf, py = scenes
    cams = views.Cameras(py, [size] * len(py.images))
    for ID in (0, 3):
        _, pts, avg = views.select_views(py, cams, ID, views.DenseOptions())
        proj, z, vz, nrm, faces, dmin, dmax = views.point_mesh(py, cams, ID, pts, views.DenseOptions(bAddCorners=corners), avg if corners else None)
        cp, cz, cn, cfaces, cmin, cmax = cf.point_mesh(ID, pts, size, avg if corners else None)
        assert len(vz) == len(pts) + (4 if corners else 0) > 1000 and len(faces) > 2000
        assert np.array_equal(u32(cp), u32(proj)) and np.array_equal(u32(cz), u32(vz)) and np.array_equal(u32(cn), u32(nrm))
        assert cfaces.dtype == np.uint32 and np.array_equal(cfaces, faces)
        assert cmin == float(z.min()) and cmax == float(z.max())                                           # the bounds of the points: the corners do not count
        assert dmin == float(np.float32(cmin) * np.float32(0.9)) and dmax == float(np.float32(cmax) * np.float32(1.1))   # the caller applies InitViews' 0.9 / 1.1
        assert cf.point_mesh(ID, pts, size, avg if corners else None, normals=False)[2] is None
        if corners:
            assert np.array_equal(cp[-4:], np.array([(0, 0), (size[0] - 1, 0), (0, size[1] - 1), (size[0] - 1, size[1] - 1)], np.float32)) and (cz[-4:] > 0).all()


def test_counts_come_back_when_the_capacities_are_zero(scenes):
    cf, py = scenes
    size = (320, 240)
    cams = views.Cameras(py, [size] * len(py.images))
    pts = np.ascontiguousarray(views.select_views(py, cams, 0, views.DenseOptions())[1], np.uint32)
    lib, nv, nf, mn, mx = cf._lib, C.c_int(-1), C.c_int(-1), C.c_float(), C.c_float()
    assert lib.mvsf_point_mesh(cf._h, 0, *size, pts, len(pts), 0, 0.0, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(mn), C.byref(mx)) == 0
    want = cf.point_mesh(0, pts, size)
    assert nv.value == len(pts) == len(want[1]) and nf.value == len(want[3]) and (mn.value, mx.value) == want[4:]
    proj = np.full((nv.value, 2), 7, np.float32); z = np.full(nv.value, 7, np.float32); faces = np.full((nf.value, 3), 7, np.uint32)
    # too small a capacity: -2, the counts, and nothing written
    assert lib.mvsf_point_mesh(cf._h, 0, *size, pts, len(pts), 0, 0.0, proj, z, None, nv.value - 1, C.byref(nv), faces, nf.value, C.byref(nf), None, None) == -2
    assert lib.mvsf_point_mesh(cf._h, 0, *size, pts, len(pts), 0, 0.0, proj, z, None, nv.value, C.byref(nv), faces, nf.value - 1, C.byref(nf), None, None) == -2
    assert (proj == 7).all() and (z == 7).all() and (faces == 7).all() and nv.value == len(pts)
    assert lib.mvsf_point_mesh(cf._h, 0, *size, pts, len(pts), 0, 0.0, proj, z, None, nv.value, C.byref(nv), faces, nf.value, C.byref(nf), None, None) == 0   # normals and bounds are optional
    assert np.array_equal(u32(proj), u32(want[0])) and np.array_equal(faces, want[3])
    # no points: an empty mesh, not an error; a point index outside the scene, an image outside the scene: -1
    assert lib.mvsf_point_mesh(cf._h, 0, *size, None, 0, 1, 5.0, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(mn), C.byref(mx)) == 0 and (nv.value, nf.value) == (0, 0)
    assert mn.value > 3e38 and mx.value == 0
    empty = cf.point_mesh(0, np.zeros(0, np.uint32), size, 5.0)
    assert empty[0].shape == (0, 2) and empty[3].shape == (0, 3)
    bad = np.array([cf.n_points], np.uint32)
    assert lib.mvsf_point_mesh(cf._h, 0, *size, bad, 1, 0, 0.0, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), None, None) == -1
    assert lib.mvsf_point_mesh(cf._h, cf.n_images, *size, pts, len(pts), 0, 0.0, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), None, None) == -1


def test_the_existing_functions_rasterise_that_mesh(scenes):
    """mvsf_triangulate_depth_map (depth only, with corners) is the face walk over mvsf_point_mesh's arrays; mvsf_init_depth_map's splats carry its depths."""
    cf, py = scenes
    size = (80, 60)
    cams = views.Cameras(py, [size] * len(py.images))
    _, pts, avg = views.select_views(py, cams, 0, views.DenseOptions())
    proj, vz, _, faces, mn, mx = cf.point_mesh(0, pts, size, avg)
    d, dmn, dmx = cf.triangulate_depth_map(0, pts, size, avg)
    assert np.array_equal(u32(d), u32(views.raster_faces_depth_map(proj, vz, faces.astype(np.int64), *size))) and (dmn, dmx) == (mn, mx) and (d > 0).all()
    proj, vz, _, _, _, _ = cf.point_mesh(0, pts, size)
    ds = cf.init_depth_map(0, pts, size)[0]
    want = np.zeros_like(ds)
    for (x, y), zz in zip(np.floor(proj).astype(np.int64), vz):
        want[max(y, 0):min(y + 2, size[1]), max(x, 0):min(x + 2, size[0])] = zz
    assert np.array_equal(u32(ds), u32(want))
