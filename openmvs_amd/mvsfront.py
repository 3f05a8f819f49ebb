"""ctypes binding of libmvsfront.so (include/mvsfront.h): the C++ scene front end -- MVSI reader, pixel cameras, neighbour-view selection,
sparse depth initialisation.  Same results as the numpy implementation in mvsi.py / views.py (tests/test_mvsfront.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi, build as _build

VIEW_SCORE_DTYPE = np.dtype([("ID", "<u4"), ("points", "<u4"), ("scale", "<f4"), ("angle", "<f4"), ("area", "<f4"), ("score", "<f4")])


class MVSFOptions(C.Structure):
    _fields_ = [("nMinViews", C.c_uint32), ("nMaxViews", C.c_uint32), ("nMinViewsTrustPoint", C.c_uint32), ("nNumViews", C.c_uint32), ("nPointInsideROI", C.c_uint32),
                ("fViewMinScore", C.c_float), ("fViewMinScoreRatio", C.c_float), ("fMinArea", C.c_float), ("fMinAngle", C.c_float), ("fOptimAngle", C.c_float), ("fMaxAngle", C.c_float)]


_TYPES = {"MVSFViewScore": VIEW_SCORE_DTYPE, "MVSFOptions": MVSFOptions}          # the mirrors by their names in include/mvsfront.h
_SIGNATURES = _cabi.signatures("mvsfront.h", _TYPES)
EXPORTS = list(_SIGNATURES)          # every function include/mvsfront.h declares
_MESH_SIGNATURES = _cabi.signatures("mvsfront_mesh.h", _TYPES)          # ... and its companion header, which mvsfront.h includes
MESH_EXPORTS = list(_MESH_SIGNATURES)
_LIB = None


def load_library() -> C.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = _cabi.declare(_cabi.declare(C.CDLL(_build.build_host_lib("libmvsfront.so")), _SIGNATURES), _MESH_SIGNATURES)
    return _LIB


def default_options(**kw) -> MVSFOptions:
    o = MVSFOptions(); load_library().mvsf_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class SceneFront:
    def __init__(self, path: str):
        self._lib = load_library(); self._h = C.c_void_p()
        rc = self._lib.mvsf_load(path.encode(), C.byref(self._h))
        if rc != 0:
            raise ValueError("mvsf_load(%s) failed: %d" % (path, rc))
        self.version = self._lib.mvsf_version(self._h); self.n_images = self._lib.mvsf_num_images(self._h); self.n_points = self._lib.mvsf_num_points(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mvsf_free(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image_info(self, i):
        name = C.create_string_buffer(1024); w = C.c_int(); h = C.c_int(); v = C.c_int()
        assert self._lib.mvsf_image_info(self._h, i, name, 1024, C.byref(w), C.byref(h), C.byref(v)) == 0
        return name.value.decode(), w.value, h.value, bool(v.value)

    def point(self, i):
        X = np.zeros(3, np.float32); n = C.c_int(); views = np.zeros(64, np.uint32)
        assert self._lib.mvsf_point(self._h, i, X, views, 64, C.byref(n)) == 0
        return X, views[:n.value].copy()

    def camera(self, i, size=(0, 0)):
        K = np.zeros((3, 3)); R = np.zeros((3, 3)); Cc = np.zeros(3)
        rc = self._lib.mvsf_camera(self._h, i, size[0], size[1], K, R, Cc)
        if rc != 0:
            raise ValueError("mvsf_camera failed: %d" % rc)
        return K, R, Cc

    def neighbors(self, i):
        """The neighbour list image i carries (archive view scores or a view-neighbours file); empty = to be selected from the sparse points."""
        n = C.c_int()
        assert self._lib.mvsf_get_neighbors(self._h, i, None, 0, C.byref(n)) == 0
        nb = np.zeros(n.value, VIEW_SCORE_DTYPE)
        assert self._lib.mvsf_get_neighbors(self._h, i, nb, len(nb), C.byref(n)) == 0
        return nb

    def set_neighbors(self, i, nb):
        nb = np.ascontiguousarray(nb, VIEW_SCORE_DTYPE)
        if self._lib.mvsf_set_neighbors(self._h, i, nb, len(nb)) != 0:
            raise ValueError("mvsf_set_neighbors(%d)" % i)

    def load_view_neighbors(self, path: str):
        """Scene::LoadViewNeighbors (`--view-neighbors-file`)."""
        rc = self._lib.mvsf_load_view_neighbors(self._h, path.encode())
        if rc != 0:
            raise ValueError("mvsf_load_view_neighbors(%s) failed: %d" % (path, rc))

    def save_view_neighbors(self, path: str):
        if self._lib.mvsf_save_view_neighbors(self._h, path.encode()) != 0:
            raise OSError("cannot write %s" % path)

    def image_depths(self, i):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        assert self._lib.mvsf_image_depths(self._h, i, C.byref(a), C.byref(b), C.byref(c)) == 0
        return a.value, b.value, c.value

    def select_neighbor_views(self, i, nMinViews=2, nMinPointViews=2, fOptimAngle=12.0, nInsideROI=1, sizes=None):
        nb = np.zeros(self.n_images, VIEW_SCORE_DTYPE); pts = np.zeros(self.n_points, np.uint32); nn = C.c_int(); npts = C.c_int(); avg = C.c_float()
        ps = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
        rc = self._lib.mvsf_select_neighbor_views(self._h, i, ps, nMinViews, nMinPointViews, fOptimAngle, nInsideROI, nb, len(nb), C.byref(nn), pts, len(pts), C.byref(npts), C.byref(avg))
        return rc == 0, nb[:nn.value].copy(), pts[:npts.value].copy(), float(avg.value)

    def select_views(self, i, opt=None, sizes=None):
        opt = opt or default_options()
        nb = np.zeros(self.n_images, VIEW_SCORE_DTYPE); pts = np.zeros(self.n_points, np.uint32); nn = C.c_int(); npts = C.c_int(); avg = C.c_float()
        ps = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
        rc = self._lib.mvsf_select_views(self._h, i, ps, C.byref(opt), nb, len(nb), C.byref(nn), pts, len(pts), C.byref(npts), C.byref(avg))
        if rc != 0:
            return None
        return nb[:nn.value].copy(), pts[:npts.value].copy(), float(avg.value)

    def init_depth_map(self, i, points, size, nMinViewsTrustPoint=2, dense=False):
        """dense: OPTDENSE::bInitSparse = 0 (rasterised triangles instead of 2x2 splats)."""
        w, h = size
        d = np.zeros((h, w), np.float32); n = np.zeros((h, w, 3), np.float32); dmin = C.c_float(); dmax = C.c_float()
        p = np.ascontiguousarray(points, np.uint32)
        if dense:
            rc = self._lib.mvsf_init_depth_map_dense(self._h, i, w, h, p, len(p), d, n, C.byref(dmin), C.byref(dmax))
        else:
            rc = self._lib.mvsf_init_depth_map(self._h, i, w, h, p, len(p), nMinViewsTrustPoint, d, n, C.byref(dmin), C.byref(dmax))
        if rc != 0:
            raise ValueError("mvsf_init_depth_map failed: %d" % rc)
        return d, n, float(dmin.value), float(dmax.value)

    def triangulate_depth_map(self, i, points, size, avg_depth=None, sparse=False):
        """mvsf_triangulate_depth_map: avg_depth not None = with the image corners.  -> (depthMap, dMin, dMax)."""
        w, h = size
        d = np.zeros((h, w), np.float32); dmin = C.c_float(); dmax = C.c_float()
        p = np.ascontiguousarray(points, np.uint32)
        rc = self._lib.mvsf_triangulate_depth_map(self._h, i, w, h, p, len(p), avg_depth is not None, avg_depth or 0.0, bool(sparse), d, C.byref(dmin), C.byref(dmax))
        if rc != 0:
            raise ValueError("mvsf_triangulate_depth_map failed: %d" % rc)
        return d, float(dmin.value), float(dmax.value)

    def point_mesh(self, i, points, size, avg_depth=None, normals=True):
        """mvsf_point_mesh: the mesh `init_depth_map` / `triangulate_depth_map` rasterise (avg_depth not None = with the image corners), as `views.point_mesh` returns it
        -> (proj (n,2) f32, vert_z (n,) f32, normals (n,3) f32 | None, faces (m,3) uint32, dMin, dMax): the bounds of the points themselves, without the 0.9 / 1.1."""
        w, h = size
        p = np.ascontiguousarray(points, np.uint32)
        nv, nf, dmin, dmax = C.c_int(), C.c_int(), C.c_float(), C.c_float()
        cap = len(p) + 4                                       # the points and the corners; a planar triangulation of n vertices has fewer than 2 n faces: one call
        proj = np.zeros((cap, 2), np.float32); z = np.zeros(cap, np.float32); nrm = np.zeros((cap, 3), np.float32) if normals else None
        faces = np.zeros((2 * cap, 3), np.uint32)
        rc = self._lib.mvsf_point_mesh(self._h, i, w, h, p, len(p), avg_depth is not None, avg_depth or 0.0, proj, z, nrm, cap, C.byref(nv), faces, 2 * cap, C.byref(nf),
                                       C.byref(dmin), C.byref(dmax))
        if rc != 0:
            raise ValueError("mvsf_point_mesh failed: %d" % rc)
        proj, z, faces = proj[:nv.value].copy(), z[:nv.value].copy(), faces[:nf.value].copy()
        nrm = None if nrm is None else nrm[:nv.value].copy()
        return proj, z, nrm, faces, float(dmin.value), float(dmax.value)


def estimate_normal_map(K, depth):
    """mvsf_estimate_normal_map (MVS::EstimateNormalMap): K 3x3, depth [h, w] -> normals [h, w, 3] float32."""
    d = np.ascontiguousarray(depth, np.float32); h, w = d.shape
    k = np.ascontiguousarray(np.asarray(K, np.float64).ravel())
    out = np.zeros((h, w, 3), np.float32)
    rc = load_library().mvsf_estimate_normal_map(k, d, w, h, out)
    if rc != 0:
        raise ValueError("mvsf_estimate_normal_map: %d" % rc)
    return out
