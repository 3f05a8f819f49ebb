"""The host statement of the mesh renderer (`views.project_mesh`, `views.compute_normal_vertices`, `views.sample_mesh_with_visibility`), the PLY reader and the
depth-map export, on the CPU.  The numpy twin is pinned to the reference's own rasteriser: every face of every case of tests/mesh_project_cases.py is rendered alone
by `oracle.pyref.ref_raster_faces` (TImage::RasterizeTriangleBary, EdgeFunction, the perspective-correct barycentrics and the raster functor, verbatim in
oracle/_ref/libref_fuse.so) from the projections, depths and normals the twin forms, the per-face maps are combined by (z, face index), rotated, and compared with the
twin bit for bit.  The device kernels are compared with the twin in tests/test_emu_mesh_project.py and tests/test_zz_gpu_mesh_project.py."""
import os

import numpy as np
import pytest

from openmvs_amd import densify, dmap, meshio, mvsi, views
from oracle import pyref as pr
from tests import mesh_project_cases as cases

f32 = np.float32
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")
U64 = np.iinfo(np.uint64).max


# ---- the twin against the reference's rasteriser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.pinning
@pytest.mark.skipif(not pr.fuse_available(), reason="oracle/_ref/libref_fuse.so not built (needs /root/reference)")
@pytest.mark.parametrize("case", cases.RENDER_CASES, ids=cases.RENDER_IDS)
def test_twin_is_the_reference_rasteriser_face_by_face(case):
    want = cases.twin(case)
    N = case.normals()
    drawn = 0
    for (K, R, C, w, h), (wd, wn) in zip(case.cams, want):
        pti, z, ok, _ = views.mesh_vertex_records(K, R, C, w, h, case.V)
        best = np.full((h, w), U64, np.uint64)
        normal = np.zeros((h, w, 3), f32)
        for fi, fa in enumerate(case.F.astype(np.int64)):
            if not ok[fa].all():                                              # TRasterMesh::Project: a face with a vertex outside is skipped whole
                continue
            d, n = pr.ref_raster_faces(w, h, pti[fa], z[fa], N[fa], np.array([[0, 1, 2]], np.uint32))
            key = np.where(d > 0, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(fi), U64)
            take = key < best
            best[take] = key[take]; normal[take] = n[take]
        depth = np.where(best != U64, (best >> np.uint64(32)).astype(np.uint32).view(f32), f32(0))
        Rf = R.astype(f32)
        rotated = np.stack([((f32(0) + Rf[i, 0] * normal[..., 0]) + Rf[i, 1] * normal[..., 1]) + Rf[i, 2] * normal[..., 2] for i in range(3)], -1).astype(f32)
        cases.same_bits(wd, depth, case.name + ": depth"); cases.same_bits(wn, rotated, case.name + ": normals")
        drawn += int((depth > 0).sum())
    assert drawn > 0


@pytest.mark.parametrize("case", cases.RENDER_CASES[:12], ids=cases.RENDER_IDS[:12])
def test_twin_is_the_sequential_loop(case):
    """`depth == 0 || depth > z` face after face in index order, written out with `views._raster_face`'s own per-pixel arithmetic (the function itself overwrites
    without a depth test, so each face is drawn alone and merged here)."""
    want = cases.twin(case)
    N = case.normals()
    for (K, R, C, w, h), (wd, wn) in zip(case.cams, want):
        pti, z, ok, _ = views.mesh_vertex_records(K, R, C, w, h, case.V)
        depth = np.zeros((h, w), f32); normal = np.zeros((h, w, 3), f32)
        for fa in case.F.astype(np.int64):
            if not ok[fa].all():
                continue
            d = np.zeros((h, w), f32); n = np.zeros((h, w, 3), f32)
            views._raster_face(pti[fa], z[fa], N[fa], d, n)
            take = (d > 0) & ((depth == 0) | (depth > d))
            depth[take] = d[take]; normal[take] = n[take]
        Rf = R.astype(f32)
        rotated = np.stack([((f32(0) + Rf[i, 0] * normal[..., 0]) + Rf[i, 1] * normal[..., 1]) + Rf[i, 2] * normal[..., 2] for i in range(3)], -1).astype(f32)
        cases.same_bits(wd, depth, case.name + ": depth"); cases.same_bits(wn, rotated, case.name + ": normals")


def test_every_case_reaches_its_edge():
    for c in cases.RENDER_CASES:
        cases.twin(c)                                                         # runs the case's own predicate once
    cams, V, F, want, first = cases.visibility_edges()
    assert np.array_equal(cases.vis_twin(cams, V, F), want) and want[:first].all() and want[first:].sum() == 2
    cams, V, F, counts = cases.visibility_counts()
    assert np.array_equal(cases.vis_twin(cams, V, F).sum(1), counts)


def test_depth_only_render_and_the_raster_helper_is_untouched():
    c = cases.RENDER_CASES[0]
    K, R, C, w, h = c.cams[0]
    d, n = views.project_mesh(K, R, C, w, h, c.V, c.F)
    assert n is None
    cases.same_bits(d, cases.twin(c)[0][0], "depth only")
    # _raster_face keeps overwriting without a depth test for its callers (the dense sparse initialisation)
    dm = np.zeros((17, 33), f32)
    views._raster_face(np.array([[4, 4], [4, 12], [12, 4]], f32), np.array([2, 2, 2], f32), None, dm, None)
    views._raster_face(np.array([[4, 4], [4, 12], [12, 4]], f32), np.array([4, 4, 4], f32), None, dm, None)
    assert dm[5, 5] == 4


# ---- vertex normals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_compute_normal_vertices_is_the_face_order_loop():
    rng = np.random.default_rng(3)
    V = (rng.normal(size=(60, 3)) * [1, 1, 1e-3] + [0, 0, 100]).astype(f32)     # nearly flat and far from the origin: the sums round, so their order shows
    F = rng.integers(0, 59, (400, 3)).astype(np.uint32)                       # vertex 59 is in no face; some faces name a vertex twice
    assert (F[:, 0] == F[:, 1]).any()
    n = views.compute_normal_vertices(V, F)
    lit = np.zeros_like(V)
    for fa in F:
        e1, e2 = V[fa[1]] - V[fa[0]], V[fa[2]] - V[fa[0]]
        t = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
        for k in fa:
            lit[k] = lit[k] + t
    rev = np.zeros_like(V)
    for fa in F[::-1]:
        e1, e2 = V[fa[1]] - V[fa[0]], V[fa[2]] - V[fa[0]]
        t = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
        for k in fa:
            rev[k] = rev[k] + t
    assert not np.array_equal(lit, rev), "the order of the float sums is part of the result here"
    for k in range(len(lit)):
        d = lit[k].astype(np.float64); nv = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        lit[k] = (d * (1.0 / nv if nv else 0.0)).astype(f32)
    cases.same_bits(n, lit, "vertex normals")
    assert not n[59].any()


# ---- the cloud a mesh stands in for --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [[0, 0, 1, 1, 0, 0, 1, 0], [1, 1, 1], [0, 0, 0], [0, 1, 0, 1, 1, 1, 0, 0, 1, 1, 0], [1, 0], [0], []], ids=str)
def test_swap_remove_order_is_the_backward_loop(keep):
    assert list(views.swap_remove_order(np.array(keep, bool))) == cases.literal_swap_remove(keep)


def test_swap_remove_order_is_not_the_stable_order():
    keep = np.array([0, 0, 1, 1, 0, 0, 1, 0], bool)                           # removed points first, last and adjacent
    assert list(views.swap_remove_order(keep)) == [3, 6, 2] != list(np.nonzero(keep)[0])


def test_sample_mesh_with_visibility_is_the_reference_loop():
    sc = mvsi.load(SCENE)
    V, F = cases.scene_mesh(SCENE)
    sc.sizes = [sc.camera(i)[3:] for i in range(len(sc.images))]
    pts, start, ids = views.sample_mesh_with_visibility(sc, V, F, max_resolution=160)
    # the reference, literally: per image the scaled camera, the render, the vertex test; then the backward loop
    point_views = [[] for _ in V]
    for ID in range(len(sc.images)):
        W, H = sc.sizes[ID]
        res, _ = views.compute_max_resolution(W, H, 0, 0, 160)
        scale = res / W if W > H else res / H
        K, R, C, w, h = sc.camera(ID, (int(np.rint(W * scale)), int(np.rint(H * scale))))
        assert max(w, h) == 160
        depth = views.project_mesh(K, R, C, w, h, V, F)[0]
        assert (depth > 0).mean() > 0.2
        for v in range(len(V)):
            X = V[v].astype(np.float64) - C
            cx, cy, cz = (float((0.0 + R[i, 0] * X[0]) + R[i, 1] * X[1] + R[i, 2] * X[2]) for i in range(3))
            if f32(cz) <= 0:
                continue
            x, y, zf = f32(K[0, 2] + K[0, 0] * (cx / cz)), f32(K[1, 2] + K[1, 1] * (cy / cz)), f32(cz)
            if x >= 1 and y >= 1 and x <= f32(w - 2) and y <= f32(h - 2) and f32(zf * f32(0.985)) < depth[int(np.floor(f32(y + f32(0.5)))), int(np.floor(f32(x + f32(0.5))))]:
                point_views[v].append(ID)
    points = [v for v in range(len(V))]
    idx = len(points)
    while idx > 0:
        idx -= 1
        if len(point_views[idx]) < 2:
            points[idx] = points[-1]; points.pop(); point_views[idx] = point_views[-1]; point_views.pop()
            continue
        points[idx] = idx; point_views[idx].sort()
    assert 50 < len(points) < len(V) and points != sorted(points), "vertices leave, and the swap-remove order shows"
    cases.same_bits(pts, V[points], "points")
    assert list(np.diff(start)) == [len(p) for p in point_views] and list(ids) == [i for p in point_views for i in p]
    # the callbacks reach the same result: a renderer, and the whole visibility matrix
    calls = []
    a = views.sample_mesh_with_visibility(sc, V, F, 160, project=lambda K, R, C, w, h: (calls.append((w, h)), views.project_mesh(K, R, C, w, h, V, F)[0])[1])
    b = views.sample_mesh_with_visibility(sc, V, F, 160, visibility=lambda cams: cases.vis_twin(cams, V, F))
    assert len(calls) == 4 and all(np.array_equal(x, y) for x, y in zip(a, (pts, start, ids))) and all(np.array_equal(x, y) for x, y in zip(b, (pts, start, ids)))


# ---- PLY -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", (True, False), ids=("binary", "ascii"))
def test_ply_round_trip(tmp_path, binary):
    rng = np.random.default_rng(8)
    V = (rng.normal(size=(50, 3)) * 10 ** rng.uniform(-6, 6, (50, 1))).astype(f32)
    V[0] = [0.1, -0.0, np.finfo(f32).max]; V[1] = [np.finfo(f32).tiny, 1e-45, -1.5]
    F = rng.integers(0, 50, (90, 3)).astype(np.uint32)
    p = str(tmp_path / "m.ply")
    meshio.save_ply(p, V, F, binary=binary)
    V2, F2 = meshio.load_ply(p)
    assert V2.dtype == f32 and F2.dtype == np.uint32 and np.array_equal(cases.bits(V2), cases.bits(V)) and np.array_equal(F2, F)
    assert open(p, "rb").read(40).startswith(b"ply\nformat " + (b"binary_little_endian" if binary else b"ascii") + b" 1.0\n")


def _ply(tmp_path, header, body=b""):
    p = str(tmp_path / "x.ply")
    with open(p, "wb") as f:
        f.write(header.encode() + body)
    return p


HEAD = "ply\nformat %s 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n%selement face %d\nproperty list uchar %s %s\n%send_header\n"


def test_ply_reads_what_other_writers_add(tmp_path):
    """Normals and colours on the vertices, `vertex_index` with uint indices, texture coordinates on the faces, an element of its own: skipped, binary and ascii."""
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("red", "u1")])
    v = np.zeros(3, vdt); v["x"] = [0, 1, 0]; v["y"] = [0, 0, 1]; v["z"] = 2; v["nx"] = 7; v["red"] = 200
    face = b"\x03" + np.array([0, 1, 2], "<u4").tobytes() + b"\x06" + np.arange(6, dtype="<f4").tobytes() + np.array([5], "<i4").tobytes()
    extra = np.array([1.5, 2.5], "<f8").tobytes()
    head = HEAD % ("binary_little_endian", "property float nx\nproperty uchar red\n", 1, "uint", "vertex_index", "property list uchar float texcoord\nproperty int texnumber\nelement camera 2\nproperty double f\n")
    V, F = meshio.load_ply(_ply(tmp_path, head, v.tobytes() + face + extra))
    assert np.array_equal(V, [[0, 0, 2], [1, 0, 2], [0, 1, 2]]) and np.array_equal(F, [[0, 1, 2]])
    head = HEAD % ("ascii", "property float nx\nproperty uchar red\n", 1, "int", "vertex_indices", "property list uchar float texcoord\nelement camera 1\nproperty double f\n")
    V, F = meshio.load_ply(_ply(tmp_path, head, b"0 0 2 7 200\n1 0 2 7 200\n0 1 2 7 200\n3 0 1 2 6 0 0 1 0 0 1\n1.5\n"))
    assert np.array_equal(V, [[0, 0, 2], [1, 0, 2], [0, 1, 2]]) and np.array_equal(F, [[0, 1, 2]])


REFUSALS = [
    ("not a PLY", "plx\n", b""),
    ("format binary_big_endian", HEAD.replace("%s 1.0", "binary_big_endian 1.0", 1) % ("", 1, "int", "vertex_indices", ""), b""),
    ("property x is double|x is double", HEAD.replace("property float x", "property double x") % ("ascii", "", 1, "int", "vertex_indices", ""), b""),
    ("no property z", HEAD.replace("property float z\n", "") % ("ascii", "", 1, "int", "vertex_indices", ""), b""),
    ("no list vertex_indices", HEAD % ("ascii", "", 1, "int", "corners", ""), b""),
    ("u2 count|ushort", HEAD.replace("list uchar", "list ushort") % ("ascii", "", 1, "int", "vertex_indices", ""), b""),
    ("i2 indices|short", HEAD % ("ascii", "", 1, "short", "vertex_indices", ""), b""),
    ("face 0 has 4 vertices", HEAD % ("ascii", "", 1, "int", "vertex_indices", ""), b"0 0 0\n1 0 0\n0 1 0\n4 0 1 2 0\n"),
    ("face 1 has 4 vertices", HEAD % ("binary_little_endian", "", 2, "int", "vertex_indices", ""),
     np.zeros(9, "<f4").tobytes() + b"\x03" + np.array([0, 1, 2], "<i4").tobytes() + b"\x04" + np.array([0, 1, 2, 0], "<i4").tobytes()),
    ("names vertex 3 of 3", HEAD % ("ascii", "", 1, "int", "vertex_indices", ""), b"0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n"),
    ("names vertex -1 of 3", HEAD % ("ascii", "", 1, "int", "vertex_indices", ""), b"0 0 0\n1 0 0\n0 1 0\n3 0 1 -1\n"),
    ("ends after", HEAD % ("binary_little_endian", "", 1, "int", "vertex_indices", ""), np.zeros(5, "<f4").tobytes()),
    ("ends inside record 0", HEAD % ("binary_little_endian", "", 1, "int", "vertex_indices", ""), np.zeros(9, "<f4").tobytes() + b"\x03\x00"),
    ("too few values", HEAD % ("ascii", "", 1, "int", "vertex_indices", ""), b"0 0 0\n1 0\n0 1 0\n3 0 1 2\n"),
    ("unknown type quad", HEAD.replace("property float y", "property quad y") % ("ascii", "", 1, "int", "vertex_indices", ""), b""),
    ("0 elements named face", "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n", b"0 0 0\n"),
    ("header does not end", "ply\nformat ascii 1.0\nelement vertex 1\n", b""),
]


@pytest.mark.parametrize("what, header, body", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ply_refusals_name_what_they_met(tmp_path, what, header, body):
    with pytest.raises(ValueError, match=what):
        meshio.load_ply(_ply(tmp_path, header, body))


def test_save_ply_refuses_a_face_outside_the_vertices(tmp_path):
    with pytest.raises(ValueError, match="names a vertex"):
        meshio.save_ply(str(tmp_path / "m.ply"), np.zeros((3, 3), f32), [[0, 1, 3]])


# ---- the export ------------------------------------------------------------------------------------------------------------------------------------------------
def test_export_mesh_depth_maps_writes_what_the_reference_writes(tmp_path):
    V, F = cases.scene_mesh(SCENE)
    sv = densify.load_scene(SCENE, opt=cases.mesh_options())
    ply = str(tmp_path / "surface.ply")
    meshio.save_ply(ply, V, F)
    names = densify.export_mesh_depth_maps(sv, ply, str(tmp_path / "gt.dmap"))
    assert [os.path.basename(n) for n in names] == ["gt%04d.dmap" % i for i in range(4)]
    N = views.compute_normal_vertices(V, F)
    for i, name in enumerate(names):
        g = dmap.load(name)
        w, h = sv.sizes[i]
        d, n = views.project_mesh(sv.K[i], sv.R[i], sv.C[i], w, h, V, F, N)
        assert (g["depth_width"], g["depth_height"], g["image_width"], g["image_height"]) == (w, h, w, h) and (d > 0).mean() > 0.2
        assert g["depth_min"] == f32(0.001) and g["depth_max"] == np.finfo(f32).max and g["has_normal"] and not g["has_conf"] and not g["has_views"]
        assert g["reference_view_id"] == i and g["neighbor_view_ids"] == [int(k) for k in sv.all_view_scores[i]["ID"]] and g["file_name"] == sv.names[i]
        assert np.array_equal(g["K"], sv.K[i]) and np.array_equal(g["R"], sv.R[i]) and np.array_equal(g["C"], sv.C[i])
        cases.same_bits(g["depth_map"], d, "depth of " + name); cases.same_bits(g["normal_map"], n, "normals of " + name)
    pfm = densify.export_mesh_depth_maps(sv, (V, F), str(tmp_path / "depth.PFM"))
    raw = open(pfm[2], "rb").read()
    w, h = sv.sizes[2]
    head = b"Pf\n%d %d\n-1.000000\n" % (w, h)
    assert raw.startswith(head) and len(raw) == len(head) + 4 * w * h and os.path.basename(pfm[2]) == "depth0002.PFM"
    cases.same_bits(np.frombuffer(raw[len(head):], "<f4").reshape(h, w)[::-1], views.project_mesh(sv.K[2], sv.R[2], sv.C[2], w, h, V, F)[0], "pfm rows bottom to top")
    for bad in ("gt.png", "gt", "gt.dmap.bak"):
        with pytest.raises(ValueError, match="extension"):
            densify.export_mesh_depth_maps(sv, (V, F), str(tmp_path / bad))
