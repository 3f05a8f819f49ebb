"""Cases of the mesh renderer (csrc/pm_mesh.hip, include/pmhip_mesh.h), shared by the host-twin suite (tests/test_mesh_project.py), the emulator suite
(tests/test_emu_mesh_project.py) and the device suite (tests/test_zz_gpu_mesh_project.py).

A case is a mesh, a list of cameras and a `prove` function: a predicate on the case's own inputs or on the host twin's intermediate results that shows the case
reaches the edge it is named after (an assertion, so a case that drifts off its edge fails instead of passing for nothing).  The twin's result of every case is computed
once (`twin`) and never modified.  Every comparison is bit for bit.

The exact cases use the camera K = I, R = I, C = 0, under which the vertex (px * z, py * z, z) projects to (px, py) exactly whenever the products are exact in float
(small px, z a short binary fraction): TransformPointW2C subtracts 0 and multiplies by 1 and 0, TransformPointC2I divides the exact product by z."""
import numpy as np

from openmvs_amd import views

f32 = np.float32
I3 = np.eye(3)
ALL_SMALL = 1 << 30          # box thresholds: every face walked by one lane ...
ALL_LARGE = 1                # ... and every face of more than one pixel by a workgroup
DEFAULT_BOX = 64             # PM_MESH_BOX_PIXELS (csrc/pm_engine.hip); `threshold_case` proves it
DEFAULT_BATCH = 4 << 30      # PM_MESH_BATCH_BYTES: every case fits one batch; a budget of 1 byte renders one view per batch


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %s: %r != %r" % (what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def cam(w, h, f=1.0, cx=0.0, cy=0.0, R=I3, C=(0.0, 0.0, 0.0)):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64), np.array(R, np.float64), np.array(C, np.float64), int(w), int(h)


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


class Soup:
    """Faces with vertices of their own, given as (px, py, z) under the exact camera."""

    def __init__(self):
        self.V, self.F, self.N = [], [], []

    def vertex(self, px, py, z, n=(0.0, 0.0, -1.0)):
        self.V.append((f32(px) * f32(z), f32(py) * f32(z), f32(z))); self.N.append(n)
        return len(self.V) - 1

    def face(self, a, b, c, n=((0.0, 0.0, -1.0),) * 3):
        ids = [self.vertex(*p, n=k) for p, k in zip((a, b, c), n)]
        self.F.append(ids)
        return len(self.F) - 1

    def arrays(self):
        return np.array(self.V, f32).reshape(-1, 3), np.array(self.F, np.uint32).reshape(-1, 3), np.array(self.N, f32).reshape(-1, 3)


class Case:
    def __init__(self, name, cams, V, F, N=None, prove=None, boxes=(-1, ALL_SMALL, ALL_LARGE), large=None, batch_bytes=(0,), batches=None):
        self.name, self.cams, self.V, self.F, self.N, self.prove = name, list(cams), np.ascontiguousarray(V, f32), np.ascontiguousarray(F, np.uint32), N, prove
        self.boxes, self.large, self.batch_bytes, self.batches = tuple(boxes), large, tuple(batch_bytes), batches

    def normals(self):
        return views.compute_normal_vertices(self.V, self.F) if self.N is None else np.ascontiguousarray(self.N, f32)

    def candidates(self, k=0):
        K, R, C, w, h = self.cams[k]
        pti, z, ok, front = views.mesh_vertex_records(K, R, C, w, h, self.V)
        return (pti, z, ok, front) + views.mesh_candidates(pti, z, ok, self.F, w, h)


_TWIN = {}


def twin(case):
    """[(depth, normal)] of `views.project_mesh` per camera, computed once per case (read-only), after the case has proved itself on it."""
    if case.name not in _TWIN:
        out = []
        for K, R, C, w, h in case.cams:
            d, n = views.project_mesh(K, R, C, w, h, case.V, case.F, case.normals())
            d.setflags(write=False); n.setflags(write=False)
            out.append((d, n))
        if case.prove:
            case.prove(case, out)
        _TWIN[case.name] = out
    return _TWIN[case.name]


def run_case(engine, case):
    """The case through pmhip_mesh_project at every box threshold (and batch budget) it lists, against the twin; the routes taken are checked where the case says which."""
    want = twin(case)
    K, R, C = (np.array([c[k] for c in case.cams]) for k in range(3))
    sizes = [c[3:] for c in case.cams]
    try:
        got_n = engine.mesh_set(case.V, case.F, case.N)
        same_bits(got_n, case.normals(), case.name + ": vertex normals")
        for bi, box in enumerate(case.boxes):
            for ci, bb in enumerate(case.batch_bytes):
                engine.mesh_tuning(box_pixels=box, batch_bytes=bb if bb else DEFAULT_BATCH)
                what = "%s (box %d, batch bytes %d)" % (case.name, box, bb)
                got = engine.mesh_project(K, R, C, sizes, normals=True)
                st = engine.mesh_tuning()
                for v, ((d, n), (wd, wn)) in enumerate(zip(got, want)):
                    same_bits(d, wd, "%s: depth of view %d" % (what, v)); same_bits(n, wn, "%s: normals of view %d" % (what, v))
                if case.large is not None:
                    assert st["large_faces"] == case.large[bi], "%s: %d faces took the workgroup route, expected %d" % (what, st["large_faces"], case.large[bi])
                if case.batches is not None:
                    assert st["batches"] == case.batches[ci], "%s: %d batches, expected %d" % (what, st["batches"], case.batches[ci])
                depth_only = engine.mesh_project(K, R, C, sizes, normals=[v % 2 == 1 for v in range(len(sizes))])
                for v, ((d, n), (wd, wn)) in enumerate(zip(depth_only, want)):
                    same_bits(d, wd, "%s: depth of view %d, mixed call" % (what, v))
                    assert (n is None) == (v % 2 == 0)
                    if n is not None:
                        same_bits(n, wn, "%s: normals of view %d, mixed call" % (what, v))
    finally:
        engine.mesh_tuning(box_pixels=-1, batch_bytes=DEFAULT_BATCH)
        engine.mesh_release()


# ---- the exact cases ---------------------------------------------------------------------------------------------------------------------------------------
UP, SIDE = (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)


def edge_case():
    s = Soup(); s.face((4, 4, 2), (4, 12, 2), (12, 4, 2))

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        on_edge = pix == 8 * 33 + 8                                        # (8, 8) lies on the hypotenuse x + y = 16
        assert on_edge.sum() == 1 and pb[on_edge][0, 0] == 0 and out[0][0][8, 8] > 0 and out[0][0][9, 8] == 0
        assert out[0][0][4, 4] > 0 and out[0][0][12, 4] > 0 and out[0][0][4, 12] > 0     # the corners themselves: two barycentrics are 0
    V, F, N = s.arrays()
    return Case("one face, edges through pixel centres", [cam(33, 17)], V, F, N, prove)


def shared_edge_case(z_second):
    s = Soup(); s.face((4, 4, 2), (4, 12, 2), (12, 4, 2), n=(UP,) * 3); s.face((12, 12, z_second), (12, 4, z_second), (4, 12, z_second), n=(SIDE,) * 3)

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        at = pix == 8 * 33 + 8
        assert sorted(face[at]) == [0, 1], "both faces own the centre on their common edge"
        if z_second == 2:
            assert bits(zz[at])[0] == bits(zz[at])[1] and out[0][1][8, 8, 2] == -1 and out[0][1][8, 8, 1] == 0       # an exact tie: the lower index
        else:
            assert out[0][1][8, 8, 1] == 1                                                                           # the nearer face, although listed second
    V, F, N = s.arrays()
    return Case("two faces sharing an edge, second at z %g" % z_second, [cam(33, 17)], V, F, N, prove)


def twice_case(reverse):
    s = Soup(); s.face((4, 4, 2), (4, 12, 4), (12, 4, 2), n=(UP,) * 3); s.face((4, 4, 2), (4, 12, 4), (12, 4, 2), n=(SIDE,) * 3)
    V, F, N = s.arrays()
    if reverse:
        F = F[::-1].copy()

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        assert len(pix) == 2 * len(np.unique(pix)) and np.array_equal(bits(zz[face == 0]), bits(zz[face == 1])), "every pixel is an exact z tie"
        hit = out[0][0] > 0
        assert hit.sum() > 30 and (out[0][1][hit][:, 1 if reverse else 2] == (1 if reverse else -1)).all()          # face 0 of the list as given
    return Case("the same face under two indices" + (", list reversed" if reverse else ""), [cam(33, 17)], V, F, N, prove)


def far_near_case(near_first):
    s = Soup()
    far, near = ((4, 4, 4), (4, 12, 4), (12, 4, 4)), ((5, 5, 2), (5, 11, 2), (11, 5, 2))
    for t, n in ((near, SIDE), (far, UP)) if near_first else ((far, UP), (near, SIDE)):
        s.face(*t, n=(n,) * 3)

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        both = np.intersect1d(pix[face == 0], pix[face == 1])
        assert len(both) > 10 and (out[0][1].reshape(-1, 3)[both][:, 1] == 1).all() and (out[0][0].reshape(-1)[both] < 3).all()
    V, F, N = s.arrays()
    return Case("a far and a near face, near %s" % ("first" if near_first else "second"), [cam(33, 17)], V, F, N, prove)


def dropped_case():
    s = Soup()
    s.face((4, 4, 2), (12, 4, 2), (4, 12, 2))                  # 0 back-facing
    s.face((4, 4, 2), (6, 6, 2), (8, 8, 2))                    # 1 collinear
    a = s.vertex(5, 5, 2); b = s.vertex(9, 9, 2); s.F.append([a, a, b])          # 2 a vertex twice
    s.face((4.25, 4.25, 2), (4.25, 4.75, 2), (4.75, 4.25, 2))  # 3 front-facing, covers no centre
    s.face((20, 4, 2), (20, 8, 2), (24, 4, 2))                 # 4 drawn

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        assert ok.all() and set(face) == {4} and out[0][0][4, 20] > 0
        x, y = pti[c.F[3]][:, 0].astype(np.float64), pti[c.F[3]][:, 1].astype(np.float64)
        assert (x[2] - x[0]) * (y[1] - y[0]) - (y[2] - y[0]) * (x[1] - x[0]) > 0, "the sliver faces the camera"
    V, F, N = s.arrays()
    return Case("back-facing, empty and sliver faces", [cam(33, 17)], V, F, N, prove)


def limits_case():
    w, h = 33, 17
    below = lambda v: np.nextafter(f32(v), f32(-1e9)); above = lambda v: np.nextafter(f32(v), f32(1e9))
    specials = [("z < 0", (5, 5, -1), False), ("z == 0", (5, 5, 0), False), ("z just above 0", (5, 5, 2.0 ** -20), True),
                ("x on the limit", (3, 5, 1), True), ("x one ulp outside", (below(3), 5, 1), False), ("x one ulp inside", (above(3), 5, 1), True),
                ("x on the far limit", (w - 4, 5, 1), True), ("x one ulp past it", (above(w - 4), 5, 1), False), ("x one ulp before it", (below(w - 4), 5, 1), True),
                ("y on the limit", (5, 3, 1), True), ("y one ulp outside", (5, below(3), 1), False),
                ("y on the far limit", (5, h - 4, 1), True), ("y one ulp past it", (5, above(h - 4), 1), False)]
    s = Soup()
    for k, (_, p, _) in enumerate(specials):                    # each face: the special vertex and two ordinary ones, ordered to face the camera; depths apart
        zz = 2.0 + k
        xs, ys = ((8, 12) if p[0] < 20 else (20, 24)), ((9, 6) if p[1] < 10 else (7, 10))
        q = [(p[0], p[1], p[2]), (xs[0], ys[0], zz), (xs[1], ys[1], zz)]
        if (float(q[2][0]) - float(q[0][0])) * (float(q[1][1]) - float(q[0][1])) - (float(q[2][1]) - float(q[0][1])) * (float(q[1][0]) - float(q[0][0])) <= 0:
            q = [q[0], q[2], q[1]]                              # (EdgeFunction's sign: the face looks at the camera)
        s.face(*q)

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        for k, (what, p, kept) in enumerate(specials):
            v = c.F[k][0]
            assert bool(ok[v]) == kept, what
            assert ok[c.F[k][1:]].all(), what
            assert (k in set(face)) == kept, "%s: the whole face is %s" % (what, "kept" if kept else "dropped")
            if p[2] > 0 and np.isfinite(p[0]):
                assert pti[v][0] == f32(p[0]) and pti[v][1] == f32(p[1]), what + ": the projection is exact"
    V, F, N = s.arrays()
    return Case("vertices at z = 0 and on the border-3 limits", [cam(w, h)], V, F, N, prove)


def whole_image_case():
    s = Soup(); s.face((3, 3, 2), (3, 29, 4), (61, 3, 8))

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        assert (pti[:, 0].max() - pti[:, 0].min() + 1) * (pti[:, 1].max() - pti[:, 1].min() + 1) == 59 * 27 and (out[0][0] > 0).sum() > 700
    V, F, N = s.arrays()
    return Case("a face whose box is the whole admissible image", [cam(65, 33)], V, F, N, prove, boxes=(-1, ALL_SMALL, 59 * 27, 59 * 27 - 1), large=(1, 0, 0, 1))


def threshold_case():
    s = Soup(); s.face((10, 4, 2), (10, 11, 2), (17, 4, 4)); s.face((20, 4, 2), (20, 6, 2), (22, 4, 2))

    def prove(c, out):
        pti = c.candidates()[0]
        assert (pti[:3, 0].max() - pti[:3, 0].min() + 1) * (pti[:3, 1].max() - pti[:3, 1].min() + 1) == DEFAULT_BOX
    V, F, N = s.arrays()
    return Case("a box of exactly the threshold's pixels", [cam(33, 17)], V, F, N, prove, boxes=(-1, DEFAULT_BOX - 1, DEFAULT_BOX, DEFAULT_BOX + 1, 8), large=(0, 1, 0, 0, 2))


def contention_case(nearest):
    n = 4096
    rng = np.random.default_rng(41)
    order = rng.permutation(n)
    at = {"first": 0, "last": n - 1, "middle": n // 2}[nearest]
    order[[at, int(np.nonzero(order == 0)[0][0])]] = order[[int(np.nonzero(order == 0)[0][0]), at]]          # depth rank 0 goes to face `at`
    s = Soup()
    nrm = rng.normal(size=(n, 3, 3))
    for k in range(n):
        z = 2.0 + float(order[k]) * 2.0 ** -10
        s.face((9.5, 9.5, z), (9.5, 10.75, z), (10.75, 9.5, z), n=[tuple(v) for v in nrm[k]])

    def prove(c, out):
        pti, z, ok, front, face, pix, zz, pb = c.candidates()
        assert len(pix) == n and (pix == 10 * 33 + 10).all() and len(np.unique(bits(zz))) == n, "4096 offers at distinct depths, all on one pixel"
        assert int(face[np.argmin(zz)]) == at and (out[0][0] > 0).sum() == 1
    V, F, N = s.arrays()
    return Case("4096 faces on one pixel, nearest %s" % nearest, [cam(33, 17)], V, F, N, prove, boxes=(-1, 4), large=(0, n))


def tiny_images_case():
    s = Soup(); s.face((3, 3, 2), (3, 4, 2), (4, 3, 2)); s.face((3, 3, 1), (3, 3, 1), (3, 3, 1))

    def prove(c, out):
        ok6, ok7, ok8 = (c.candidates(k)[2] for k in range(3))
        assert not ok6.any() and not out[0][0].any(), "6 x 6: no vertex can be inside"
        assert ok7[3:].all() and not ok7[:3].all() and not out[1][0].any(), "7 x 7: the one admissible pixel holds only an empty face"
        assert ok8.all() and out[2][0][3, 3] > 0 and out[2][0][3, 4] > 0 and out[2][0][4, 3] > 0 and out[2][0][4, 4] == 0
    V, F, N = s.arrays()
    return Case("6 x 6, 7 x 7 and 8 x 8 images", [cam(6, 6), cam(7, 7), cam(8, 8)], V, F, N, prove)


# ---- generic meshes ----------------------------------------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, x0, x1, y0, y1, z0, amp, seed):
    """A displaced (nx x ny)-cell grid that faces a camera looking along +z with x to the right and y down."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1))
    z = z0 + amp * np.sin(xs * 1.7 + 0.3) * np.cos(ys * 2.3) + amp * 0.2 * rng.random(xs.shape)
    V = np.stack([xs, ys, z], -1).reshape(-1, 3).astype(f32)
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    F = np.concatenate([np.stack([i, i + nx + 1, i + 1], 1), np.stack([i + nx + 2, i + 1, i + nx + 1], 1)]).astype(np.uint32)
    return V, F


def generic_cam(w, h, seed, dist=3.0):
    rng = np.random.default_rng(seed)
    f = 0.9 * w + rng.random()
    R = rot(*(rng.uniform(-0.12, 0.12, 3)))
    C = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), -dist + rng.uniform(-0.2, 0.2)])
    return cam(w, h, f, (w - 1) / 2 + rng.uniform(-0.5, 0.5), (h - 1) / 2 + rng.uniform(-0.5, 0.5), R, C)


def normals_case():
    V, F = grid_mesh(9, 7, -1.2, 1.2, -0.7, 0.7, 0.0, 0.15, 3)
    V = np.concatenate([V, [[5.0, 5.0, 5.0]]]).astype(f32)                                 # an isolated vertex
    lone = len(V) - 1
    F = np.concatenate([F[:40], [[3, 3, 17], [lone - 1, lone - 1, lone - 1]], F[40:]]).astype(np.uint32)     # two faces whose cross product is zero, mid-list

    def prove(c, out):
        n = c.normals()
        assert not n[lone].any() and np.abs(np.linalg.norm(n[:lone].astype(np.float64), axis=1) - 1).max() < 1e-6
        literal = np.zeros_like(c.V)
        for fa in c.F.astype(np.int64):                                                     # Mesh::ComputeNormalVertices, literally
            e1, e2 = c.V[fa[1]] - c.V[fa[0]], c.V[fa[2]] - c.V[fa[0]]
            t = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
            for k in fa:
                literal[k] = literal[k] + t
        for k in range(len(literal)):
            d = literal[k].astype(np.float64); nv = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            literal[k] = (d * (1.0 / nv if nv else 0.0)).astype(f32)
        assert np.array_equal(bits(literal), bits(n)) and (out[0][0] > 0).sum() > 500
    return Case("computed vertex normals: an isolated vertex, empty faces", [generic_cam(65, 33, 5)], V, F, None, prove)


def batch_case():
    V, F = grid_mesh(24, 12, -1.3, 1.3, -0.7, 0.7, 0.0, 0.2, 7)
    cams = [generic_cam(65, 33, 11), generic_cam(6, 6, 12), generic_cam(33, 17, 13), generic_cam(7, 7, 14), generic_cam(8, 8, 15), generic_cam(65, 33, 16, dist=1.2)]

    def prove(c, out):
        assert (out[0][0] > 0).sum() > 500 and (out[2][0] > 0).sum() > 50 and not out[1][0].any() and not out[3][0].any()
        assert 0 < (out[5][0] > 0).sum() and not c.candidates(5)[2].all(), "a close camera: part of the mesh leaves the frame, faces with a vertex outside are skipped whole"
    return Case("one batch of views of three and more sizes", cams, V, F, None, prove, boxes=(-1, ALL_LARGE), batch_bytes=(0, 1), batches=(1, 6))


def render_cases():
    return ([edge_case(), shared_edge_case(2), shared_edge_case(1), twice_case(False), twice_case(True), far_near_case(True), far_near_case(False), dropped_case(),
             limits_case(), whole_image_case(), threshold_case(), tiny_images_case(), normals_case(), batch_case()]
            + [contention_case(k) for k in ("first", "last", "middle")])


RENDER_CASES = render_cases()
RENDER_IDS = [c.name for c in RENDER_CASES]


# ---- visibility --------------------------------------------------------------------------------------------------------------------------------------------
def slanted_plane():
    """Vertices at the integer pixels (3..29) x (3..13) of the exact 33 x 17 camera, z = 2 + (px - 10) / 4: the rendered depth grows by about 0.25 per column."""
    px, py = np.meshgrid(np.arange(3, 30), np.arange(3, 14))
    z = (2.0 + (px - 10) * 0.25).astype(f32)
    V = np.stack([px.astype(f32) * z, py.astype(f32) * z, z], -1).reshape(-1, 3)
    nx, ny = 26, 10
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    F = np.concatenate([np.stack([i, i + nx + 1, i + 1], 1), np.stack([i + nx + 2, i + 1, i + nx + 1], 1)]).astype(np.uint32)
    return V.astype(f32), F


def vis_twin(cams, V, F, th=0.985):
    out = np.zeros((len(V), len(cams)), bool)
    for k, (K, R, C, w, h) in enumerate(cams):
        out[:, k] = views.mesh_visibility(K, R, C, w, h, V, views.project_mesh(K, R, C, w, h, V, F)[0], th)
    return out


def visibility_edges():
    """-> (cams, V, F, expected (n, 1) bool, first special vertex).  The special vertices are isolated: they change no depth."""
    c = cam(33, 17)
    V, F = slanted_plane()
    D = views.project_mesh(*c, V, F)[0]
    th = f32(0.985)
    extra, want = [], []
    # z * 0.985f == depth exactly (strict <: hidden), and the nearest z below it that is visible
    d = D[8, 10]
    z = f32(d / th)
    cand = [z]
    for _ in range(8):
        cand = [np.nextafter(cand[0], f32(0))] + cand + [np.nextafter(cand[-1], f32(9))]
    eq = [v for v in cand if f32(v * th) == d]
    assert eq, "some z has z * 0.985f == the depth exactly"
    lt = max(v for v in cand if f32(v * th) < d)
    extra += [(f32(10) * eq[0], f32(8) * eq[0], eq[0]), (f32(10) * lt, f32(8) * lt, lt)]; want += [False, True]
    # ROUND2INT up and down: z = 2.125 lies in front of column 11's surface and behind column 10's
    zf = f32(2.125)
    assert f32(zf * th) > D[8, 10] and f32(zf * th) < D[8, 11]
    extra += [(f32(22.3125), f32(8) * zf, zf), (np.nextafter(f32(22.3125), f32(0)), f32(8) * zf, zf)]; want += [True, False]
    # the border-1 limits (the surface ends at the border of 3, so the depth there is 0 and neither side is visible: the test cannot decide anything the renderer
    # leaves visible; the cases keep the reads in bounds) and behind the camera
    up = lambda v: np.nextafter(f32(v), f32(99)); dn = lambda v: np.nextafter(f32(v), f32(-99))
    for x, y in ((1, 8), (dn(1), 8), (31, 8), (up(31), 8), (10, 1), (10, dn(1)), (10, 15), (10, up(15)), (-5, 8), (40, 30), (32.4, 16.4)):
        extra.append((f32(x), f32(y), f32(1))); want.append(False)
    extra += [(f32(20), f32(16), f32(-2)), (f32(0), f32(0), f32(0)), (f32(20), f32(16), f32(1e-45))]; want += [False, False, False]
    first = len(V)
    V = np.concatenate([V, np.array(extra, f32)])
    want = np.concatenate([np.ones(first, bool), want])[:, None]                # every surface vertex sees itself: z * 0.985 < z
    pti, zz, ok, front = views.mesh_vertex_records(*c, V)
    px = np.floor(pti[:, 0] + f32(0.5))
    assert px[first + 2] == 11 and px[first + 3] == 10 and pti[first + 2, 0] == f32(10.5), "the two vertices round to different columns"
    assert pti[first + 4, 0] == 1 and pti[first + 5, 0] < 1 and pti[first + 6, 0] == 31 and pti[first + 7, 0] > 31
    return [c], V, F, want, first


def visibility_counts():
    """36 views -- 33 times camera A, twice B, once C -- of patches seen by A, by A and B, by B, by C and by nobody: vertices seen by 33, 35, 2, 1 and 0 views, the
    33 crossing the bitset's word boundary; the first vertex, the last and runs of adjacent ones are removed."""
    def patch(x_world):
        px, py = np.meshgrid(np.arange(0, 5), np.arange(4, 9))
        X = np.stack([x_world + 2.0 * px, 2.0 * py, np.full(px.shape, 2.0)], -1).reshape(-1, 3)
        i = (np.arange(4)[:, None] * 5 + np.arange(4)[None, :]).ravel()
        return X.astype(f32), np.concatenate([np.stack([i, i + 5, i + 1], 1), np.stack([i + 6, i + 1, i + 5], 1)])
    A, B, Cc = cam(33, 17), cam(33, 17, C=(30, 0, 0)), cam(33, 17, C=(200, 0, 0))
    parts = [("none", 1000.0), ("A", 10.0), ("C", 210.0), ("AB", 40.0), ("B", 70.0), ("none", 2000.0)]
    Vs, Fs, tags, n = [], [], [], 0
    for tag, x in parts:
        v, f = patch(x)
        if tag == "none" and not Vs:
            v, f = v[:3], f[:0]                                                 # the first vertices of the mesh: in no face, in no frame
            f = np.zeros((0, 3), np.int64)
        Vs.append(v); Fs.append(f + n); tags += [tag] * len(v); n += len(v)
    V, F = np.concatenate(Vs).astype(f32), np.concatenate(Fs).astype(np.uint32)
    cams = [A] * 16 + [B] + [A] * 17 + [B, Cc]
    want = {"none": 0, "A": 33, "AB": 35, "B": 2, "C": 1}
    return cams, V, F, np.array([want[t] for t in tags])


def literal_swap_remove(keep):
    """The backward loop of SampleMeshWithVisibility over a cList whose RemoveAt moves the last element into the hole, written out."""
    points, kept = list(range(len(keep))), [bool(k) for k in keep]             # pointcloud.points / "pointViews[idx].size() >= 2", removed together (RemovePoint)
    idx = len(points)
    while idx > 0:
        idx -= 1
        if not kept[idx]:
            points[idx] = points[len(points) - 1]; del points[len(points) - 1]
            kept[idx] = kept[len(kept) - 1]; del kept[len(kept) - 1]
    return points


def run_visibility(engine, cams, V, F, want, what):
    K, R, C = (np.array([c[k] for c in cams]) for k in range(3))
    try:
        engine.mesh_set(V, F)
        for bb in (0, 1):                                                       # one batch, and one view per batch (the word is read back and completed)
            engine.mesh_tuning(batch_bytes=bb if bb else DEFAULT_BATCH)
            got = engine.mesh_visibility(K, R, C, [c[3:] for c in cams], len(V))
            assert got.shape == want.shape and np.array_equal(got, want), "%s (batch bytes %d): %d of %d bits differ" % (what, bb, (got != want).sum(), want.size)
    finally:
        engine.mesh_tuning(batch_bytes=DEFAULT_BATCH)
        engine.mesh_release()


def visibility_edges_case(engine):
    cams, V, F, want, first = visibility_edges()
    assert np.array_equal(vis_twin(cams, V, F), want)
    run_visibility(engine, cams, V, F, want, "visibility edges")


def visibility_counts_case(engine):
    cams, V, F, counts = visibility_counts()
    want = vis_twin(cams, V, F)
    assert np.array_equal(want.sum(1), counts) and {0, 1, 2, 33} <= set(counts)
    run_visibility(engine, cams, V, F, want, "visibility counts")
    # other front-depth factors reach the kernel
    try:
        engine.mesh_set(V, F)
        K, R, C = (np.array([c[k] for c in cams]) for k in range(3))
        assert not engine.mesh_visibility(K, R, C, [c[3:] for c in cams], len(V), th_front_depth=1.5).any()
    finally:
        engine.mesh_release()


def interleaved_engines(make):
    """Two engines in one process, their meshes and sizes in turn: nothing of one call survives into the other engine's."""
    a, b = make(), make()
    try:
        ca, cb = RENDER_CASES[0], RENDER_CASES[-4]                              # the edge case (33 x 17) and the batch of mixed sizes
        a.mesh_set(ca.V, ca.F, ca.N); b.mesh_set(cb.V, cb.F, cb.N)
        for _ in range(2):
            for e, c in ((a, ca), (b, cb), (b, cb), (a, ca)):
                K, R, C = (np.array([v[k] for v in c.cams]) for k in range(3))
                for (d, n), (wd, wn) in zip(e.mesh_project(K, R, C, [v[3:] for v in c.cams]), twin(c)):
                    same_bits(d, wd, c.name + ", interleaved"); same_bits(n, wn, c.name + ", interleaved")
    finally:
        a.close(); b.close()


def error_cases(engine, Error):
    """Every refusal of include/pmhip_mesh.h, each followed by a call that succeeds on the same engine."""
    import pytest
    c = RENDER_CASES[0]
    K, R, C, w, h = c.cams[0]
    ok = lambda: same_bits(engine.mesh_project([K], [R], [C], [(w, h)])[0][0], twin(c)[0][0], "after a refusal")
    engine.mesh_release()
    with pytest.raises(Error, match="no mesh"):
        engine.mesh_project([K], [R], [C], [(w, h)])
    with pytest.raises(Error, match="no mesh"):
        engine.mesh_visibility([K], [R], [C], [(w, h)], 3)
    assert engine._lib.pmhip_mesh_get_vertex_normals(engine._h, np.zeros(3, f32)) == -4
    with pytest.raises(Error, match="face 0 names vertex 3 of 3"):
        engine.mesh_set(c.V, [[0, 1, 3]])
    with pytest.raises(Error, match="at least one face"):
        engine.mesh_set(c.V, np.zeros((0, 3), np.uint32))
    engine.mesh_set(c.V, c.F, c.N); ok()
    with pytest.raises(Error, match="names vertex"):
        engine.mesh_set(c.V, [[0, 1, 2], [0, 1, len(c.V)]])
    ok()                                                                        # a refused mesh leaves the one before in place
    for bad in ((0, 5), (5, 0), (-3, 4), (65536, 65536)):
        with pytest.raises(Error, match="view 1 is"):
            engine.mesh_project([K, K], [R, R], [C, C], [(w, h), bad])
        with pytest.raises(Error, match="view 1 is"):
            engine.mesh_visibility([K, K], [R, R], [C, C], [(w, h), bad], len(c.V))
        ok()
    import ctypes
    fp = ctypes.POINTER(ctypes.c_float)
    d = np.zeros((h, w), f32)
    args = (np.ascontiguousarray(np.stack([K, K]).reshape(-1)), np.ascontiguousarray(np.stack([R, R]).reshape(-1)), np.ascontiguousarray(np.stack([C, C]).reshape(-1)),
            np.array([w, h, w, h], np.int32))
    assert engine._lib.pmhip_mesh_project(engine._h, 2, *args, (fp * 2)(d.ctypes.data_as(fp), fp()), None) == -1 and b"view 1 has no depth map" in engine._lib.pmhip_last_error(engine._h)
    assert not d.any(), "nothing was rendered"
    assert engine._lib.pmhip_mesh_project(engine._h, 2, *args, None, None) == -1 and engine._lib.pmhip_mesh_visibility(engine._h, 2, *args, None, 0.985) == -1
    assert engine._lib.pmhip_mesh_project(engine._h, 2, None, args[1], args[2], args[3], (fp * 2)(d.ctypes.data_as(fp), d.ctypes.data_as(fp)), None) == -1
    assert engine.mesh_project(np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2), np.int32)) == []
    ok()
    engine.mesh_release(); engine.mesh_release()


# ---- the routes --------------------------------------------------------------------------------------------------------------------------------------------
def scene_mesh(mvs):
    """A surface for the test scene: its sparse points triangulated in image 0 (views.triangulate_points), faces turned towards that camera."""
    from openmvs_amd import mvsi
    sc = mvsi.load(mvs)
    cams = views.Cameras(sc)
    X = sc.vertices[:600]
    proj, z, vert, faces = views.triangulate_points(cams.K[0], cams.P[0], X, int(cams.size[0][0]), int(cams.size[0][1]))
    a, b, c = (proj[faces[:, k]].astype(np.float64) for k in range(3))
    front = (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1]) - (c[:, 1] - a[:, 1]) * (b[:, 0] - a[:, 0]) > 0
    return np.ascontiguousarray(X, f32), np.where(front[:, None], faces, faces[:, ::-1]).astype(np.uint32)


def mesh_options():
    return views.DenseOptions(nResolutionLevel=2, nMinResolution=80)


def mesh_file_case(engine, mvs, tmp_path):
    """`--mesh-file` on a scene whose images carry no neighbours: the cloud the engine's visibility makes is the twin's, point for point and view for view, so view
    selection ends with the same neighbour lists, depth ranges and seed maps; the engine holds no mesh afterwards; a scene with neighbours ignores the mesh."""
    import os
    from openmvs_amd import densify, meshio, mvsi
    V, F = scene_mesh(mvs)
    ply = os.path.join(str(tmp_path), "surface.ply")
    meshio.save_ply(ply, V, F)
    sc = mvsi.load(mvs)
    assert not any(len(im.view_scores) for im in sc.images)
    sizes = [sc.camera(i)[3:] for i in range(len(sc.images))]
    dev = densify.replace_cloud_by_mesh(mvsi.load(mvs), ply, sizes, engine)
    host = densify.replace_cloud_by_mesh(mvsi.load(mvs), (V, F), sizes)
    assert 50 < len(host.vertices) < len(V), "some vertices are seen by fewer than two images and leave"
    assert np.array_equal(bits(dev.vertices), bits(host.vertices)) and np.array_equal(dev.vertex_view_start, host.vertex_view_start)
    assert np.array_equal(dev.vertex_views["image_id"], host.vertex_views["image_id"])
    assert not np.array_equal(bits(host.vertices), bits(sc.vertices[:len(host.vertices)]))
    with np.testing.assert_raises(Exception):
        engine.mesh_project([np.eye(3)], [np.eye(3)], [np.zeros(3)], [(8, 8)])                       # released
    a = densify.load_scene(mvs, opt=mesh_options(), mesh=ply, mesh_engine=engine)
    b = densify.load_scene(mvs, opt=mesh_options(), mesh=(V, F))
    plain = densify.load_scene(mvs, opt=mesh_options())
    assert a.ids == b.ids and len(a.ids) >= 2
    for i in a.ids:
        assert np.array_equal(a.neighbors[i], b.neighbors[i]) and np.array_equal(a.view_scores[i], b.view_scores[i]) and (a.dmin[i], a.dmax[i]) == (b.dmin[i], b.dmax[i])
        same_bits(a.init_depth[i], b.init_depth[i], "seed depth %d" % i)
    assert any(not np.array_equal(a.view_scores[i]["score"], plain.view_scores[i]["score"]) for i in a.ids if i in plain.ids and len(a.view_scores[i]) == len(plain.view_scores[i])) \
        or a.ids != plain.ids or any(len(a.view_scores[i]) != len(plain.view_scores[i]) for i in a.ids), "the mesh's cloud, not the archive's, was scored"
    # a scene that carries neighbours keeps its cloud
    nbf = os.path.join(str(tmp_path), "neighbours.txt")
    with open(nbf, "w") as f:
        f.write("0 1 2\n1 0 2\n2 1 3\n3 2 1\n")
    c = densify.load_scene(mvs, opt=mesh_options(), view_neighbors_file=nbf, mesh=ply, mesh_engine=engine)
    d = densify.load_scene(mvs, opt=mesh_options(), view_neighbors_file=nbf)
    assert all(np.array_equal(c.neighbors[i], d.neighbors[i]) for i in range(4))


def grid_visibility_case(engine):
    """One 320-pixel visibility run over 5 views of a ~2 000-face displaced grid whose bumps hide parts of it from the oblique cameras."""
    V, F = grid_mesh(32, 31, -1.3, 1.3, -1.0, 1.0, 0.0, 0.35, 9)
    assert len(F) == 1984
    cams = []
    for k in range(5):
        ang = (k - 2) * 0.3
        R = rot(0.05 * k, ang, 0.02 * k)
        C = -R.T @ np.array([0.0, 0.0, 3.2])                                  # the grid's centre at 3.2 in front of every camera
        cams.append(cam(320, 240, 330.0 + k, 159.5, 119.5, R, C))
    want = vis_twin(cams, V, F)
    per_view = want.sum(0)
    assert (per_view > 200).all() and (per_view < len(V)).all() and len(set(want.sum(1))) >= 4, "every camera sees a part of the surface, none all of it"
    run_visibility(engine, cams, V, F, want, "displaced grid at 320 pixels")


def dense_reconstruction_case(engine, mvs, tmp_path, light=False):
    """`densify.dense_reconstruction(mesh_file=...)` up to the depth maps: the views it estimates and their neighbour lists are those the twin's cloud selects, and the
    engine holds no mesh afterwards.  `light` (the emulator): an eighth of the resolution, one level, one sweep -- the estimation is not what the case is about."""
    import os
    from openmvs_amd import densify, meshio, optdense
    V, F = scene_mesh(mvs)
    ply = os.path.join(str(tmp_path), "surface_dr.ply")
    meshio.save_ply(ply, V, F, binary=False)
    opt = optdense.defaults()
    opt.nResolutionLevel = 2; opt.nMinResolution = 80; opt.nNumViews = 2; opt.nEstimateNormals = 2; opt.nEstimationGeometricIters = 0; opt.nOptimize = 0
    if light:
        opt.nResolutionLevel = 3; opt.nMinResolution = 40; opt.nSubResolutionLevels = 0; opt.nEstimationIters = 1
    sv, cloud = densify.dense_reconstruction(engine, mvs, opt=opt, fusion_mode=1, mesh_file=ply)
    host = densify.load_scene(mvs, opt=opt, mesh=(V, F))
    assert cloud is None and sv.ids == host.ids and len(sv.ids) >= 2
    for i in sv.ids:
        assert np.array_equal(sv.neighbors[i], host.neighbors[i]) and np.array_equal(sv.view_scores[i], host.view_scores[i])
        assert (engine.scene_get_maps(i)[0] > 0).mean() > (0.0 if light else 0.2)
    try:
        engine.mesh_project([np.eye(3)], [np.eye(3)], [np.zeros(3)], [(8, 8)])
    except Exception as ex:
        assert "no mesh" in str(ex)
    else:
        raise AssertionError("the mesh is still resident")
