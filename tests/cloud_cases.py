"""Restatements of the last block of Scene::DenseReconstruction (SceneDensify.cpp:1724-1737 in the reference) for the tests of
pmhip_scene_cloud_finish: the crop as a literal RFOREACH + cList::RemoveAt loop, EstimatePointColors with the byte arithmetic of TPixel, and
the PCA normals of EstimatePointNormals over cKDTree neighbour sets.  Test infrastructure only."""
import numpy as np

F = np.float32


def obb_enlarged(rot, pos, ext, border):
    """The ROI of SceneDensify.cpp:1728: EnlargePercent (extents times border) for border > 0, Enlarge(-border) for border < 0."""
    ext = np.asarray(ext, F)
    if border > 0:
        ext = (ext * F(border)).astype(F)
    elif border < 0:
        ext = (ext + F(-border)).astype(F)
    return np.asarray(rot, F), np.asarray(pos, F), ext


def obb_inside(points, rot, pos, ext):
    """TOBB<float,3>::Intersects, float, each row of rot * (p - pos) summed left to right."""
    p = np.asarray(points, F)
    d = [(p[:, a] - F(pos[a])).astype(F) for a in range(3)]
    ok = np.ones(len(p), bool)
    for r in range(3):
        v = ((F(rot[r][0]) * d[0] + F(rot[r][1]) * d[1]).astype(F) + F(rot[r][2]) * d[2]).astype(F)
        ok &= np.abs(v) <= F(ext[r])
    return ok


def crop_reference(cloud, inside):
    """PointCloud::RemovePointsOutside: RFOREACH(i, points) if (!inside) RemovePoint(i) -- RemoveAt moves the current last element into i."""
    P = int(cloud["nPoints"])
    vs = cloud["viewStart"]
    idx = list(range(P))
    for i in range(P - 1, -1, -1):
        if not inside[i]:
            idx[i] = idx[-1]
            idx.pop()
    idx = np.asarray(idx, np.int64)
    out = dict(nPoints=len(idx), points=cloud["points"][idx])
    counts = (vs[1:] - vs[:-1]).astype(np.int64)[idx]
    nvs = np.zeros(len(idx) + 1, np.uint32); nvs[1:] = np.cumsum(counts)
    gather = np.concatenate([np.arange(vs[i], vs[i + 1]) for i in idx]).astype(np.int64) if len(idx) else np.zeros(0, np.int64)
    out["viewStart"] = nvs
    for k in ("views", "weights", "projs"):
        if cloud.get(k) is not None:
            out[k] = cloud[k][gather]
    for k in ("colors", "normals"):
        out[k] = None if cloud.get(k) is None else cloud[k][idx]
    return out


def compose_P(K, R, C):
    """Camera::ComposeP as pm_fuse.h's pmfu_composeP: M = K R summed left to right, P = [M | M (-C)]."""
    K = np.asarray(K, np.float64); R = np.asarray(R, np.float64); C = np.asarray(C, np.float64)
    M = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s = s + K[i, k] * R[k, j]
            M[i, j] = s
    P = np.zeros((3, 4))
    P[:, :3] = M
    for i in range(3):
        P[i, 3] = M[i, 0] * (-C[0]) + M[i, 1] * (-C[1]) + M[i, 2] * (-C[2])
    return P


def _mulu8(a, v):
    """TPixel<uint8_t> * float: (uint8_t)(v * r)."""
    return (v.astype(F) * np.asarray(a, F)).astype(F).astype(np.uint8)


def colors_reference(cloud, Ps, images):
    """EstimatePointColors (DepthMap.cpp:1429-1465): Ps[i] the 3x4 double P of image i, images[i] its (h, w, 3) uint8 BGR or None (skipped)."""
    pts = np.asarray(cloud["points"], F)
    vs = cloud["viewStart"].astype(np.int64); views = cloud["views"].astype(np.int64)
    n = len(pts)
    X = pts.astype(np.float64)
    best = np.full(n, float(np.finfo(F).max)); bi = np.full(n, -1, np.int64)
    cnt = vs[1:] - vs[:-1]
    for j in range(int(cnt.max()) if n else 0):
        has = cnt > j
        v = np.where(has, views[np.minimum(vs[:-1] + j, len(views) - 1)], 0)
        P = np.stack([Ps[i] for i in range(len(Ps))])[v]
        d = ((P[:, 2, 0] * X[:, 0] + P[:, 2, 1] * X[:, 1]) + P[:, 2, 2] * X[:, 2]) + P[:, 2, 3]
        ok = has & np.array([images[i] is not None for i in range(len(images))])[v] & (best > d)
        best = np.where(ok, d, best); bi = np.where(ok, v, bi)
    col = np.full((n, 3), 255, np.uint8)
    for i, img in enumerate(images):
        sel = np.nonzero(bi == i)[0]
        if img is None or not len(sel):
            continue
        P = Ps[i]; x = X[sel]
        q = [(((P[r, 0] * x[:, 0] + P[r, 1] * x[:, 1]) + P[r, 2] * x[:, 2]) + P[r, 3]).astype(F) for r in range(3)]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invZ = (F(1) / q[2]).astype(F)
            px = (q[0] * invZ).astype(F); py = (q[1] * invZ).astype(F)
        h, w = img.shape[:2]
        inside = (q[2] != 0) & (px >= 1) & (py >= 1) & (px <= F(w - 2)) & (py <= F(h - 2))
        sel, px, py = sel[inside], px[inside], py[inside]
        lx = px.astype(np.int64); ly = py.astype(np.int64)
        fx = (px - lx.astype(F)).astype(F); fx1 = (F(1) - fx).astype(F)
        fy = (py - ly.astype(F)).astype(F); fy1 = (F(1) - fy).astype(F)
        for c in range(3):
            a, b = img[ly, lx, c], img[ly, lx + 1, c]
            cc, dd = img[ly + 1, lx, c], img[ly + 1, lx + 1, c]
            top = ((_mulu8(a, fx1).astype(np.int64) + _mulu8(b, fx)) & 255).astype(np.uint8)
            bot = ((_mulu8(cc, fx1).astype(np.int64) + _mulu8(dd, fx)) & 255).astype(np.uint8)
            col[sel, c] = ((_mulu8(top, fy1).astype(np.int64) + _mulu8(bot, fy)) & 255).astype(np.uint8)
    return col


def knn_reference(points, queries, k):
    """cKDTree over the float points promoted to double: (indices (nq, k), distances (nq, k + 1)) -- the (k+1)-th tells where ties make the set ambiguous."""
    from scipy.spatial import cKDTree
    X = np.asarray(points, F).astype(np.float64)
    kk = min(k + 1, len(X))
    d, i = cKDTree(X).query(X[queries], k=kk)
    d = np.asarray(d).reshape(len(queries), kk); i = np.asarray(i).reshape(len(queries), kk)
    return i[:, :k], d


def knn_tie_order(points, queries, idx):
    """Re-sort each neighbour list by (double squared distance, index): the tie rule of the device."""
    X = np.asarray(points, F).astype(np.float64)
    out = np.empty_like(idx)
    for r, q in enumerate(queries):
        dx = X[idx[r]] - X[q]
        d = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
        out[r] = idx[r][np.lexsort((idx[r], d))]
    return out


def pca_normals(points, nbrs, c_first):
    """The plane fit of linear_least_squares_fitting_3 over each neighbour set (np.linalg.eigh, double), cast to float and oriented like
    EstimatePointNormals: flipped where normal.dot(Cast<float>(C) - point) < 0 in float.  Returns (normals, eigenvalues ascending)."""
    X = np.asarray(points, F).astype(np.float64)
    nb = X[nbrs]                                             # (q, k, 3)
    c = nb.mean(axis=1)
    d = nb - c[:, None, :]
    cov = np.einsum("qki,qkj->qij", d, d)
    lam, vec = np.linalg.eigh(cov)
    n = vec[:, :, 0].astype(F)
    return n, lam


def orient(normals, points, c_first):
    n = np.asarray(normals, F).copy(); p = np.asarray(points, F); cf = np.asarray(c_first, F)
    d = (cf - p).astype(F)
    dot = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]).astype(F) + n[:, 2] * d[:, 2]).astype(F)
    n[dot < 0] *= -1
    return n, dot


def random_cloud(sc, n, seed=0, max_views=4, jitter=0.0):
    """Points on the synthetic scene's surface: random pixels of random views back-projected with the ground-truth depth (float32), each
    with 1..max_views ascending views that contain its projection's image (the first the one it came from)."""
    rng = np.random.default_rng(seed)
    V = len(sc.K)
    src = rng.integers(0, V, n)
    H, W = sc.gt_depth.shape[1:]
    x = rng.uniform(0, W - 1, n); y = rng.uniform(0, H - 1, n)
    z = sc.gt_depth[src, y.astype(int), x.astype(int)].astype(np.float64)
    ok = z > 0
    src, x, y, z = src[ok], x[ok], y[ok], z[ok]
    Kinv = np.linalg.inv(sc.K[src])
    ray = np.einsum("nij,nj->ni", Kinv, np.stack([x, y, np.ones_like(x)], 1))
    Xc = ray * z[:, None]
    Xw = np.einsum("nji,nj->ni", sc.R[src], Xc) + sc.C[src]
    Xw = Xw + rng.normal(0, jitter, Xw.shape) if jitter else Xw
    pts = Xw.astype(F)
    vs = [0]; views = []
    for i in range(len(pts)):
        k = int(rng.integers(1, max_views + 1))
        others = [v for v in rng.permutation(V)[:k] if v != src[i]]
        lst = sorted(set([int(src[i])] + [int(v) for v in others]))
        views += lst; vs.append(len(views))
    w = rng.uniform(0.1, 2, len(views)).astype(F)
    return dict(nPoints=len(pts), points=pts, viewStart=np.asarray(vs, np.uint32), views=np.asarray(views, np.uint32), weights=w)


def angle(a, b):
    """Angle in radians between the rows of a and b (atan2 of |a x b| and a.b: exact near 0, unlike arccos of a float dot product)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum("ij,ij->i", a, b))
