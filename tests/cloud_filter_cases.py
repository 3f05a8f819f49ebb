"""Restatements of Scene::PointCloudFilter (SceneDensify.cpp:2225-2359 in the reference) and PointCloud::RemoveMinViews (PointCloud.cpp:88-93) for the
tests of pmhip_scene_cloud_filter: the vote as the sum over ALL points per cone (one vectorised TConeIntersect::Classify in float32, step by step), the
removal through cloud_cases.crop_reference (the literal RFOREACH + RemoveAt loop), and a maker of clouds with floaters.  Test infrastructure only."""
import numpy as np

from tests import cloud_cases as cc

F = np.float32


def cone_constants(K, widths):
    """angle = float(ComputeFOV(0) / width) with ComputeFOV(0) = 2 atan(width / (2 K00)) in double (Image.cpp:209-213); cosAngleSq in DOUBLE, for the 1 ulp check
    of the float constants the engine reports (the tests classify with the engine's own)."""
    ang = np.array([F(2.0 * np.arctan(float(w) / (2.0 * float(k[0][0]))) / float(w)) for k, w in zip(K, widths)], F)
    return ang, np.cos(ang.astype(np.float64)) ** 2


def _dot3(a0, a1, a2, b0, b1, b2):
    """(a0 b0 + a1 b1) + a2 b2 in float32, every product and sum rounded."""
    return ((a0 * b0).astype(F) + (a1 * b1).astype(F)).astype(F) + (a2 * b2).astype(F)


def classify_cone(pts, O, X, cos_sq):
    """One cone (origin O, through X) against the points `pts` (n, 3) float32: (counted mask, behind mask).  Collector::Init + Classify + IsDepthSimilar."""
    O = np.asarray(O, F); X = np.asarray(X, F); cos_sq = F(cos_sq)
    with np.errstate(all="ignore"):
        D = (X - O).astype(F)
        distance = np.sqrt(_dot3(D[0:1], D[1:2], D[2:3], D[0:1], D[1:2], D[2:3]).astype(F)).astype(F)[0]
        d = (D / distance).astype(F)
        max_h = F(distance * F(1.02))
        E = (pts - O).astype(F)
        t = _dot3(np.broadcast_to(d[0], len(E)), np.broadcast_to(d[1], len(E)), np.broadcast_to(d[2], len(E)), E[:, 0], E[:, 1], E[:, 2]).astype(F)
        e2 = _dot3(E[:, 0], E[:, 1], E[:, 2], E[:, 0], E[:, 1], E[:, 2]).astype(F)
        ok = (np.abs(t) >= F(1e-4)) & (t >= F(0)) & (t <= max_h) & ((t * t).astype(F) > (cos_sq * e2).astype(F))
        similar = (np.abs((distance - t).astype(F)) / distance).astype(F) < F(0.01)
        ok &= ~similar
        return ok, t > distance


def visibility_reference(cloud, cam_C, cos_sq, targets=None):
    """visibility (int32) of PointCloudFilter as the sum over all points per cone.  cam_C (n, 3) double, cos_sq (n,) float32 as the engine used them.
    `targets`: only these point indices are classified (the result has their length)."""
    pts = np.asarray(cloud["points"], F); vs = cloud["viewStart"].astype(np.int64); views = cloud["views"].astype(np.int64)
    nv = (vs[1:] - vs[:-1]).astype(np.int64)
    sel = np.arange(len(pts)) if targets is None else np.asarray(targets, np.int64)
    cand = pts[sel]; cand_nv = nv[sel]
    vis = np.zeros(len(sel), np.int64)
    O = np.asarray(cam_C, np.float64).astype(F)
    for i in range(len(pts)):
        for v in views[vs[i]:vs[i + 1]]:
            ok, behind = classify_cone(cand, O[v], pts[i], cos_sq[v])
            vis += np.where(ok & behind, cand_nv, 0)
            vis -= np.where(ok & ~behind, nv[i], 0)
    return vis.astype(np.int32)


def remove_min_views(cloud, th):
    """PointCloud::RemoveMinViews: RFOREACH(i) if (pointViews[i].size() < th) RemovePoint(i)."""
    vs = cloud["viewStart"].astype(np.int64)
    return cc.crop_reference(cloud, (vs[1:] - vs[:-1]) >= th)


def filter_reference(cloud, cam_C, cos_sq, th_remove=None, min_views=0):
    """(cloud after the filter, visibility or None): RemoveMinViews(min_views) when > 0, then the vote and RFOREACH(i) if (visibility[i] <= th) RemovePoint(i)."""
    if min_views > 0:
        cloud = remove_min_views(cloud, min_views)
    if th_remove is None or cloud["nPoints"] == 0:
        return cloud, None
    vis = visibility_reference(cloud, cam_C, cos_sq)
    return cc.crop_reference(cloud, vis > th_remove), vis


def move_along_first_ray(cloud, cam_C, share, seed, front=True, behind=True):
    """A seeded `share` of the points moved along the ray from the centre of their first view: half to 0.60-0.95 of their distance (floaters in front), half to
    1.011-1.019 (just behind: inside the cone's 2 % reach, outside the 1 % similarity band).  Returns (cloud with new points, indices moved)."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(cloud["points"], F).astype(np.float64)
    n = len(pts)
    idx = np.sort(rng.choice(n, int(round(n * share)), replace=False))
    first = cloud["views"][cloud["viewStart"][:-1].astype(np.int64)][idx].astype(np.int64)
    O = np.asarray(cam_C, np.float64)[first]
    in_front = rng.random(len(idx)) < 0.5 if (front and behind) else np.full(len(idx), bool(front))
    s = np.where(in_front, rng.uniform(0.60, 0.95, len(idx)), rng.uniform(1.011, 1.019, len(idx)))
    pts[idx] = O + (pts[idx] - O) * s[:, None]
    out = dict(cloud); out["points"] = pts.astype(F)
    return out, idx


def with_attributes(cloud, seed):
    """Seeded colours (BGR bytes) and unit normals for a cloud that has none."""
    rng = np.random.default_rng(seed)
    n = int(cloud["nPoints"])
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(cloud, colors=rng.integers(0, 256, (n, 3)).astype(np.uint8), normals=nrm.astype(F))


def classify_cones(O, Xs, p, cos_sq):
    """Many cones of one camera (origin O, through the rows of Xs) against ONE point p: (counted, behind) per cone.  The same float32 steps as classify_cone."""
    O = np.asarray(O, F); Xs = np.asarray(Xs, F).reshape(-1, 3); p = np.asarray(p, F); cos_sq = F(cos_sq)
    with np.errstate(all="ignore"):
        D = (Xs - O).astype(F)
        distance = np.sqrt(_dot3(D[:, 0], D[:, 1], D[:, 2], D[:, 0], D[:, 1], D[:, 2]).astype(F)).astype(F)
        d = (D / distance[:, None]).astype(F)
        max_h = (distance * F(1.02)).astype(F)
        E = (p - O).astype(F)
        n = len(Xs)
        t = _dot3(d[:, 0], d[:, 1], d[:, 2], np.broadcast_to(E[0], n), np.broadcast_to(E[1], n), np.broadcast_to(E[2], n)).astype(F)
        e2 = _dot3(E[0:1], E[1:2], E[2:3], E[0:1], E[1:2], E[2:3]).astype(F)[0]
        ok = (np.abs(t) >= F(1e-4)) & (t >= F(0)) & (t <= max_h) & ((t * t).astype(F) > F(cos_sq * e2))
        similar = (np.abs((distance - t).astype(F)) / distance).astype(F) < F(0.01)
        return ok & ~similar, t > distance


def visibility_sampled(cloud, cam_C, angle, cos_sq, targets, margin=12.0):
    """visibility of the `targets` summed over ALL cones of the cloud, for clouds too large for visibility_reference.  Per camera and target the cones are
    pre-selected in double -- the angle at the camera between the cone's point and the target below `margin` cone angles (at least 10; the float test's own
    rounding widens a cone by far less than one angle plus 2e-3 rad, which is added) -- and the exact float32 test runs on the survivors."""
    assert margin >= 10
    pts = np.asarray(cloud["points"], F); vs = cloud["viewStart"].astype(np.int64); views = cloud["views"].astype(np.int64)
    nv = (vs[1:] - vs[:-1]).astype(np.int64)
    owner = np.repeat(np.arange(len(pts)), nv)
    targets = np.asarray(targets, np.int64)
    vis = np.zeros(len(targets), np.int64)
    X = pts.astype(np.float64)
    for v in np.unique(views):
        ent = owner[views == v]                                      # one entry per (point, view) pair: a view listed twice votes twice
        O = np.asarray(cam_C[v], np.float64).astype(F)
        U = X[ent] - O.astype(np.float64)
        with np.errstate(all="ignore"):
            U /= np.linalg.norm(U, axis=1, keepdims=True)
        lim = np.cos(min(margin * float(angle[v]) + 2e-3, np.pi))
        for k, j in enumerate(targets):
            u = X[j] - O.astype(np.float64)
            nu = np.linalg.norm(u)
            if not nu > 0:
                continue                                             # at the camera centre: t == 0, never counted
            near = ~((U @ (u / nu)) < lim)                           # (a cone without a direction stays in: the exact test drops it)
            i = ent[near]
            ok, behind = classify_cones(O, pts[i], pts[j], cos_sq[v])
            vis[k] += int(nv[j]) * int((ok & behind).sum()) - int(nv[i][ok & ~behind].sum())
    return vis.astype(np.int32)
