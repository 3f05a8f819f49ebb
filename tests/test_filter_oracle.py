"""CPU known-answer tests of the FilterDepthMap oracle (SceneDensify.cpp:1050-1299)."""
import numpy as np
import pytest

from oracle import pyoracle as po


@pytest.fixture(scope="module")
def gt_scene():
    from openmvs_amd import synth
    sc = synth.make_scene(5, 96, 64, n_src=4)
    depth = sc.gt_depth.copy()
    depth[:, :4] = 0; depth[:, -4:] = 0; depth[:, :, :4] = 0; depth[:, :, -4:] = 0     # estimated maps have an empty 4-px border
    conf = np.where(depth > 0, np.float32(0.8), np.float32(0)).astype(np.float32)
    return sc, depth, conf


@pytest.mark.parametrize("adjust", [True, False])
def test_consistent_depth_maps_survive(gt_scene, adjust):
    sc, depth, conf = gt_scene
    rc, nd, nc = po.filter_depth_map(depth, conf, sc.K, sc.R, sc.C, 0, list(sc.neighbors[0]), sc.dmin[0], sc.dmax[0], bAdjust=adjust)
    assert rc == 0
    m = depth[0] > 0
    kept = (nd > 0) & m
    assert kept.sum() > 0.6 * m.sum() and (nd[~m] == 0).all()
    assert np.abs(nd[kept] - depth[0][kept]).max() / depth[0][kept].mean() < 6e-3   # averaged with splatted neighbour depths (thDepthDiff 1.2 %)
    if adjust:
        assert (nc[kept] >= np.float32(0.8)).all()          # own confidence + agreeing neighbours - violations > own
    else:
        assert (nc[kept] == np.float32(0.8)).all() and np.array_equal(nd[kept], depth[0][kept])


def test_outliers_are_removed_and_too_few_neighbours_is_refused(gt_scene):
    sc, depth, conf = gt_scene
    d = depth.copy()
    d[0, 20:30, 30:50] *= 1.5                                # a block of wrong depths in the reference view
    rc, nd, nc = po.filter_depth_map(d, conf, sc.K, sc.R, sc.C, 0, list(sc.neighbors[0]), sc.dmin[0], sc.dmax[0] * 2)
    assert rc == 0 and (nd[20:30, 30:50] == 0).mean() > 0.9
    rc, _, _ = po.filter_depth_map(d, conf, sc.K, sc.R, sc.C, 0, [1], sc.dmin[0], sc.dmax[0])   # N = 1 < nMinViewsFilter = 2 (:1060)
    assert rc == 1


def test_gap_interpolation_fills_small_similar_gaps_only():
    h, w = 12, 30
    depth = np.full((h, w), 2.0, np.float32); conf = np.full((h, w), 0.5, np.float32)
    normal = np.zeros((h, w, 3), np.float32); normal[..., 2] = -1
    depth[3, 5:9] = 0            # 4-px row gap between equal depths -> filled
    depth[5, 10:18] = 0          # 8-px gap > nIpolGapSize -> untouched
    depth[7, 0:3] = 0            # touches the row start -> row pass leaves it; the column pass fills it (1-px column gaps)
    depth[9, 20:23] = 0; depth[9, 23:] = 2.2   # ends differ by 10 % > 2.5 % -> row pass leaves it; column pass fills it
    conf[3, 4] = 0.3
    d, n, c = po.gap_interpolation(depth, normal, conf)
    assert np.allclose(d[3, 5:9], 2.0) and np.allclose(c[3, 5:9], 0.3) and np.allclose(n[3, 5:9], [0, 0, -1], atol=1e-6)
    assert (d[5, 10:18] == 2.0).all()      # the column pass closes 1-row gaps whatever their width
    assert (d[7, 0:3] == 2.0).all() and (d[9, 20:23] == 2.0).all()
    depth2 = depth.copy(); depth2[4:7, 10:18] = 0   # now 3 rows missing: columns fill it (3 <= 7)
    d2, _, _ = po.gap_interpolation(depth2, normal, conf)
    assert (d2[4:7, 10:18] == 2.0).all()
    depth3 = np.full((20, 30), 2.0, np.float32); depth3[4:14, 10:20] = 0   # 10x10 hole: too large both ways
    d3, _, _ = po.gap_interpolation(depth3, np.broadcast_to(normal[0, 0], (20, 30, 3)).copy(), np.full((20, 30), 0.5, np.float32))
    assert (d3[4:14, 10:20] == 0).all()
    ramp = np.full((4, 12), 2.0, np.float32); ramp[1, 3:6] = 0; ramp[1, 6:] = 2.04     # 2 % step: interpolated linearly
    dr, _, _ = po.gap_interpolation(ramp, np.broadcast_to(normal[0, 0], (4, 12, 3)).copy(), np.full((4, 12), 0.5, np.float32))
    assert np.allclose(dr[1, 3:6], [2.01, 2.02, 2.03], atol=1e-6)


def _reformulated_remove_small_segments(depth, speckle, th):
    """Pure-python model of the GPU formulation (pm_filter.hip): union-find over MUTUAL edges with root = smallest
    column-major index, then a replay of the seed order on the quotient graph of asymmetric edges."""
    h, w = depth.shape
    cm = lambda x, y: x * h + y
    parent = list(range(w * h))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a
    sim = lambda a, b: abs(np.float32(a) - np.float32(b)) / np.float32(a) < np.float32(th)
    for y in range(h):
        for x in range(w):
            d = depth[y, x]
            if not d > 0: continue
            for qx, qy in ((x + 1, y), (x, y + 1)):
                if qx < w and qy < h and depth[qy, qx] > 0 and sim(d, depth[qy, qx]) and sim(depth[qy, qx], d):
                    a, b = find(cm(x, y)), find(cm(qx, qy))
                    if a != b: parent[max(a, b)] = min(a, b)
    root = np.array([[find(cm(x, y)) for x in range(w)] for y in range(h)])
    size = np.bincount(root.ravel(), minlength=w * h)
    adj = {}
    for y in range(h):
        for x in range(w):
            d = depth[y, x]
            if not d > 0: continue
            for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if 0 <= qx < w and 0 <= qy < h and depth[qy, qx] > 0 and sim(d, depth[qy, qx]) and not sim(depth[qy, qx], d) and root[y, x] != root[qy, qx]:
                    adj.setdefault(root[y, x], set()).add(root[qy, qx]); adj.setdefault(root[qy, qx], set())
    decided = {}
    done = set()
    for r in sorted(adj):
        if r in done: continue
        seg = [r]; done.add(r); q = 0
        while q < len(seg):
            for nb in sorted(adj[seg[q]]):
                if nb not in done: done.add(nb); seg.append(nb)
            q += 1
        rm = sum(size[s] for s in seg) < speckle
        for s in seg: decided[s] = rm
    remove = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            r = root[y, x]
            remove[y, x] = decided[r] if r in decided else size[r] < speckle
    return remove


def test_remove_small_segments_reformulation_equals_the_sequential_region_growing():
    r = np.random.RandomState(11)
    th = np.float32(0.01) * np.float32(0.7)
    n_asym_cases = 0
    for trial in range(60):
        h, w = r.randint(8, 22), r.randint(8, 22)
        # piecewise-constant levels spaced right at the similarity threshold so that one-directional edges are common
        levels = 2.0 * (1 + float(th)) ** (r.randint(0, 5, (h, w)) * r.choice([0.97, 1.0, 1.03]))
        depth = levels.astype(np.float32)
        depth[r.rand(h, w) < 0.15] = 0
        normal = np.zeros((h, w, 3), np.float32); normal[..., 2] = -1; conf = np.full((h, w), 0.5, np.float32)
        speckle = int(r.choice([3, 6, 12, 30]))
        od, on, oc = po.remove_small_segments(depth, normal, conf, nSpeckleSize=speckle)
        rm = _reformulated_remove_small_segments(depth, speckle, th)
        want = (depth > 0) & (od == 0)
        assert np.array_equal(rm & (depth > 0), want), f"trial {trial}"
        assert (on[od == 0] == 0).all() and (oc[od == 0] == 0).all()
        a = depth[:, :-1]; b = depth[:, 1:]
        with np.errstate(divide="ignore", invalid="ignore"):
            n_asym_cases += int((((np.abs(a - b) / a < th) != (np.abs(a - b) / b < th)) & (a > 0) & (b > 0)).sum())
    assert n_asym_cases > 50          # the test really exercises one-directional edges
    # the ramps of tests/post_filter_cases.py: every neighbouring pair one-directional (a quotient graph of 2wh - w - h edges over n singletons), and
    # columns linked by one-directional edges (segment sizes are sums over the replay); 13 x 9, so a column has 9 pixels and a pair of columns 18
    from tests import post_filter_cases as cases
    w, h = 13, 9
    ramps = [m for m in cases.segment_maps(w, h, 0.01) if "ramp" in m[0] or "xpairs" in m[0]]
    assert [m[0] for m in ramps] == ["ramp_rising", "ramp_falling", "xramp_rising", "xramp_falling", "xpairs_down", "xpairs_up"]
    for name, depth, claim in ramps:
        share = cases.asymmetric_share(depth, th)
        assert (share == 1.0) if name.startswith("ramp") else (0 < share < 1), (name, share)
        normal = np.zeros((h, w, 3), np.float32); normal[..., 2] = -1; conf = np.full((h, w), 0.5, np.float32)
        for speckle in (0, 1, 2, 9, 10, 18, 19, 117, 118):
            od, on, oc = po.remove_small_segments(depth, normal, conf, nSpeckleSize=speckle)
            assert int((od > 0).sum()) == claim(speckle), (name, speckle)
            assert np.array_equal(_reformulated_remove_small_segments(depth, speckle, th), od == 0), (name, speckle)


def test_remove_small_segments_basic():
    depth = np.zeros((30, 40), np.float32); depth[2:20, 2:30] = 2.0        # 504-px segment: kept
    depth[24:27, 5:9] = 2.0                                                # 12-px island: removed
    depth[22:28, 20:36] = 3.0                                              # 96-px island: removed (< 100)
    normal = np.zeros((30, 40, 3), np.float32); normal[..., 2] = -1; conf = np.full((30, 40), 0.5, np.float32)
    d, n, c = po.remove_small_segments(depth, normal, conf)
    assert (d[2:20, 2:30] == 2.0).all() and (d[24:27, 5:9] == 0).all() and (d[22:28, 20:36] == 0).all()
    assert (n[24:27, 5:9] == 0).all() and (c[22:28, 20:36] == 0).all()


def test_filter_golden_fixture_pins_the_post_filter_oracles():
    import os
    G = os.path.join(os.path.dirname(__file__), "golden")
    g = np.load(os.path.join(G, "pm_golden_96x64.npz")); f = np.load(os.path.join(G, "filter_golden_96x64.npz"))
    nv = int(g["n_views"]); depth = g["depth_photo_all"]
    for v in range(nv):
        sd, sn, sc_ = po.remove_small_segments(depth[v], f["normal"][v], f["conf"][v], nSpeckleSize=30)
        assert np.array_equal(sd, f["speckle_depth"][v])
        gd, gn, gc = po.gap_interpolation(sd, sn, sc_)
        assert np.array_equal(gd, f["gap_depth"][v]) and np.array_equal(gn, f["gap_normal"][v]) and np.array_equal(gc, f["gap_conf"][v])
    for v in range(nv):
        rc, fd, fc = po.filter_depth_map(f["gap_depth"], f["gap_conf"], g["K"], g["R"], g["C"], v, list(g["neighbors"][v]), g["dmin"][v], g["dmax"][v])
        assert rc == 0 and np.array_equal(fd, f["filt_depth"][v]) and np.array_equal(fc, f["filt_conf"][v])
        rc, sd, sc_ = po.filter_depth_map(f["gap_depth"], f["gap_conf"], g["K"], g["R"], g["C"], v, list(g["neighbors"][v]), g["dmin"][v], g["dmax"][v], bAdjust=False)
        assert np.array_equal(sd, f["strict_depth"][v]) and np.array_equal(sc_, f["strict_conf"][v])
