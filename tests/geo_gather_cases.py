"""Cases for the geometric term's depth gather (pm_geo_request / pm_depth_quads_kernel, csrc/pm_kernels.hip; the derivation of the quad copies at the head of every
geometric call, csrc/pm_host_estimate.hip).  pm_sweep2_kernel reads a quad copy of every source depth map -- entry (lx, ly) = the four texels of a bilinear footprint, folded
anti-diagonal-major -- that is derived from the row-major maps, which stay the truth: commits, copies, uploads and raw pointer writes change them.

1. check_quads: the copy itself, on maps of 2x2 .. 130x67 filled with bit patterns a copy through float arithmetic could damage.
2. never_stale: a resident 5-view 96x72 scene with 4 sources per view, pm_sweep2_kernel forced (the reader of the copies); after each of four ways of changing one
   source view's map the next geometric estimate equals the sequential oracle's for the changed inputs, bit for bit.
3. families: the same scene -- its source 1 looks the other way, so a third of the evaluations end early or are redone and drop their gather -- through pm_sweep2
   forced with four lanes per pixel (the quad copy, requested at the head of the trip: <4,1> with the scene's four sources, and <4,2>, the benchmark's instantiation, on
   a 7-view scene of the same kind with six), the two-wide, four-wide and eight-wide kernels and the init pass (part of every call; the row-major map), from planted
   steep normals.

Run on the wave64 emulator by tests/test_emu_geo_gather.py and on the device by tests/test_zz_gpu_geo_gather.py."""
import ctypes as C
import functools
import os
import types

import numpy as np

from openmvs_amd import synth
from openmvs_amd.patchmatch import default_params
from oracle import pyoracle as po
from tests.test_gpu_patchmatch import _same

W, H, SEED, NV = 96, 72, 11, 5
SIZES = [(2, 2), (3, 2), (2, 3), (5, 4), (17, 9), (64, 33), (130, 67)]      # (dw, dh)
FLIP = np.diag([-1.0, 1.0, -1.0])
TUNINGS = {"sweep2-lanes4": dict(wideMaxViews=-1, sweepLanes=4), "sweep2-lanes4-two-views-per-lane": dict(wideMaxViews=-1, sweepLanes=4),
           "sweep2-lanes4-own-size-source": dict(wideMaxViews=-1, sweepLanes=4), "wide2-own-size-source": dict(wideMaxViews=64, wideHyps=2), "wide2": dict(wideMaxViews=64, wideHyps=2), "wide4": dict(wideMaxViews=64, wideHyps=4),
           "wide8-one-view": dict(wideMaxViews=64, wideHyps=8)}
# views of the scene a tuning runs on, where not NV: six sources on four lanes per pixel are pm_sweep2_kernel<4,2> (sweepMapping), the benchmark's instantiation, whose lanes
# request the footprints of two views at the head of a trip; NV's four sources are <4,1>
SCENE_VIEWS = {"sweep2-lanes4-two-views-per-lane": 7}
# one source view with its own size beside scene-sized ones (pmhip_scene_set_view_sized): its image, its camera and its previous-round map are 72 x 54, so its quad copy
# follows scene-sized ones in the call's buffer at an offset of its own and is addressed with its own dw, dh
OWN_SIZE = {"sweep2-lanes4-own-size-source": (72, 54), "wide2-own-size-source": (72, 54)}


def bit_patterns(dw, dh, seed):
    """dw x dh floats by bit pattern: +-0, negatives, denormals, quiet and signalling NaNs with payloads, +-inf, and ordinary values -- every pixel its own pattern."""
    r = np.random.RandomState(seed)
    u = r.randint(0, 1 << 32, size=(dh, dw), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0xBF800000, 0x3F800000], np.uint32)
    flat = u.reshape(-1)
    idx = r.permutation(flat.size)[:min(flat.size, 2 * special.size)]
    flat[idx] = special[np.arange(idx.size) % special.size]
    return u.view(np.float32)


def check_quads(e):
    for n, (dw, dh) in enumerate(SIZES):
        d = bit_patterns(dw, dh, 100 + n)
        q = e.resample(e.RESAMPLE_DEPTH_QUADS, d, (dw, dh), np.full(dw * dh * 4, np.float32(7.0)), (dw, dh)).reshape(dw * dh, 4).view(np.uint32)
        u = d.view(np.uint32)
        assert q.shape == (dw * dh, 4)
        ly, lx = np.mgrid[0:dh, 0:dw]
        at = ((lx + ly) % dw) * dh + ly
        assert np.array_equal(np.sort(at.reshape(-1)), np.arange(dw * dh)), "the folded order is a permutation"
        got = q[at]                                                       # [ly, lx, 4]
        # every entry an inside sample can read (pm_inside1: lx <= dw - 2, ly <= dh - 2): the four row-major values, as bits
        want = np.stack([u[:-1, :-1], u[:-1, 1:], u[1:, :-1], u[1:, 1:]], -1)
        assert np.array_equal(got[:-1, :-1], want), "%dx%d: an entry differs from its four texels" % (dw, dh)
        # last column / row: the texels the map has, 0 for the others
        assert np.array_equal(got[:, -1, 0], u[:, -1]) and np.array_equal(got[-1, :, 0], u[-1, :])
        assert not got[:, -1, 1].any() and not got[:, -1, 3].any() and not got[-1, :, 2].any() and not got[-1, :, 3].any()
        assert np.array_equal(got[:-1, -1, 2], u[1:, -1]) and np.array_equal(got[-1, :-1, 1], u[-1, 1:])


@functools.lru_cache(maxsize=None)
def scene(nv=NV, own=None):
    """nv views (five), every other one a source of each; view 0's first source is turned to look the other way.  own = (w, h): view 0's third source has that size."""
    sc = synth.make_scene(nv, W, H, n_src=nv - 1)
    R = [r.copy() for r in sc.R]
    R[int(sc.neighbors[0][0])] = FLIP @ R[int(sc.neighbors[0][0])]
    sc.R = R
    if own:
        small = synth.make_scene(nv, own[0], own[1], n_src=nv - 1)
        s = int(sc.neighbors[0][2])
        mixed = {name: list(getattr(sc, name)) for name in ("gray", "K", "gt_depth")}
        for name in mixed:
            mixed[name][s] = getattr(small, name)[s]
        sc = types.SimpleNamespace(n_views=nv, width=W, height=H, R=sc.R, C=sc.C, dmin=sc.dmin, dmax=sc.dmax, neighbors=sc.neighbors,
                                   sizes=[own if v == s else (W, H) for v in range(nv)], **mixed)
    return sc


def steep_normals(sc, ref, seed):
    from tests.tap_fallback_cases import _steep_normals
    return _steep_normals(sc, ref, seed)


def _poke(e, ptr, arr):
    """Raw write of a host array to a device pointer of the engine's (the emulated device is host memory)."""
    a = np.ascontiguousarray(arr, np.float32)
    e.sync()
    if os.environ.get("OPENMVS_AMD_TEST_EMULATOR") == "1":
        C.memmove(ptr, a.ctypes.data, a.nbytes)
    else:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0
        assert hip.hipDeviceSynchronize() == 0


def _oracle_geo(sc, start, snaps, cams=None):
    ids = [0] + [int(i) for i in sc.neighbors[0]]
    views, keep = po.make_views(sc.gray, sc.K, sc.R, sc.C, ids, depth_maps={i: snaps[i] for i in ids[1:]}, depth_cams=cams)
    return po.estimate_depth_map(views, len(ids), float(sc.dmin[0]), float(sc.dmax[0]), po.default_opt(seed=SEED, viewID=0, nSubResolutionLevels=0, nEstimationGeometricIters=1),
                                 geo_iter=0, depth=start[0], normal=start[1])


def _geo_round(e, p, start):
    e.scene_set_maps(0, depth=start[0], normal=start[1])
    e.scene_estimate([0], 0, p)
    return e.scene_get_maps(0)


def never_stale(e):
    sc = scene()
    # pm_sweep2_kernel for every launch: it is the reader of the quad copies (a batch this small goes to the speculative kernels otherwise, which read the row-major maps)
    force = TUNINGS["sweep2-lanes4"]
    assert all(e.tuning(**force)[k] == v for k, v in force.items())
    p = default_params(seed=SEED, nSubResolutionLevels=0, nEstimationGeometricIters=1)
    allv = list(range(NV))
    e.Init(False); e.scene_load(sc, n_levels=0)
    e.scene_estimate(allv, -1, p)
    photo = [e.scene_get_maps(v) for v in allv]
    start = (photo[0][0].copy(), photo[0][1].copy())
    snaps = {v: photo[v][0].copy() for v in allv}
    e.scene_commit_round(); e.Init(True)
    seen = []

    def check(what, cams=None):
        got = _geo_round(e, p, start)
        want = _oracle_geo(sc, start, snaps, cams)
        for a, b, name in zip(got, want, ("depth", "normal", "conf")):
            _same(a, b, "%s: geometric %s of view 0" % (what, name))
        assert all((got[0] != s).any() for s in seen), "%s: the estimate is one seen before, the change of the source map did not reach it" % what
        seen.append(got[0].copy())

    check("first round")
    s = int(sc.neighbors[0][1])                    # an ordinary source of view 0
    r = np.random.RandomState(SEED)
    change = lambda d: (d * (1.0 + 0.08 * r.rand(*d.shape))).astype(np.float32)
    # (1) the depth map changes and a round is committed (the snapshot of every view is taken again; view 0's own is not read by view 0)
    new = change(snaps[s])
    e.scene_set_maps(s, depth=new)
    e.scene_commit_round()
    for v in allv[1:]:
        snaps[v] = e.scene_get_maps(v)[0].copy()
    assert np.array_equal(snaps[s], new)
    check("commit_round")
    # (2) a device-to-device copy into the snapshot
    t = int(sc.neighbors[0][2])
    new = change(snaps[s])
    e.scene_set_maps(t, depth=new)                 # (view t's depth array is the device buffer the copy reads; its snapshot stays)
    e.scene_copy(4, s, 1, e.scene_device_ptr(1, t), True)
    snaps[s] = new
    check("scene_copy(what = 4)")
    # (3) a raw write through the snapshot's device pointer
    new = change(snaps[s])
    _poke(e, e.scene_device_ptr(4, s), new)
    snaps[s] = new
    check("write through scene_device_ptr(what = 4)")
    # (4) a map of its own size with its own camera, installed and removed
    dw, dh = 80, 60
    ys, xs = (np.arange(dh) * H // dh), (np.arange(dw) * W // dw)
    own = change(snaps[s][np.ix_(ys, xs)])
    Kd = sc.K[s].copy(); Kd[0] *= dw / W; Kd[1] *= dh / H
    e.scene_set_source_depth(s, own, Kd, sc.R[s], sc.C[s])
    snaps[s] = own
    check("scene_set_source_depth", cams={s: (Kd, sc.R[s], sc.C[s])})
    e.scene_set_source_depth(s, None)
    got = _geo_round(e, p, start)
    assert np.array_equal(got[0].view(np.uint32), seen[-2].view(np.uint32)), "after the installed map's removal the snapshot is read again"


@functools.lru_cache(maxsize=None)
def _families_expected(nv=NV, own=None):
    sc = scene(nv, own)
    start = (sc.gt_depth[0].copy(), steep_normals(sc, 0, SEED))
    snaps = {v: sc.gt_depth[v].copy() for v in range(nv)}
    want = _oracle_geo(sc, start, snaps)
    for a in want:
        a.setflags(write=False)
    return start, snaps, want


def families(e, tuning):
    """One geometric round of view 0 from the ground-truth depth and steep planted normals (0 .. 89.9 degrees off the viewing ray: hypotheses whose patches leave the
    sources), the sources' maps the ground truth; source 1 looks away."""
    nv = SCENE_VIEWS.get(tuning, NV)
    own = OWN_SIZE.get(tuning)
    sc = scene(nv, own)
    start, snaps, want = _families_expected(nv, own)
    got_t = e.tuning(**TUNINGS[tuning])
    assert all(got_t[k] == v for k, v in TUNINGS[tuning].items())
    p = default_params(seed=SEED, nSubResolutionLevels=0, nEstimationGeometricIters=1)
    e.Init(True); e.scene_load(sc, n_levels=0)
    for v in range(1, nv):
        e.scene_set_maps(v, depth=snaps[v])
    e.scene_commit_round()
    got = _geo_round(e, p, start)
    for a, b, name in zip(got, want, ("depth", "normal", "conf")):
        _same(a, b, "%s: geometric %s" % (tuning, name))
    assert (got[0] > 0).mean() > 0.3 and (got[0] != start[0]).any()
