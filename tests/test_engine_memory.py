"""Device memory of the two engines under the wave64 emulator, whose header counts the live allocations (hipemu_live_allocs) and can make the k-th hipMalloc
fail (hipemu_fail_malloc_at): the whole chain leaves nothing behind after pmhip_destroy / sgmhip_destroy, pmhip_release followed by a larger scene leaks nothing,
and a call whose k-th allocation fails returns PMHIP_E_HIP, keeps nothing it does not own for later, and succeeds when repeated."""
import ctypes as C

import numpy as np
import pytest

from openmvs_amd import patchmatch, sgm, synth
from tests import cloud_cases as cc
from tests import emu
from tests import engine_chain_cases as ec
from tests import fuse_cases as fc
from tests import sgm_cases

PMHIP_E_HIP = -3


@pytest.fixture(scope="module")
def lib():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield patchmatch.load_library()


def _live(lib):
    out = (C.c_uint64 * 2)()
    lib.hipemu_live_allocs(out)
    return int(out[0]), int(out[1])


def _fail_at(lib, k):
    lib.hipemu_fail_malloc_at(C.c_int64(k))


# ---- (i), (ii): nothing is left behind --------------------------------------------------------------------------------------------------------
def test_whole_chain_then_destroy_leaves_no_allocation(lib):
    start = _live(lib)
    e = patchmatch.PatchMatchHIP(0)
    ec.run_chain(e, ec.make_case(4, 64, 48))
    assert _live(lib)[0] > start[0]
    e.close()
    assert _live(lib) == start


def test_release_then_a_larger_scene_leaks_nothing(lib):
    start = _live(lib)
    e = patchmatch.PatchMatchHIP(0)
    ec.run_chain(e, ec.make_case(4, 64, 48))
    e.Release()
    assert _live(lib) == start                                           # (pmhip_create itself allocates nothing on the device)
    ec.run_chain(e, ec.make_case(5, 96, 80, own=(2, 80, 64)))
    e.Release()
    assert _live(lib) == start
    e.close()
    assert _live(lib) == start


def test_sgm_match_then_destroy_leaves_no_allocation():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        lib = sgm.load_library()
        start = _live(lib)
        m = sgm.SemiGlobalMatcherHIP(0)
        lb, lg, rg = sgm_cases.stereo_pair(96, 64, 5, seed=3)
        px, n, mx = sgm_cases.ranges(96, 64, "uniform", -8, 56, seed=4)
        m.set_problem(lb, lg, rg, px, n, mx)
        m.Match()
        m.results()
        assert _live(lib)[0] > start[0]
        m.close()
        assert _live(lib) == start


# ---- (iii): a failing allocation ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return synth.make_scene(5, 96, 72, n_src=4)


def _engine_with_maps(sc):
    e = patchmatch.PatchMatchHIP(0)
    e.scene_load(sc, n_levels=0)
    d, n, c = fc.make_maps(sc, seed=5)
    for v in range(sc.n_views):
        e.scene_set_maps(v, d[v], n[v]); e.scene_set_conf(v, c[v])
    return e


def _maps(e, sc):
    return {"%d.%d" % (v, j): a for v in range(sc.n_views) for j, a in enumerate(e.scene_get_maps(v))}


def _cloud(sc):
    cl = cc.random_cloud(sc, 3000, seed=6)
    rng = np.random.default_rng(7)
    cl["colors"] = rng.integers(0, 256, (cl["nPoints"], 3)).astype(np.uint8)
    cl["normals"] = rng.normal(size=(cl["nPoints"], 3)).astype(np.float32)
    return cl


def _cases(sc):
    ids = list(range(sc.n_views))
    cl = _cloud(sc)
    load = lambda e: e.scene_cloud_load(cl["points"], cl["viewStart"], cl["views"], cl["weights"], cl["colors"], cl["normals"])
    get = lambda e, sc: {k: v for k, v in e.scene_cloud_get().items() if k != "nPoints"}
    # name -> (the call, its results, the allocations it makes)
    return {"gap_interpolation": (lambda e: e.scene_gap_interpolation(ids), _maps, 2),
            "remove_small_segments": (lambda e: e.scene_remove_small_segments(ids, nSpeckleSize=30), _maps, 5),
            "cloud_load": (load, get, 7)}


@pytest.mark.parametrize("name", ["gap_interpolation", "remove_small_segments", "cloud_load"])
def test_failing_allocation_is_an_error_that_leaks_nothing(lib, scene, name):
    sc = scene
    call, results, n_allocs = _cases(sc)[name]
    start = _live(lib)
    e = _engine_with_maps(sc)
    before = _live(lib)
    call(e)
    kept = _live(lib)[1] - before[1]                                     # what a successful call keeps: the resident cloud (grow-only), nothing for the two filters
    assert kept == 0 or name == "cloud_load"
    want = results(e, sc)
    e.close()
    assert _live(lib) == start
    k = 0
    while True:                                                           # every k from 1 to the number of allocations the call makes, each on an undisturbed engine
        k += 1
        e = _engine_with_maps(sc)
        before = _live(lib)
        _fail_at(lib, k)
        try:
            call(e)
            failed = False
        except patchmatch.PatchMatchError as ex:
            failed = True
            assert ("pmhip error %d:" % PMHIP_E_HIP) in str(ex), str(ex)
        finally:
            _fail_at(lib, -1)
        if failed:
            after = _live(lib)
            # nothing above what was there, but for the grow-only buffers of the cloud that a later allocation's failure leaves in place (and then less than all of them)
            assert after[1] <= before[1] or (name == "cloud_load" and k > 5 and after[1] < before[1] + kept), (k, before, after)
            call(e)                                                       # the same call then succeeds ...
        ec.same(results(e, sc), want, "%s, allocation %d failed" % (name, k))   # ... with an undisturbed engine's results
        e.close()
        assert _live(lib) == start, k
        if not failed:
            break
    assert k - 1 == n_allocs
