"""-m gpu: the tSGM steps around Match on the device (csrc/sgm_post.hip and the scan of csrc/sgm_tsgm.hip through the C ABI) on the hand-built maps of
tests/sgm_post_edge_cases.py, against the sequential oracle: every element, bit for bit, twice on one engine.  The one exception is a NaN result (0 * inf where a projection
hits a pixel centre, NaN inputs): its position must coincide, its sign and payload are not compared.  Every case first proves on the oracle's result that it reaches the edge
it is named after.

This file is the judge of the float -> int conversions: the emulator converts as x86 does, the device saturates and turns NaN into 0 unless sgmp_f2i (sgm_post.h) decides
first.  It is also the only place where the scan that builds the 2x pixel table in the resident loop runs with more than 256 tiles, i.e. with its carry."""
import time

import numpy as np
import pytest

from openmvs_amd import sgm, tsgm
from oracle import pyoracle as po
from tests import sgm_cases as sc
from tests import sgm_post_edge_cases as ec
from tests.test_emu_sgm_post_edges import refine_on_the_resident_problem
from tests.tsgm_backends import OracleBackend

pytestmark = pytest.mark.gpu

SIZES = (ec.SMALL,) + ec.THIN + (ec.LARGE,)
ids = lambda s: "%dx%d" % s if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


@pytest.mark.parametrize("size", SIZES, ids=ids)
@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_device_steps_on_hand_built_maps(matcher, family, size):
    t = time.time()
    n = ec.check_family(matcher, family, size)
    print("\n%s %dx%d: %d comparisons, %.2f s with the oracle and the predicates" % (family, size[0], size[1], n, time.time() - t))
    assert n > 0


def test_device_limits(matcher):
    """65534 columns flip, 65535 are refused (the column key has 16 bits); 32 pairs fuse, 33 are refused."""
    c = ec.flip_widest()
    want = ec.run(c, ec.ORACLE); c.check(want)
    for _ in range(2):
        ec.same(ec.run(c, matcher), want, c.name)
    with pytest.raises(sgm.SGMError):
        matcher.FlipDirection(np.zeros((1, 65535), np.int16))
    deps, rgs, cfs, _ = ec.fusion_cases(5, 3, 33)[0].args
    with pytest.raises(sgm.SGMError):
        matcher.FusePairs(deps, rgs, cfs, 1)


@pytest.mark.parametrize("size", (ec.SMALL, ec.LARGE), ids=ids)
def test_device_refine_on_a_resident_problem(matcher, size):
    assert refine_on_the_resident_problem(matcher, size) > 0


# The CPU oracle's loop at this size, measured on one core: 10.5 s (518 x 518) and 10.1 s (520 x 518) when the first level searches the default range of 66 disparities
# (the literal O(D^2) recurrence), 1.7 s when an initial disparity map narrows it to 11 -- so the case hands one over; its holes keep patches of the 33-wide ranges.
@pytest.mark.parametrize("w,h,tiles", [(518, 518, 256), (520, 518, 257)])
def test_resident_loop_scan_with_and_without_the_carry(matcher, w, h, tiles):
    """sgmhip_tsgm_match against openmvs_amd/tsgm.py on the oracle: two levels, the finest with a valid grid of 512 x 512 (exactly 256 tiles of 1024 pixels: one chunk of the
    tile scan, no carry) and of 514 x 512 (257 tiles: the second chunk starts from the carry).  Besides the final maps, the cost volume and the 8-path sums of the last
    left Match are compared: they are laid out by the pixel table's idx, so every idx the scan produced is checked, not only through the disparities that survive."""
    d0 = 9
    lb, lg, rg = sc.stereo_pair(w, h, d0, seed=6)
    rb = np.roll(lb, d0, axis=1)
    mask = np.full((h, w), 255, np.uint8); mask[:, :7] = 0; mask[h // 3:h // 3 + 40, w // 2:w // 2 + 90] = 0
    assert tsgm.compute_scale(w, h, 200) == 1
    init = np.full((int(np.rint((h >> 1) * 0.5)) - 6, int(np.rint((w >> 1) * 0.5)) - 6), d0 >> 2, np.int16); init[::7, ::5] = tsgm.NO_DISP; init[40:60, 30:80] = tsgm.NO_DISP
    n2 = (w - 6) * (h - 6)
    assert (n2 + 1023) // 1024 == tiles and (tiles > 256) == (w == 520)                    # the predicate: more than 256 tiles on the ragged level
    ob = OracleBackend()
    t = time.time()
    ref = tsgm.tsgm_match(ob, lb, lg, rb, rg, mask, mask, min_resolution=200, init_left_disparity=init)
    t_ref = time.time() - t
    px, n = ob._prob[3], ob._prob[4]
    assert px.size == n2 and len(set(np.diff(px["idx"].astype(np.int64)).tolist())) >= 2     # ragged: the running index is no multiple of the pixel index
    for k in range(2):
        t = time.time()
        dev = matcher.tsgm_match(lb, rb, lg, rg, mask, mask, min_resolution=200, init_left_disparity=init)
        t_dev = time.time() - t
        assert dev[2] == ref[2] == 2
        assert np.array_equal(dev[0], ref[0]) and np.array_equal(dev[1], ref[1])
        matcher._num = n                                                                    # the size of the resident volume: the oracle's, checked by the sums below
        _, _, costs, acc = matcher.results(volumes=True)
        assert np.array_equal(costs, ob._costs), "cost volume: %d of %d entries differ" % (int((costs != ob._costs).sum()), n)
        assert np.array_equal(acc, ob._acc), "8-path sums: %d of %d entries differ" % (int((acc != ob._acc).sum()), n)
    print("\n%dx%d: %d tiles, %d costs; oracle loop %.2f s, device call %.3f s" % (w, h, tiles, n, t_ref, t_dev))
    assert (dev[0] != tsgm.NO_DISP).mean() > 0.5
