"""-m gpu: FuseDepthMaps on the device (csrc/pm_fuse.hip) on the scenes of tests/fuse_contention_cases.py, against the sequential oracle and exactly.  A second call on the same
engine must give the same cloud (a reservation or a claim left behind would show), and the number of rounds must be the host emulation's: it depends only on which seeds share
cells, so a difference means that the device reserves a cell the host does not, or the reverse.  The compaction kernels (tile sums, scan, scatter) run on the device only: the
compaction_* and seventeen_*_full scenes put kept points on the first and the last pixel, on both sides of a tile border, nowhere, and everywhere with 17 views each."""
import time

import numpy as np
import pytest

from openmvs_amd.patchmatch import PatchMatchHIP
from tests import fuse_cases as fc
from tests import fuse_contention_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.all_cases((cc.SMALL,) + cc.THIN + (cc.LARGE,))


@pytest.fixture(scope="module")
def emul():
    return cc.emulator()


@pytest.fixture(scope="module")
def engine():
    e = PatchMatchHIP(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_fuse_of_a_contended_scene(engine, emul, name):
    c = CASES[name]
    ref = c.fuse()
    if c.check:
        c.check(c, ref)
    _, rounds, _ = cc.emulate(emul, c, 0)
    c.load(engine)
    t = time.time()
    got = engine.scene_fuse(c.order, **c.kw)
    dt = time.time() - t
    print("\n%s: %d points from %d depths in %d rounds, %.1f ms on the device" % (name, got["nPoints"], got["nDepths"], got["rounds"], dt * 1e3))
    fc.same_cloud(cc.canon(got), cc.canon(ref), name)
    assert got["rounds"] == rounds, "%s: %d rounds on the device, %d in the emulator" % (name, got["rounds"], rounds)
    again = engine.scene_fuse(c.order, **c.kw)
    fc.same_cloud(cc.canon(again), cc.canon(ref), name + ", second call")
    assert again["rounds"] == rounds
    d0, _, _ = engine.scene_get_maps(0)
    assert np.array_equal(d0.view(np.uint32), c.deps[0].view(np.uint32))          # fusion zeroes its own copies


def test_a_seventeenth_neighbour_is_refused(engine):
    """The reference fuses any number of neighbours; the engine holds 16 per view and says so when the view is set instead of dropping the rest."""
    c = cc.eighteen(*cc.SMALL)
    with pytest.raises(Exception):
        c.load(engine)
