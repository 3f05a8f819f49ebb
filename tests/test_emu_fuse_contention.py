"""CPU: the device fusion's per-seed functions (openmvs_amd/csrc/pm_fuse.h) under the host emulation of the GPU scheduler (tests/cpp/fuse_emul.cpp) on the scenes of
tests/fuse_contention_cases.py -- seeds that contend for cells by the dozen and by the thousand, outcomes that depend on the order inside an image, points of 17 views,
thresholds straddled by one ulp, views of their own sizes, values that are not numbers -- against the sequential oracle, under ascending, descending and random thread
orders.  The emulator fails with code 7 when a round makes no progress and with 8 when a reservation outlives its image; either raises here."""
import numpy as np
import pytest

from tests import fuse_cases as fc
from tests import fuse_contention_cases as cc

CASES = cc.all_cases()


@pytest.fixture(scope="module")
def emul():
    return cc.emulator()


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_of_a_contended_scene_is_the_sequential_fuse(emul, name):
    c = CASES[name]
    ref = c.fuse()
    if c.check:
        c.check(c, ref)                                   # the scene is what its name says, by the oracle's result and the inputs alone
    rounds = set()
    for mode in (0, 1, 2):
        got, r, seeds = cc.emulate(emul, c, mode)
        fc.same_cloud(cc.canon(got), cc.canon(ref), "%s, thread order %d" % (name, mode))
        rounds.add(r)
    assert len(rounds) == 1, "the number of rounds depends on which seeds share cells, not on the schedule: %s" % rounds
    r = rounds.pop()
    w, h = c.sizes[0]
    if c.name in ("funnel4", "funnel_occluded", "funnel_occluded3"):
        assert r >= 16                                    # 4 x 4 seeds per cell commit one per round
    if c.name == "funnel64":
        # the seeds of view 0 sit in two or three cells and leave one per cell and round; view 1 adds one round.  (Half of ALL seeds cannot be reached: view 1's seeds are half
        # of them and need a single round, and a 67-pixel row spans more than one 64-pixel cell.)
        assert r >= cc.max_population(c, 0, 1) + 1 and 2 * r >= w * h
    if c.name.startswith("mixed_funnel"):
        assert r >= cc.max_population(c, 2, 1)
    if c.name.startswith("seventeen") and c.kw["nMinViewsFuse"] >= 17:
        assert r >= 17                                    # one image after the other finds its seeds rolled back


@pytest.mark.parametrize("size", (cc.SMALL,) + cc.THIN)
def test_the_two_sides_of_every_threshold_differ(size):
    """|q2 - depthB| / q2 < 0.01, dot > cos 25, max(1 - conf, 0.03) and Round2Int at x.5 on both image borders, one ulp to either side: the oracle must tell them apart (that
    the emulator and the device follow it on each side is the parametrised test's business)."""
    for name, a, b in cc.ties(*size):
        cc.check_tie(name, a, b, a.fuse(), b.fuse())


def test_a_seventeenth_neighbour_is_refused_not_dropped(emul):
    """The oracle, like the reference (tests/test_ref_fuse.py), fuses a view with 17 neighbours into points of 18 views; the engine holds 16 and refuses the view (the device
    test shows that), and the emulator, which used to cut the list, refuses with it."""
    c = cc.eighteen(*cc.SMALL)
    c.check(c, c.fuse())
    with pytest.raises(RuntimeError, match="fuse failed: 9"):
        cc.emulate(emul, c, 0)
