"""-m gpu, collected last: the three depth-map post-filters (csrc/pm_filter.hip) and the SGM speckle filter (csrc/sgm_post.hip) on adversarial maps, against the
sequential oracle, bit for bit.  The cases are shared with the emulator suite (tests/post_filter_cases.py, tests/test_emu_post_filter_edges.py), which runs its
fibers in a fixed order: contention on a union-find root, on a splat key or on the edge counter exists only here.  67 x 37 and the narrowest sizes as there, and
331 x 211 (about 1090 waves in 273 blocks) only here -- but for the two full ramps of the segment filter, which run at 131 x 77: their host replay of
139 000 edges takes half a second a call at the large size.  Every case runs once."""
import pytest

from openmvs_amd import patchmatch, sgm
from tests import post_filter_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = patchmatch.PatchMatchHIP(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


def test_remove_small_segments_on_adversarial_maps(engine):
    calls = len(cases.SPECKLE_SIZES) * len(cases.SEGMENT_THRESHOLDS)
    for size in (cases.SMALL,) + cases.THIN:
        assert cases.segments_equal_the_oracle(engine, size) >= 11 * calls
    names = [m[0] for m in cases.segment_maps(*cases.LARGE, 0.01)]
    assert cases.segments_equal_the_oracle(engine, cases.LARGE, maps=[n for n in names if n not in cases.FULL_RAMPS]) == (len(names) - 2) * calls == 10 * calls
    assert cases.segments_equal_the_oracle(engine, cases.MEDIUM, maps=cases.FULL_RAMPS) == 2 * calls          # (see post_filter_cases.MEDIUM)


def test_gap_interpolation_on_adversarial_maps(engine):
    for size in (cases.SMALL,) + cases.THIN:
        assert cases.gaps_equal_the_oracle(engine, size) == 30 * len(cases.GAP_SIZES) * len(cases.GAP_THRESHOLDS)
    assert cases.gaps_equal_the_oracle(engine, cases.LARGE, n_maps=10) == 10 * len(cases.GAP_SIZES) * len(cases.GAP_THRESHOLDS)


def test_filter_depth_map_on_tied_splats(engine):
    for size in (cases.SMALL,) + cases.THIN_SCENE + (cases.LARGE,):
        assert cases.filter_equals_the_oracle(engine, size) == 3 * 2 * (3 + 4 + 4 + 3)


def test_sgm_filter_speckles_on_adversarial_maps(matcher):
    for size in (cases.SMALL,) + cases.THIN_SGM + (cases.LARGE,):
        assert cases.speckles_equal_the_oracle(matcher, size) >= 6 * len(cases.SGM_SPECKLES)
