"""Plain SGM (minResolution = 0), the host side: the global range's int16 arithmetic (tsgm.plain_range and sgmhip_plain_range), and the product loop
tsgm.tsgm_match(..., min_resolution=0) on the CPU oracle backend -- it finds a planted disparity, it equals a literal restatement of the reference's steps bit for bit,
and it keeps the reference's sign rule (the first Match takes the range as it is, the second its negation) where that rule loses the true disparity."""
import numpy as np
import pytest

from openmvs_amd import sgm, tsgm
from tests import sgm_cases as sc
from tests import sgm_plain_cases as pc
from tests.tsgm_backends import OracleBackend


def test_plain_range_table():
    """min, max of the seed -> [minDisp, maxDisp): the table of the reference's int16 arithmetic, wraps included, by both implementations"""
    for lo, hi, a, b in pc.RANGE_TABLE:
        seed = np.array([[hi, lo, hi], [lo, hi, lo]], np.int16)
        assert tsgm.plain_range(seed) == (a, b), (lo, hi)
        assert sgm.plain_range(seed) == (a, b), (lo, hi)
    r = np.random.RandomState(5)
    for _ in range(200):                                             # the two agree on any seed
        seed = r.randint(-32768, 32768, r.randint(1, 6)).astype(np.int16)
        if r.rand() < 0.3:
            seed[0] = tsgm.NO_DISP
        assert tsgm.plain_range(seed) == sgm.plain_range(seed), seed
    assert [b - a for _, _, a, b in pc.RANGE_TABLE] == [66, 532, 992, 32, 110, 62, 32]
    with pytest.raises(ValueError):
        tsgm.plain_range(np.zeros((0, 4), np.int16))
    with pytest.raises(sgm.SGMError):
        sgm.plain_range(np.zeros((0, 4), np.int16))


def test_plain_loop_finds_a_planted_disparity():
    """stereo_pair(160, 96, 12) with a seed of -6 | +6: the range [-28, 28); one level, valid-grid shapes, and the thresholds of the tSGM test in the core"""
    args, seed, core, d, D = pc.loop_case("narrow")
    assert (d, D) == (12, 56) and args[1].shape == (96, 160) and tsgm.plain_range(seed) == (-28, 28)
    disp, cost = pc.loop_oracle("narrow")                            # asserts levels, shapes and the thresholds
    assert disp.shape == (90, 154) and cost.dtype == np.uint16


@pytest.mark.parametrize("one_sided", [False, True])
def test_plain_loop_equals_its_literal_restatement(one_sided):
    args, seed, core, d, D = pc.loop_case("narrow")
    if one_sided:
        seed = np.full_like(seed, 6)                                 # all +6: the range [-4, 28)
        assert tsgm.plain_range(seed) == (-4, 28)
        got = tsgm.tsgm_match(OracleBackend(), *args, min_resolution=0, init_left_disparity=seed)
    else:
        got = pc.loop_oracle("narrow") + (1,)
    rd, rc, rng = pc.restated_plain(OracleBackend(), *args, seed)
    assert rng == tsgm.plain_range(seed)
    assert got[2] == 1 and np.array_equal(got[0], rd) and np.array_equal(got[1], rc)
    valid = (got[0][core] != tsgm.NO_DISP).mean()
    if one_sided:
        # left -> right searches [-28, 4): the true disparity 12 is outside it.  This pins "the first Match takes the un-negated range".
        assert valid < 0.5, valid
    else:
        assert valid > 0.9


def test_plain_loop_errors():
    lb, lg, rg = sc.stereo_pair(40, 13, 2, seed=3)
    mask = np.full((13, 40), 255, np.uint8)
    with pytest.raises(ValueError, match="empty"):                   # round(13 / 2) - 6 = 0 rows of seed
        tsgm.tsgm_match(OracleBackend(), lb, lg, lb, rg, mask, mask, min_resolution=0)
    lb, lg, rg = sc.stereo_pair(40, 20, 2, seed=3)
    mask = np.full((20, 40), 255, np.uint8)
    seed = np.zeros((4, 14), np.int16); seed[0, 0] = -300; seed[1, 1] = 300
    with pytest.raises(ValueError) as e:
        tsgm.tsgm_match(OracleBackend(), lb, lg, lb, rg, mask, mask, min_resolution=0, init_left_disparity=seed)
    assert "-300" in str(e.value) and "300" in str(e.value) and "1232" in str(e.value)
    seed[:] = tsgm.NO_DISP; seed[0, 0] = -32768 + 15                 # wraps to a range of <= 0 disparities
    a, b = tsgm.plain_range(seed)
    assert b - a <= 0 or b - a > 1024
    with pytest.raises(ValueError):
        tsgm.tsgm_match(OracleBackend(), lb, lg, lb, rg, mask, mask, min_resolution=0, init_left_disparity=seed)
    with pytest.raises(ValueError, match="must be"):                 # the seed size is checked as for tSGM
        tsgm.tsgm_match(OracleBackend(), lb, lg, lb, rg, mask, mask, min_resolution=0, init_left_disparity=np.zeros((5, 14), np.int16))
