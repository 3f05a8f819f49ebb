"""-m gpu: what surrounds the taps of a patch evaluation, on the device: the cases of tests/eval_trim_cases.py -- the fallback cameras and the geometric `families`
scene once more, a source that sees the upper half of a band of patches, its mirror image, and a two-level run in which the prior blend takes part -- against the
sequential oracle, bit for bit, through pm_sweep2_kernel with 4 and 8 lanes per pixel under buffer and pointer addressing and the engine's default.  The census of the
branches is the emulator's (tests/test_emu_eval_trim.py)."""
import pytest

from tests import eval_trim_cases as cases, tap_fallback_cases as tap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", tap.PHOTO_CASES + tap.GEO_CASES + ["families"] + cases.NEW_CASES)
def test_case_under_every_tuning(engine, case):
    for tuning in cases.TUNINGS:
        cases.run(engine, case, tuning)


@pytest.mark.parametrize("tuning", sorted(cases.PRIOR_TUNINGS))
def test_prior_blend(engine, tuning):
    cases.prior(engine, tuning)
