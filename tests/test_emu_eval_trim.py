"""What surrounds the taps of a patch evaluation, on the wave64 emulator: the cases of tests/eval_trim_cases.py against the sequential oracle, bit for bit, through
libpmhip_emu_redo.so (PM_DEBUG_REDO), whose census says for the two new cases that the branch each was made for ran: `row0_outside` ends evaluations at the test of the
first row's corners before any load, `half_seen` passes that test everywhere and is found outside by the verdict after the gather."""
import ctypes

import pytest

from openmvs_amd import patchmatch
from tests import emu, eval_trim_cases as cases, tap_fallback_cases as tap


@pytest.fixture(scope="module")
def pm_census():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so", defines=["PM_DEBUG_REDO"], out_name="libpmhip_emu_redo.so"):
        yield


@pytest.fixture()
def engine(pm_census):
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    yield e
    e.close()


def _outside_after_gather(reset=True):
    out = (ctypes.c_ulonglong * 2)()
    patchmatch.load_library().pm_debug_tap_census_outside(out, 1 if reset else 0)
    return {"init": int(out[0]), "sweep": int(out[1])}


@pytest.mark.parametrize("tuning", sorted(cases.TUNINGS))
@pytest.mark.parametrize("case", tap.PHOTO_CASES + tap.GEO_CASES + ["families"])
def test_earlier_case(engine, case, tuning):
    cases.run(engine, case, tuning)


@pytest.mark.parametrize("tuning", sorted(cases.TUNINGS))
@pytest.mark.parametrize("case", cases.NEW_CASES)
def test_new_case_and_its_branch(engine, case, tuning):
    emu.tap_census(patchmatch, reset=True); _outside_after_gather()
    cases.run(engine, case, tuning)
    c = emu.tap_census(patchmatch, reset=True)["sweep"]; late = _outside_after_gather()["sweep"]
    print("%s, %s: %d evaluations of the sweep kernels, %d ended before any load, %d found outside after the gather" % (case, tuning, c["early_outside"] + c["optimistic"], c["early_outside"], late))
    assert c["optimistic"] > 100000, c
    band = cases.BAND_ROWS[case] * cases.ROW_PIXELS          # every pixel of the band scores a hypothesis against the shifted source at least once
    if case == "row0_outside" and tuning == "default":
        assert late >= band, (c, late)       # (the engine's own choice for one reference view is a speculative kernel, which has no test before the loads)
    elif case == "row0_outside":
        assert c["early_outside"] >= band, (c, late)
    else:
        assert c["early_outside"] == 0 and late >= band, (c, late)   # no first row leaves any source: whatever is outside is found after the gather


@pytest.mark.parametrize("tuning", sorted(cases.PRIOR_TUNINGS))
def test_prior_blend(engine, tuning):
    cases.prior(engine, tuning)
