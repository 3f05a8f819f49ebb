"""The geometric term's depth gather on the wave64 emulator (tests/cpp/hipemu): the cases of tests/geo_gather_cases.py -- the quad copy of a source depth map, its
derivation at the head of every geometric call whatever changed the row-major map, and every kernel family on the term -- against the sequential oracle, bit for bit.
The library is the PM_DEBUG_REDO build: its census says what share of the (hypothesis, view) evaluations of the sweep kernels ended at the early corner test, i.e. dropped
a gather they had requested."""
import pytest

from openmvs_amd import patchmatch
from tests import emu, geo_gather_cases as cases


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


def test_quad_copy_of_every_small_size(engine):
    cases.check_quads(engine)


def test_quad_copies_are_never_stale(engine):
    cases.never_stale(engine)


@pytest.mark.parametrize("tuning", sorted(cases.TUNINGS))
def test_kernel_family(engine, tuning):
    emu.tap_census(patchmatch, reset=True)
    cases.families(engine, tuning)
    c = emu.tap_census(patchmatch, reset=True)["sweep"]
    dropped = c["early_outside"] / max(1, c["early_outside"] + c["optimistic"])
    print("%s: %d evaluations of the sweep kernels, %.1f %% ended at the corner test (their gather dropped), %.1f %% of the rest redone" %
          (tuning, c["early_outside"] + c["optimistic"], 100 * dropped, 100 * c["redone"] / max(1, c["optimistic"])))
    assert c["optimistic"] > 50000
    if tuning.startswith("sweep2-lanes4"):
        assert dropped > 0.02, "the case is there for the gathers that are requested and dropped"
