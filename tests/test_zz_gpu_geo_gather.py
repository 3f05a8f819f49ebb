"""-m gpu: the geometric term's depth gather on the device -- the cases of tests/geo_gather_cases.py (counted and described on the emulator by
tests/test_emu_geo_gather.py) against the sequential oracle, bit for bit."""
import pytest

from tests import geo_gather_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture()
def engine():
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
    cases.families(engine, tuning)
