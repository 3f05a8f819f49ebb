"""-m gpu, collected last: the level resamplers of csrc/pm_kernels.hip on the device -- each kernel launched once through pmhip_resample, production's launch helper, at
every small size at which its rule can go wrong, against the literal walks of tests/resample_cases.py, bit for bit; then the oracle's resamplers against the same walks.
The cases are shared with the emulator suite (tests/test_emu_resample.py), which also holds the predicates on the walks alone; the grid-stride cases (a destination just
above the kernel's block cap, so that the loop takes a second trip) run only here."""
import pytest

from openmvs_amd import patchmatch
from tests import resample_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = patchmatch.PatchMatchHIP(0)
    yield e
    e.close()


@pytest.mark.parametrize("f", cases.AREA_FACTORS)
def test_kernel_area(engine, f):
    cases.area_cases(engine, f)


@pytest.mark.parametrize("f", cases.AREA_FACTORS)
def test_kernel_nearest_down(engine, f):
    cases.nearest_down_cases(engine, f)


@pytest.mark.parametrize("transpose", (0, 1), ids=("widths", "heights"))
@pytest.mark.parametrize("nearest_depth", (0, 1), ids=("linear", "nearest"))
def test_kernel_upsample(engine, nearest_depth, transpose):
    cases.upsample_cases(engine, nearest_depth, transpose)


@pytest.mark.parametrize("transpose", (0, 1), ids=("widths", "heights"))
@pytest.mark.parametrize("level", (1, 2, 3))
def test_kernel_mask_level(engine, level, transpose):
    cases.mask_level_cases(engine, transpose, level)


@pytest.mark.parametrize("transpose", (0, 1), ids=("widths", "heights"))
@pytest.mark.parametrize("level", (1, 2, 3))
def test_kernel_nearest_up(engine, level, transpose):
    cases.nearest_up_cases(engine, transpose, level)


def test_kernel_skew(engine):
    cases.skew_quad_cases(engine, engine.RESAMPLE_SKEW)


def test_kernel_quad(engine):
    cases.skew_quad_cases(engine, engine.RESAMPLE_QUAD)


@pytest.mark.parametrize("name", cases.GRID_STRIDE)
def test_grid_stride_loop_takes_a_second_trip(engine, name):
    cases.grid_stride_case(engine, name)


def test_end_to_end_striped_mask_at_86x58():
    cases.e2e_predicate()
    e = patchmatch.PatchMatchHIP(0)
    try:
        cases.e2e_case(e, cases.e2e_scene())
    finally:
        e.close()
