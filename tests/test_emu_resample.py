"""The level resamplers of csrc/pm_kernels.hip on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py), each kernel launched once through
pmhip_resample -- production's launch helper -- at every small size at which its rule can go wrong, against the literal walks of tests/resample_cases.py, bit for bit;
then the oracle's resamplers against the same walks.  The cases are those of tests/test_zz_gpu_resample.py; the grid-stride cases run on the device only.  The predicates
(which branch, which clamp, which sizes tell the two nearest rules apart) are computed on the walks alone."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import patchmatch
from tests import emu
from tests import resample_cases as cases


@pytest.fixture(scope="module")
def emulated():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield lambda: patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine(emulated):
    e = emulated()
    yield e
    e.close()


def test_the_emulated_library_exports_the_hook(emulated):
    assert hasattr(patchmatch.load_library(), "pmhip_resample") and hasattr(patchmatch.load_library(), "hipemu_counters")


# ---- on the walks alone ----------------------------------------------------------------------------------------------------------------------------------
def test_the_two_nearest_rules_differ_at_exactly_the_listed_sizes():
    cases.disagreement_predicate()


def test_upsample_sweep_reaches_both_clamps_and_cannot_tell_the_scales_apart():
    cases.upsample_predicates()


def test_end_to_end_mask_tells_the_two_rules_apart():
    cases.e2e_predicate()


def test_level_masks_from_a_level0_sized_label_image_equal_the_direct_route():
    cases.label_route_agrees_at_level0_size()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------------
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


def test_hook_refuses_sizes_a_kind_does_not_take(engine):
    import numpy as np
    for kind, s, d, arg in ((engine.RESAMPLE_AREA, (10, 10), (4, 5), 2), (engine.RESAMPLE_NEAREST_DOWN, (10, 10), (5, 6), 2), (engine.RESAMPLE_SKEW, (10, 10), (10, 9), 0)):
        n = {engine.RESAMPLE_NEAREST_DOWN: 4}.get(kind, 1)
        with pytest.raises(patchmatch.PatchMatchError):
            engine.resample(kind, np.zeros(n * s[0] * s[1], np.float32), s, np.zeros(n * d[0] * d[1], np.float32), d, arg=arg)
    src = cases.coded(10, 9)                                   # the engine stays usable
    cases.same_bits(engine.resample(engine.RESAMPLE_SKEW, src, (10, 9), cases.filled(90), (10, 9)), cases.skew_walk(src), "skew after the refusals")


def test_end_to_end_striped_mask_at_86x58(emulated):
    e = emulated()
    try:
        cases.e2e_case(e, cases.e2e_scene())
    finally:
        e.close()


@pytest.mark.parametrize("order", ["reverse"])
def test_kernel_results_do_not_depend_on_the_execution_order(order):
    """Every kernel case again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER, as tests/test_emu_kernels.py does): each
    output has one writer, so the bits must not move."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_kernel_ and not execution_order"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPEMU_ORDER=order), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
