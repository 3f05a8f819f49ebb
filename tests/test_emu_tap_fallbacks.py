"""The fallbacks of the optimistic tap path (pm_score_view) on the wave64 emulator: the cases of tests/tap_fallback_cases.py through libpmhip_emu_redo.so -- the emulated
library built with PM_DEBUG_REDO, whose census says how often the init and sweep kernels rechecked a patch's positions (branch 4) or redid it through the guarded path
(branch 1).  Per case and tuning: first the conditions on the input -- the oracle's map is mostly valid, the census shows the case's branch deciding at least the share
tests/tap_fallback_cases.FLOORS names (about half of what the cases produce: twin 1.7 - 3.3 % rechecked, behind / own_size / eight 32 - 38 % redone, in_scene 18 - 20 %) --
then emulator == oracle bit for bit.  The floors say that the branch ran, never what it returns.  What the emulator cannot see is the device's division chain
(pm_div2_inrange is `/` in a host build): tests/test_zz_gpu_tap_fallbacks.py runs the same cases there."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import patchmatch
from tests import emu, tap_fallback_cases as cases


@pytest.fixture(scope="module")
def pm_census():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so", defines=["PM_DEBUG_REDO"], out_name="libpmhip_emu_redo.so"):
        yield


def _share(rows, branch):
    opt = sum(r["optimistic"] for r in rows)
    return sum(r[b] for r in rows for b in branch.split("+")) / opt if opt else None


@pytest.mark.parametrize("tuning", sorted(cases.EMU_TUNINGS))
@pytest.mark.parametrize("case", cases.PHOTO_CASES + cases.GEO_CASES)
def test_tap_fallback_case(pm_census, case, tuning):
    from openmvs_amd.patchmatch import PatchMatchHIP
    cases.check_input(case)
    e = PatchMatchHIP(0)
    try:
        cases.set_tuning(e, cases.EMU_TUNINGS[tuning])
        emu.tap_census(patchmatch, reset=True)
        results = cases.compute(e, case)
        census = emu.tap_census(patchmatch, reset=True)
    finally:
        e.close()
    branch, floor = cases.FLOORS[case]
    assert census["sweep"]["optimistic"] > 100000, census
    for what, rows, floor in (("init and sweep kernels", [census["init"], census["sweep"]], floor), ("init kernel", [census["init"]], cases.INIT_FLOORS.get(case, floor))):
        share = _share(rows, branch)          # (None: the init kernel scored through the guarded rows -- pointer addressing, mode 0)
        assert share is None or share >= floor, "%s, %s: %s decided %.2f %% of the %s' optimistic evaluations, the case needs %.0f %%: %r" % (case, tuning, branch, 100 * share, what, 100 * floor, census)
    cases.compare(results, "%s, %s" % (case, tuning))


def test_tap_fallbacks_do_not_depend_on_the_execution_order():
    """Every photometric case once more with the lanes of every workgroup and the workgroups of every grid in reverse order (HIPEMU_ORDER, as tests/test_emu_kernels.py)."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "sweep2-lanes4 and not geo"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPEMU_ORDER="reverse"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
