"""The post-filters on adversarial maps (tests/post_filter_cases.py) on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py), run
through the same C ABI and Python mirrors as on the device, against the sequential oracle -- bit for bit.  The cases are those of
tests/test_zz_gpu_post_filter_edges.py, at 67 x 37 and at the narrowest sizes; the device adds 331 x 211.

The ramps of the segment cases fill the list of one-directional edges to its bound, 2wh - w - h pairs; while the list was sized at one pair per pixel the engine
refused them ("remove_small_segments: asymmetric edge list overflow")."""
import os
import subprocess
import sys

import pytest

from openmvs_amd import patchmatch, sgm
from tests import emu
from tests import post_filter_cases as cases

SIZES = (cases.SMALL,) + cases.THIN
ids = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def engine():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        e = patchmatch.PatchMatchHIP(0)
        yield e
        e.close()


@pytest.fixture(scope="module")
def matcher():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        m = sgm.SemiGlobalMatcherHIP(0)
        yield m
        m.close()


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_remove_small_segments_on_adversarial_maps(engine, size):
    assert cases.segments_equal_the_oracle(engine, size) >= 11 * len(cases.SPECKLE_SIZES) * len(cases.SEGMENT_THRESHOLDS)


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_gap_interpolation_on_adversarial_maps(engine, size):
    assert cases.gaps_equal_the_oracle(engine, size) == 30 * len(cases.GAP_SIZES) * len(cases.GAP_THRESHOLDS)


@pytest.mark.parametrize("size", (cases.SMALL,) + cases.THIN_SCENE, ids=ids)
def test_filter_depth_map_on_tied_splats(engine, size):
    assert cases.filter_equals_the_oracle(engine, size) == 3 * 2 * (3 + 4 + 4 + 3)


@pytest.mark.parametrize("size", (cases.SMALL,) + cases.THIN_SGM, ids=ids)
def test_sgm_filter_speckles_on_adversarial_maps(matcher, size):
    assert cases.speckles_equal_the_oracle(matcher, size) >= 6 * len(cases.SGM_SPECKLES)


@pytest.mark.parametrize("order", ["reverse"])
def test_segment_and_speckle_results_do_not_depend_on_the_execution_order(order):
    """The union-find cases again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER, as
    tests/test_emu_kernels.py::test_results_do_not_depend_on_the_execution_order does): which union wins a root changes, the bits must not."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    env = dict(os.environ, HIPEMU_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "segments_on or speckles_on"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
