"""The tSGM steps around Match on the hand-built maps of tests/sgm_post_edge_cases.py, on the CPU, against the sequential oracle and bit for bit (NaN results by position):
the host+device functions of csrc/sgm_post.h under the host-loop emulation (tests/cpp/sgm_post_emul.cpp) in ascending, descending and two scrambled thread orders, and the
kernels themselves (libsgmhip compiled against the wave64 emulator, tests/emu.py) through the C ABI, forwards here and with every workgroup and lane in reverse in a child
run.  Every case first proves on the oracle's result that it reaches the edge it is named after.

The conversions that x86 and the GPU perform differently (NaN and out-of-int to int) cannot fail here -- the emulator converts as x86 does; the device file
tests/test_zz_gpu_sgm_post_edges.py is their judge.  The device scan's carry (more than 256 tiles of 1024 pixels) runs there only: an emulated 520 x 518 loop takes minutes,
against seconds for every other emulated SGM case."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from openmvs_amd import sgm
from oracle import pyoracle as po
from tests import emu
from tests import sgm_post_edge_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (ec.SMALL,) + ec.THIN
ids = lambda s: "%dx%d" % s if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def loops():
    src = os.path.join(HERE, "cpp", "sgm_post_emul.cpp")
    out = os.path.join(HERE, "cpp", "build", "libsgm_post_emul.so")
    hdr = os.path.join(HERE, "..", "openmvs_amd", "csrc", "sgm_post.h")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(out):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out + ".tmp", src])
        os.replace(out + ".tmp", out)
    L = C.CDLL(out)
    yield L
    L.emu_sgm_set_order(0)


@pytest.fixture(scope="module")
def matcher():
    with emu.emulated(sgm, "SGMHIP_LIB", "libsgmhip_emu.so"):
        m = sgm.SemiGlobalMatcherHIP(0)
        yield m
        m.close()


# (131 x 83 adds the full 41 x 41 window of Disparity2RangeMap; the other families run at that size on the device)
@pytest.mark.parametrize("family,size", [(f, s) for f in sorted(ec.FAMILIES) for s in SIZES] + [("ranges", ec.LARGE)], ids=ids)
def test_host_loops_in_four_thread_orders(loops, family, size):
    be = ec.Steps(loops, "emu_sgm_")
    for order in (0, 1, 2, 3):                                       # scrambled, ascending, descending, scrambled with other seeds
        loops.emu_sgm_set_order(order)
        assert ec.check_family(be, family, size, predicates=order == 0) > 0


@pytest.mark.parametrize("size", SIZES, ids=ids)
@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_emulated_kernels(matcher, family, size):
    assert ec.check_family(matcher, family, size) > 0


def test_emulated_limits(matcher):
    """65534 columns flip, 65535 are refused (the column key has 16 bits); 32 pairs fuse, 33 are refused."""
    c = ec.flip_widest()
    want = ec.run(c, ec.ORACLE); c.check(want)
    ec.same(ec.run(c, matcher), want, c.name)
    with pytest.raises(sgm.SGMError):
        matcher.FlipDirection(np.zeros((1, 65535), np.int16))
    deps, rgs, cfs, _ = ec.fusion_cases(5, 3, 33)[0].args
    with pytest.raises(sgm.SGMError):
        matcher.FusePairs(deps, rgs, cfs, 1)


def test_refine_with_hand_written_sums(loops):
    px, acc, maps = ec.refine_synthetic()
    be = dict(impl=loops, prefix="emu_sgm_")
    zero = 0
    for order in (0, 1, 2):
        loops.emu_sgm_set_order(order)
        for name, d in maps.items():
            for mode in range(7):
                for steps in (1, 4, 64):
                    a = po.sgm_refine(d, px, acc, mode, steps); b = po.sgm_refine(d, px, acc, mode, steps, **be)
                    assert np.array_equal(a, b), (name, mode, steps)
                    zero += int((a == 0).sum())
    assert zero > 0


def refine_on_the_resident_problem(m, size):
    """The body of the emulated and the device test: Match on the hand-built problem, then every map x mode x step count through set_disparity + RefineDisparityMap."""
    bgr, gray, px, n, mxd, mn, mx, maps = ec.refine_problem(*size)
    od, oc, ocosts, oacc = po.sgm_match(bgr, gray, gray, px, n, mxd, m.P1, m.P2s)
    st = ec.refine_predicates(oacc, px, mn, mx, maps)
    assert st["zero_other"] > 0 and st["eq_prev"] > 0 and st["eq_next"] > 0 and st["wraps"] > 0 and {1, 2, 3} <= st["widths"], st
    m.set_problem(bgr, gray, gray, px, n, mxd); m.Match()
    d, c, costs, acc = m.results(volumes=True)
    assert np.array_equal(acc, oacc) and np.array_equal(d, od)
    hit = 0
    for name, dm in maps.items():
        for mode in range(7):
            for steps in (1, 4, 64):
                want = po.sgm_refine(dm, px, oacc, mode, steps)
                for k in range(2):
                    m.set_disparity(dm); m.RefineDisparityMap(mode, steps)
                    got = m.results()[0]
                    assert np.array_equal(got, want), "%s mode %d steps %d call %d: %d differ" % (name, mode, steps, k, int((got != want).sum()))
                if mode and steps > 1:
                    hit += int(((want == 0) & (dm != ec.NO) & (dm != 0)).sum())      # +-inf and NaN offsets convert to INT_MIN, which int16_t cuts to 0
    assert hit > 0
    return hit


def test_emulated_refine_on_a_resident_problem(matcher):
    refine_on_the_resident_problem(matcher, ec.SMALL)


@pytest.mark.parametrize("order", ["reverse"])
def test_results_do_not_depend_on_the_execution_order(order):
    """The kernels again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER, as tests/test_emu_kernels.py does): who wins
    an atomic max / min or a union-find root changes, the bits must not."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    env = dict(os.environ, HIPEMU_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "emulated"],
                       cwd=os.path.dirname(HERE), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
