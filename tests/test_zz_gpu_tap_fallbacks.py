"""-m gpu: what protects the sweep kernels' unguarded division, on the device.

1. pm_div2_inrange itself (pm_math_kernel kinds 10 and 11: either slot of the packed chain) against the correctly rounded quotient over the domain the kernels claim for it
   -- 2^-40 <= z <= 2^40, |x| < 5e17 -- with both ends, every power of two between them and their neighbours, and numerators around the image test's edges.  The host
   build of the function is `/`, so only this test sees the reciprocal chain.
2. The cases of tests/tap_fallback_cases.py -- cameras that make pm_score_view's recheck and redo branches decide percents of the evaluations (counted on the emulator by
   tests/test_emu_tap_fallbacks.py) -- against the sequential oracle, bit for bit, under every mapping of the batch onto the device."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import tap_fallback_cases as cases

pytestmark = pytest.mark.gpu

N = 1 << 20
Z_LO, Z_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
TINY = 2.0 ** -126          # the smallest normal float


def _denominators(r, n):
    """n values of z: a quarter of them the ends of [2^-40, 2^40], every power of two between them and the neighbours of each, 1 ulp towards the inside; the rest log-uniform."""
    p = np.float32(2.0) ** np.arange(-40, 41, dtype=np.float32)
    special = np.unique(np.clip(np.concatenate([p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))]), Z_LO, Z_HI))
    assert special.size == 3 * 81 - 2 and special[0] == Z_LO and special[-1] == Z_HI
    z = np.exp2(r.uniform(-40, 40, n)).astype(np.float32)
    z[:n // 4] = special[r.randint(0, special.size, n // 4)]
    z[0], z[1] = Z_LO, Z_HI
    return np.clip(z, Z_LO, Z_HI)[r.permutation(n)]


def div_sets():
    """[(name, a, b)]: numerators and denominators of the three sets, N values each."""
    r = np.random.RandomState(40)
    sign = lambda n: np.where(r.rand(n) < 0.5, -1.0, 1.0)
    # any numerator the kernels allow: +0, -0 and magnitudes from the smallest normal float to 5e17, log-uniform, both signs
    a = (sign(N) * np.exp(r.uniform(np.log(TINY), np.log(5e17), N))).astype(np.float32)
    a[::64] = 0.0; a[32::64] = -0.0
    a[1], a[2] = np.float32(5e17), np.float32(-5e17)
    sets = [("any numerator", a, _denominators(r, N))]
    # pixel-sized quotients: the positions the kernels work with
    b = _denominators(r, N)
    sets.append(("positions", (b.astype(np.float64) * r.uniform(-100, 70000, N)).astype(np.float32), b))
    # quotients astride the edges of the image test (1, w - 2, h - 2): a = fl(k b) and its neighbours 1 and 2 ulp either side
    b = _denominators(r, N)
    k = np.array([1, 94, 70, 1918, 1078, 3838, 2158, 65533], np.float32)[r.randint(0, 8, N)]
    a = k * b
    for _ in range(2):
        step = r.randint(-1, 2, N)
        a = np.where(step < 0, np.nextafter(a, np.float32(0)), np.where(step > 0, np.nextafter(a, np.float32(np.inf)), a))
    sets.append(("image edges", a.astype(np.float32), b))
    return sets


NUM_LO = 2.0 ** -102        # numerators from here on have exact residuals in the chain (csrc/pm_math.h)


def div_disagreements(dev, a, b):
    """The contract of pm_div2_inrange (csrc/pm_math.h, derived there) on one set; returns the indices that break (the exact rule, the rule for quotients below 1).
    Exact rule -- the numerator is +0 or has magnitude >= 2^-102, and the exact quotient has magnitude >= 2^-126: the IEEE quotient, bit for bit.
    A numerator of -0 gives +0, not the IEEE -0: the chain's first residual is fma(-z, -0, -0) = +0 + -0 = +0 and the correction fma(+0, r, -0) = +0.
    Below the exact rule -- a subnormal exact quotient, or a numerator of magnitude below 2^-102, whose residual x - z q (a multiple of 2^-47 times x's leading power of two) is
    no longer a float: the result may be off in its last place (758 of 2^20 log-uniform numerators are, all below 2.5e-35), and all that is asserted is that it stays where
    the exact quotient is, far below 1: |q| < 2^-125 for a subnormal quotient, |q| < 2^-61 for a tiny numerator (the exact one is below 2^-102 / 2^-40).  Every comparison
    the kernels make -- against 1 and the image size, as floats or as bit patterns -- then agrees, and the sums of an accepted patch, whose positions are >= 1, never hold
    such a value.  This is narrower than "bit for bit wherever the exact quotient is 0 or at least 2^-126": that rule fails on the device for the two classes above
    (measured once: 16 384 of 16 384 numerators of -0 returned +0; 758 numerators below 2.5e-35 were off by one ulp, quotients from 1.2e-38 to 5.8e-24)."""
    q = a.astype(np.float64) / b.astype(np.float64)
    want = po.math_eval(10, a, b)
    assert np.array_equal(want.view(np.uint32), (a / b).view(np.uint32)) and np.array_equal(want.view(np.uint32), q.astype(np.float32).view(np.uint32))   # three roads to the IEEE quotient
    want = np.where(a == 0, np.float32(0), want)       # (-0 / z: +0, see above)
    exact = (a == 0) | ((np.abs(a) >= NUM_LO) & (np.abs(q) >= TINY))
    bad_exact = np.flatnonzero(exact & (dev.view(np.uint32) != want.view(np.uint32)))
    bound = np.where(np.abs(q) < TINY, 2.0 ** -125, 2.0 ** -61)
    bad_small = np.flatnonzero(~exact & ~(np.abs(dev) < bound))
    return bad_exact, bad_small


def test_unguarded_division_is_the_ieee_quotient_on_its_claimed_domain():
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    try:
        for name, a, b in div_sets():
            assert a.size == N and b.min() == Z_LO and b.max() == Z_HI and np.abs(a).max() <= 5e17
            for kind in (10, 11):
                dev = e.math_eval(kind, a, b)
                bad_exact, bad_sub = div_disagreements(dev, a, b)
                print("%s, kind %d: %d of %d values differ from the IEEE quotient, %d quotients below the exact rule out of bounds" % (name, kind, bad_exact.size, N, bad_sub.size))
                i = bad_exact[:5]
                assert bad_exact.size == 0, "%s, kind %d: %d values differ from a / b, first %r / %r: %r vs %r" % (name, kind, bad_exact.size, a[i], b[i], dev[i], (a / b)[i])
                assert bad_sub.size == 0, "%s, kind %d: %d quotients of tiny numerators or subnormal size left their bound, first %r / %r: %r" % (name, kind, bad_sub.size, a[bad_sub[:5]], b[bad_sub[:5]], dev[bad_sub[:5]])
    finally:
        e.close()


def _tunings(case):
    t = list(cases.DEVICE_TUNINGS.items())
    if case.startswith("geo-"):
        t += [("sweep2-lanes4-buffer, 3 view groups", dict(cases.DEVICE_TUNINGS["sweep2-lanes4-buffer"], viewGroups=3)), ("default, 3 view groups", dict(cases.product_defaults(), viewGroups=3))]
    return t


@pytest.mark.parametrize("case", cases.PHOTO_CASES + cases.GEO_CASES)
def test_tap_fallback_case(case):
    from openmvs_amd.patchmatch import PatchMatchHIP
    e = PatchMatchHIP(0)
    try:
        for name, tuning in _tunings(case):
            cases.set_tuning(e, tuning)
            cases.run(e, case, name)
    finally:
        e.close()
