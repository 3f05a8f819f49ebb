"""-m gpu: SemiGlobalMatcher::Match on the device on the hand-built problems of tests/sgm_match_edge_cases.py -- every mapping of work to lanes, both aggregation routes,
against oracle.pyoracle.sgm_match bit for bit (cost volume, 8-path sums, disparity, cost).  Every problem first proves that it reaches the edge it is named after.

Each family runs twice on one engine with its problems interleaved by size (the largest, the smallest, the second largest, ...; the second pass the other way round), so
that what an earlier, larger problem left in the engine's scratch -- the eight byte volumes, the accumulators, the 256 spare bytes behind the cost volume -- would show.

This file is the judge of what the emulator cannot see: the conversion of a grey difference that is not finite (the device saturates where x86 gives INT_MIN, unless
sgmp_p2_index decides first) and the device's handling of subnormal grey values."""
import time

import numpy as np
import pytest

from openmvs_amd import sgm
from tests import sgm_match_edge_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    m = sgm.SemiGlobalMatcherHIP(0)
    yield m
    m.close()


def interleaved(family):
    by_size = list(np.argsort([p.n for p in ec.problems(family)], kind="stable"))
    out = []
    while by_size:
        out.append(int(by_size.pop()))
        if by_size:
            out.append(int(by_size.pop(0)))
    return out


@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_device_match(matcher, family):
    order = interleaved(family)
    t0 = time.time()
    for p in ec.problems(family):
        ec.prove(p)
    t1 = time.time()
    runs = ec.check_family(matcher, family, order=order) + ec.check_family(matcher, family, order=order[::-1])
    print("\n%s: %d problems, %d runs compared in %.2f s (predicates and oracle before: %.2f s)" % (family, len(order), runs, time.time() - t1, t1 - t0))
    assert runs >= 8 * len(order)


def test_device_refusals(matcher):
    for _ in range(2):
        ec.check_refusals(matcher)
