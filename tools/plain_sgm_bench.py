"""Plain SGM timing (GPU box): one uniform range at 2048x1536 -- D = 256 through the pixel-table entry (sgmhip_set_problem: sgm_cost_uni_kernel<256>, sgm_path_kernel<4>)
and through sgmhip_set_problem_uniform, D = 512 and 1024 through the latter (csrc/sgm_kernels_wide.hip) -- with per-kernel HIP-event times, five repeats each and their
spread; then whole plain pairs (the two of tests/sgm_plain_cases.loop_case and a 2048x1536 one with D = 432), resident call against the step-wise loop.
Output kept in profiles/plain_sgm_bench.log."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openmvs_amd import sgm
from tests import sgm_cases as sc

w, h = 2048, 1536
REPEATS, MATCHES = 5, 3
lb, lg, rg = sc.stereo_pair(w, h, 21, seed=9)
m = sgm.SemiGlobalMatcherHIP(0)
nPix = (w - 6) * (h - 6)


def measure(label, D, route):
    lo = 21 - D // 2                                                 # the planted disparity in the middle of the range
    if route == "table":
        px = np.zeros(nPix, sgm.PIXEL_DTYPE)
        px["idx"] = np.arange(nPix, dtype=np.uint64) * np.uint64(D); px["minDisp"] = lo; px["maxDisp"] = lo + D
        m.set_problem(lb, lg, rg, px, nPix * D, D)
    else:
        m.set_problem_uniform(lb, lg, rg, lo, lo + D)
    n = nPix * D
    m.Match()                                                        # warm-up: allocates the byte volumes
    hit = float((m.results()[0] == 21).mean())
    rows = []
    for _ in range(REPEATS):
        m.stats_reset(True); t = time.time()
        for _ in range(MATCHES): m.Match(sync=False)
        m.sync(); dt = (time.time() - t) / MATCHES
        s = m.stats_get()
        rows.append((dt * 1e3, s.costMs / MATCHES, s.aggrMs / MATCHES, s.wtaMs / MATCHES))
    a = np.array(rows)
    med, lo_, hi_ = np.median(a, 0), a.min(0), a.max(0)
    print("%-28s numCosts %7.1fM: %8.2f ms/Match [%.2f .. %.2f] (cost %.2f [%.2f .. %.2f], aggr %.2f [%.2f .. %.2f], wta %.2f) = %.4f ns/cost [%.4f .. %.4f], %.0f GB/s on the 43 B/cost model; winner = 21 at %.3f of the pixels" % (
        label, n / 1e6, med[0], lo_[0], hi_[0], med[1], lo_[1], hi_[1], med[2], lo_[2], hi_[2], med[3], med[0] * 1e6 / n, lo_[0] * 1e6 / n, hi_[0] * 1e6 / n, 43.0 * n / 1e9 / (med[0] / 1e3), hit), flush=True)
    return m.results()[0]


print("plain SGM, %dx%d, %d repeats of %d Matches each: median [min .. max]" % (w, h, REPEATS, MATCHES), flush=True)
d_table = measure("D = 256, pixel table", 256, "table")
d_uni = measure("D = 256, uniform entry", 256, "uniform")
print("D = 256: the two entries give identical disparities: %s" % bool(np.array_equal(d_table, d_uni)), flush=True)
measure("D = 512, uniform entry", 512, "uniform")
measure("D = 1024, uniform entry", 1024, "uniform")
m.P2s = np.minimum(m.P2s.astype(np.int64) * 40 + 200, 3000).astype(np.uint16)
measure("D = 512, u16 atomic sums", 512, "uniform")
m.P2s = sgm.generate_p2s()

# one whole plain pair: the resident call against the step-wise loop through host buffers
from openmvs_amd import tsgm
from tests import sgm_plain_cases as pc
from tests.tsgm_backends import DeviceBackend
for name in ("narrow", "wide"):
    (a_lb, a_lg, a_rb, a_rg, a_lm, a_rm), seed, core, d, D = pc.loop_case(name)
    m.tsgm_match(a_lb, a_rb, a_lg, a_rg, a_lm, a_rm, min_resolution=0, init_left_disparity=seed)
    t = time.time(); d1, c1, lv = m.tsgm_match(a_lb, a_rb, a_lg, a_rg, a_lm, a_rm, min_resolution=0, init_left_disparity=seed); t1 = time.time() - t
    t = time.time(); d2, c2, _ = tsgm.tsgm_match(DeviceBackend(m, None), a_lb, a_lg, a_rb, a_rg, a_lm, a_rm, min_resolution=0, init_left_disparity=seed); t2 = time.time() - t
    print("plain pair %dx%d, D = %d: resident call %.2f ms, step-wise loop %.2f ms, identical: %s, valid %.3f" % (
        a_lg.shape[1], a_lg.shape[0], D, t1 * 1e3, t2 * 1e3, bool(np.array_equal(d1, d2) and np.array_equal(c1, c2)), float((d1 != 32767).mean())), flush=True)
# the same at full size: a synthetic 2048x1536 pair with a planted disparity of 21 and a seed of -100 | +100 at half resolution: D = 2 (200 + 16) = 432
rb = np.roll(lb, 21, axis=1); mask = np.full((h, w), 255, np.uint8)
seed = pc.two_sided_seed(w, h, 100)
m.tsgm_match(lb, rb, lg, rg, mask, mask, min_resolution=0, init_left_disparity=seed)
t = time.time(); d1, c1, lv = m.tsgm_match(lb, rb, lg, rg, mask, mask, min_resolution=0, init_left_disparity=seed); t1 = time.time() - t
t = time.time(); d2, c2, _ = tsgm.tsgm_match(DeviceBackend(m, None), lb, lg, rb, rg, mask, mask, min_resolution=0, init_left_disparity=seed); t2 = time.time() - t
print("plain pair %dx%d, D = %d: resident call %.1f ms, step-wise loop %.1f ms, identical: %s, valid %.3f" % (
    w, h, tsgm.plain_range(seed)[1] - tsgm.plain_range(seed)[0], t1 * 1e3, t2 * 1e3, bool(np.array_equal(d1, d2) and np.array_equal(c1, c2)), float((d1 != 32767).mean())), flush=True)
