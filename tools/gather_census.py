"""Census of the sweep kernel's tap gathers on the wave64 emulator (no GPU needed): for the shipped lane order of pm_sweep2_kernel, how many distinct 64-byte blocks
(four 16-byte quad-image entries) the four lanes of a quad touch in one tap wave-load -- what the texture-address unit is paid by.

    python tools/gather_census.py [WxH ...]          # default: 512x288 960x540
    python tools/gather_census.py --geo [WxH ...]    # the geometric term's depth gather instead (profiles/geo_gather_census.txt)
    python tools/gather_census.py --widen [WxH ...]  # the speculative kernel pm_sweep_widen_kernel<2> instead (profiles/widen_lane_order_census.txt)

Builds the emulated library (tests/emu.py's recipe) with -DPM_GATHER_CENSUS -- a hook in the HOST branch of pm_bufload5 and two markers in pm_visit, nothing in the device
build -- and runs, in a child process per scene, the photometric pass (3-level pyramid) of view 4 of the nine-view synthetic scene with pm_sweep2_kernel<4,2> forced.
Prints, per level (image width): tap wave-loads, active lanes per load, mean blocks per wave-load under the shipped view-major order and under the pixel-major order it
replaced (the same indices, regrouped), mean blocks per quad, and the share of quads by the number of blocks they touch.  Not a pass / fail test:
profiles/lane_order_census.txt is its output.

--geo: the same scenes through one geometric round on top of the photometric pass (the sources' depth maps: the ground truth).  A hook in the host branch of pm_geo_request
records the footprint every lane requests; printed: per wave-gather -- one (trip, view round) of a wave of pm_sweep2_kernel<4,2> -- the distinct 64-byte blocks the lanes touch
with the row-major float map read by two 8-byte loads on two rows (what the kernels did before the quad copy) and with a quad copy in row-major, anti-diagonal-major and
folded anti-diagonal-major order (the shipped one, pm_dq_index).

--widen: the same scenes with the two-wide speculative kernel forced (wideHyps = 2: 16 lanes per pixel, four pixels per wave).  Two markers in pm_sweep_widen_kernel (host
branch only) name the trip and arm the same hook in pm_bufload5, filing each lane's indices under the lane it would have in the candidate order lane = sub * 4 + pixel
(sub = hypothesis slot * 8 + source view: a quad is four neighbouring diagonal pixels on one source view); the second column regroups the same indices in the shipped
order, lane = pixel * 16 + sub, where a quad is one pixel's four source views."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD = """
import sys
sys.path.insert(0, %(root)r)
from openmvs_amd import patchmatch, synth
from openmvs_amd.patchmatch import PatchMatchHIP, default_params
patchmatch.load_library()
W, H = %(w)d, %(h)d
sc = synth.make_scene(9, W, H, n_src=8)
e = PatchMatchHIP(0)
if %(widen)d:
    got = e.tuning(wideMaxViews=64, wideHyps=2)
    assert got["wideHyps"] == 2 and got["wideMaxViews"] == 64
else:
    e.tuning(wideMaxViews=-1, sweepLanes=4, wideHyps=-1)
e.Init(False)
ids = [4] + list(sc.neighbors[4])
d, n, c = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[4], sc.dmax[4], params=default_params(seed=5, nSubResolutionLevels=2))
print("scene %%dx%%d, 9 views, view 4 against 8 sources, photometric pass over 3 levels: valid %%.3f" %% (W, H, float((d > 0).mean())), file=sys.stderr)
if %(geo)d:
    e.Init(True)
    p = default_params(seed=5, nSubResolutionLevels=2, nEstimationGeometricIters=1)
    g = e.EstimateDepthMap(sc.gray, sc.K, sc.R, sc.C, ids, sc.dmin[4], sc.dmax[4], depth=d, normal=n, src_depths={i: sc.gt_depth[i] for i in ids[1:]}, nGeometricIter=0, params=p)
    print("scene %%dx%%d: one geometric round on top: valid %%.3f" %% (W, H, float((g[0] > 0).mean())), file=sys.stderr)
e.close()
"""


def build():
    from tests import emu
    if emu._clang() is None:
        raise SystemExit("no clang++ to build the emulated library")
    return emu.build("libpmhip_emu.so", defines=["PM_GATHER_CENSUS"], out_name="libpmhip_census.so")


def main(argv):
    geo, widen = "--geo" in argv, "--widen" in argv
    argv = [a for a in argv if a not in ("--geo", "--widen")]
    sizes = [tuple(int(v) for v in a.lower().split("x")) for a in argv] or [(512, 288), (960, 540)]
    lib = build()
    env = dict(os.environ, PMHIP_LIB=lib, OPENMVS_AMD_TEST_EMULATOR="1")
    for w, h in sizes:
        r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, w=w, h=h, geo=int(geo), widen=int(widen))], env=env, stderr=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith(("scene ", "gather census:"))]
        if geo:
            lines = [ln for ln in lines if not ln.startswith("gather census: level")]
        if r.returncode != 0 or len(lines) < 2:
            sys.stderr.write(r.stderr)
            raise SystemExit("the census run of %dx%d failed (exit %d)" % (w, h, r.returncode))
        print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
