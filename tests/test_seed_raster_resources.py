"""The resource figures DESIGN.md section 4.13 quotes for the kernels of the seed rasteriser (csrc/seed_raster.hip), as the compiler reports them for gfx950 (hipcc
cross-compiles: no GPU needed) through tools/kernel_resources.py: scatter and per-pixel kernels that must not spill.  The figures are read from the build of
libsgmhip.so, the smaller of the two libraries that include the file; both compile it with the same flags."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("seed_face_kernel", "seed_large_kernel", "seed_point_kernel", "seed_resolve_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_seed_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    from openmvs_amd import build as _b
    assert _b.LIB_FLAGS["libsgmhip.so"] == _b.LIB_FLAGS["libpmhip.so"]
    seen = kernel_resources.resources(lib="libsgmhip.so")
    kernels = {}
    for mangled, r in seen.items():
        m = re.match(r"_Z(\d+)(seed_\w+)", mangled)                             # _Z<length><name><parameter types>
        if m:
            kernels[m.group(2)[:int(m.group(1))]] = r
    assert sorted(kernels) == sorted(KERNELS), sorted(seen)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.13"):]
    for k, r in kernels.items():
        assert r["scratch"] == 0 and r["lds"] == 0 and r["occupancy"] == 8 and r["vgpr"] <= 64, (k, r)
        assert "| `%s` | %d | %d | %d | %d |" % (k, r["vgpr"], r["sgpr"], r["scratch"], r["occupancy"]) in section, (k, r)      # the figures the document records
