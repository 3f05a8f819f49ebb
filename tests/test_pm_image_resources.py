"""The resource figures DESIGN.md section 4.9 quotes for the kernels of the image store (csrc/pm_image.hip), as the compiler reports them for gfx950 (hipcc
cross-compiles: no GPU needed): memory-bound kernels that must neither spill nor lose residency.  Only pm_image.hip is compiled, with the product's flags."""
import os
import re
import shutil
import subprocess

import pytest

from openmvs_amd import build as _b

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_image_kernels_do_not_spill(tmp_path):
    src = tmp_path / "only_pm_image.hip"
    inst = "".join("template __global__ void pmimg_area_u8_kernel<%d, %d>(PMImgU8);\n" % (m, p) for m in range(4) for p in (1, 4))
    src.write_text('#include "%s"\n%s' % (os.path.join(_b._CSRC, "pm_image.hip"), inst))
    p = subprocess.run([HIPCC] + _b.FLAGS + _b.LIB_FLAGS["libpmhip.so"] + ["-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "x.so")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    seen = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        seen[blk.split("\n")[0].split(" ")[0]] = (g("VGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]"))
    kernels = {k: v for k, v in seen.items() if "pmimg_" in k}
    assert len(kernels) == 8 + 3, sorted(seen)             # four modes x {1, 4} pixels per lane of the 8-bit kernel, and the three ScaleImage kernels
    for k, (vgpr, scratch, occupancy, lds) in kernels.items():
        assert scratch == 0 and lds == 0 and occupancy == 8 and vgpr <= 64, (k, vgpr, scratch, occupancy, lds)
