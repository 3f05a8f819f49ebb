"""The companion headers of the device seed (include/pmhip_seed.h, include/sgmhip_seed.h, include/mvsfront_mesh.h): each parses with the header reader of the bindings,
every name it declares is exported by its library and bound, each main header includes its companion at its end, and the main headers' pinned prototype counts
(tests/test_abi.py) are what they were."""
import ctypes as C
import os
import re

from openmvs_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b((?:pmhip|sgmhip|mvsf)_[a-z_0-9]+)\s*\(", src)))


def _check(header, main, module, exports, expected):
    sigs = _cabi.signatures(header, module._TYPES)
    assert sorted(sigs) == _declared(header) == sorted(exports) == sorted(expected), header
    lib = module.load_library()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                                                  # exported ...
        assert fn.restype is res and list(fn.argtypes) == args, name             # ... and declared to ctypes from the header
    text = open(os.path.join(ROOT, "include", main)).read()
    assert text.rstrip().splitlines()[-1].startswith("#endif") and text.index('#include "%s"' % header) > text.rindex("}"), "%s includes %s at its end" % (main, header)
    return sigs


def test_pmhip_seed_header():
    from openmvs_amd import patchmatch
    sigs = _check("pmhip_seed.h", "pmhip.h", patchmatch, patchmatch.SEED_EXPORTS, ["pmhip_seed_raster", "pmhip_scene_seed_view", "pmhip_seed_set_tuning", "pmhip_seed_get_stats"])
    assert len(sigs["pmhip_seed_raster"][1]) == 12 and len(sigs["pmhip_scene_seed_view"][1]) == 9 and len(sigs["pmhip_seed_set_tuning"][1]) == 2
    assert sigs["pmhip_seed_raster"][1][0] is C.c_void_p and sigs["pmhip_seed_raster"][1][7] is C.c_uint32 and sigs["pmhip_seed_get_stats"][1][1].dtype == "uint64"
    assert (patchmatch.SEED_POINTS, patchmatch.SEED_FACES) == (0, 1) and "PMHIP_SEED_POINTS = 0, PMHIP_SEED_FACES = 1" in open(os.path.join(ROOT, "include", "pmhip_seed.h")).read()
    assert patchmatch.PMHIP_ABI_VERSION == 7 and patchmatch.load_library().pmhip_abi_version() == 7          # new functions only


def test_sgmhip_seed_header():
    from openmvs_amd import sgm
    sigs = _check("sgmhip_seed.h", "sgmhip.h", sgm, sgm.SEED_EXPORTS, ["sgmhip_seed_raster", "sgmhip_seed_disparity", "sgmhip_tsgm_match_rectified_seeded", "sgmhip_seed_clear"])
    assert len(sigs["sgmhip_seed_raster"][1]) == 9 and len(sigs["sgmhip_seed_disparity"][1]) == 7 and len(sigs["sgmhip_tsgm_match_rectified_seeded"][1]) == 10
    assert len(sgm.load_library().sgmhip_tsgm_match_rectified.argtypes) == 11                               # the seeded form is that call less its host pointer


def test_mvsfront_mesh_header():
    from openmvs_amd import mvsfront
    sigs = _check("mvsfront_mesh.h", "mvsfront.h", mvsfront, mvsfront.MESH_EXPORTS, ["mvsf_point_mesh"])
    assert len(sigs["mvsf_point_mesh"][1]) == 18


def test_the_main_headers_keep_their_pinned_counts():
    from openmvs_amd import mvsfront, patchmatch, sgm
    counts = {h: len(_cabi.signatures(h, m._TYPES)) for h, m in (("pmhip.h", patchmatch), ("sgmhip.h", sgm), ("mvsfront.h", mvsfront))}
    assert counts == {"pmhip.h": 65, "sgmhip.h": 33, "mvsfront.h": 20}
