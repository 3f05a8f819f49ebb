"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/pmhip.h declares,
and fails loudly (no CPU fallback) without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b((?:pmhip|sgmhip|mvsf|dmap|dimap)_[a-z_0-9]+)\s*\(", src)))


def test_pmhip_exports_every_declared_symbol():
    from openmvs_amd import patchmatch
    lib = patchmatch.load_library()
    names = _declared("pmhip.h")
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(patchmatch.EXPORTS) == names


def test_sgmhip_exports_every_declared_symbol():
    from openmvs_amd import sgm
    lib = sgm.load_library()
    names = _declared("sgmhip.h")
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(sgm.EXPORTS) == names
    assert sgm.PIXEL_DTYPE.itemsize == 16 and C.sizeof(sgm.SGMHipStats) == 40
    # GenerateP2s needs no GPU: P2*(1+alpha) .. P2
    p = sgm.generate_p2s()
    assert p[0] == 60 and p[255] == 4


def test_struct_sizes_match_header():
    from openmvs_amd import patchmatch as pm
    assert C.sizeof(pm.PMHipParams) == 4 * 4 + 9 * 4 + 4
    assert C.sizeof(pm.PMHipView) == 8 + 8 + 21 * 8 + 8 + 21 * 8 + 16   # id, dw, dh + 4 bytes of tail padding
    assert C.sizeof(pm.PMHipKernelStats) == 64 and C.sizeof(pm.PMHipTuning) == 8 * 4


def _bindings():
    from openmvs_amd import dmap, mvsfront, optdense, patchmatch, sgm
    return {"pmhip.h": patchmatch, "sgmhip.h": sgm, "mvsfront.h": mvsfront, "optdense.h": optdense, "dmapio.h": dmap}


def test_the_header_reader_drops_no_prototype():
    """Every name the headers declare (by the name regex above, which knows nothing of types) has a parsed signature, and EXPORTS is that list."""
    from openmvs_amd import _cabi
    counts = {}
    for header, module in _bindings().items():
        sigs = _cabi.signatures(header, module._TYPES)
        assert sorted(sigs) == _declared(header) == sorted(module.EXPORTS), header
        counts[header] = len(sigs)
    assert counts == {"pmhip.h": 65, "sgmhip.h": 33, "mvsfront.h": 20, "optdense.h": 9, "dmapio.h": 5}


def test_an_unknown_type_spelling_is_an_error_that_names_the_function():
    from openmvs_amd import _cabi
    with pytest.raises(TypeError, match=r"sgmhip_set_problem.*SGMHipPixelData"):
        _cabi.signatures("sgmhip.h", {})              # without the binding module's mirrors the struct is an unknown spelling


def test_signatures_pinned_by_hand():
    """Types a default ctypes call would get wrong, written out here so that the reader is not only checked against itself."""
    from openmvs_amd import patchmatch, sgm
    lib = patchmatch.load_library()
    assert lib.pmhip_scene_cloud_set.argtypes[-1] is C.c_uint64
    assert lib.pmhip_math_eval.argtypes[-1] is C.c_size_t
    assert lib.pmhip_scaled_size.argtypes[2] is C.c_float
    dev = lib.pmhip_scene_copy.argtypes[4].from_param((1 << 40) + 8)          # a device address above 2^32 arrives whole
    assert isinstance(dev, C.c_void_p) and dev.value == (1 << 40) + 8
    for f in (lib.pmhip_scene_bytes, lib.pmhip_image_bytes, lib.pmhip_scene_fuse_rounds):
        assert f.restype is C.c_uint64
    assert lib.pmhip_last_error.restype is C.c_char_p
    assert lib.pmhip_destroy.restype is None
    assert lib.pmhip_stream.restype is C.c_void_p
    assert len(sgm.load_library().sgmhip_tsgm_match.argtypes) == 19


def test_bad_arrays_are_refused_before_the_call():
    from openmvs_amd import patchmatch, sgm
    lib = sgm.load_library()
    read_only = np.zeros(256, np.uint16); read_only.flags.writeable = False
    for bad in (np.zeros(256, np.float32), np.zeros(512, np.uint16)[::2], read_only):
        with pytest.raises(C.ArgumentError):
            lib.sgmhip_generate_p2s(4, 14.0, 38.0, bad)
    p = np.zeros(256, np.uint16)
    assert lib.sgmhip_generate_p2s(4, 14.0, 38.0, p) == 0 and p[0] == 60 and p[255] == 4
    assert lib.sgmhip_generate_p2s(np.int64(4), np.float32(14.0), 38, p) == 0 and p[0] == 60 and p[255] == 4          # numpy scalars and an int for a float
    depth = patchmatch.load_library().pmhip_scene_set_maps.argtypes[2]          # const float*
    assert depth.from_param(None) is None
    assert depth.from_param(read_only.view(np.float32)).value == read_only.ctypes.data         # const: a read-only array will do
    with pytest.raises(TypeError):
        depth.from_param(np.zeros(4, np.float64))


def _layout(name, mirror):
    """(size, {field: (offset, size)}) of a struct mirror: a C.Structure class or a numpy dtype."""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, {f: (off, t.itemsize) for f, (t, off) in mirror.fields.items()}
    return C.sizeof(mirror), {f: (getattr(mirror, f).offset, getattr(mirror, f).size) for f, _ in mirror._fields_}


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    """sizeof and every field's offsetof / sizeof, printed by a program the host compiler builds from the five headers, against the ctypes and numpy
    mirrors.  A field the header lacks fails the build; a field the mirror lacks shows as a size mismatch."""
    mirrors = {}
    for module in _bindings().values():
        mirrors.update(module._TYPES)
    assert len(mirrors) == 15
    src = ["#include <cstddef>", "#include <cstdio>"] + ['#include "%s"' % h for h in _bindings()] + ["int main() {"]
    for name, mirror in mirrors.items():
        src.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in _layout(name, mirror)[1]:
            src.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f))
    src.append("    return 0;\n}")
    (tmp_path / "layout.cpp").write_text("\n".join(src) + "\n")
    cxx = shutil.which("g++")            # the compiler openmvs_amd.build makes the host libraries with
    assert cxx, "no host compiler"
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", str(tmp_path / "layout")])
    got = {}
    for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines():
        key, *numbers = line.split()
        got[key] = tuple(int(v) for v in numbers)
    for name, mirror in mirrors.items():
        size, fields = _layout(name, mirror)
        assert got[name] == (size,), name
        for f, where in fields.items():
            assert got["%s.%s" % (name, f)] == where, (name, f)


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from openmvs_amd.patchmatch import PatchMatchError, PatchMatchHIP
    with pytest.raises(PatchMatchError):
        PatchMatchHIP(0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "openmvs_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                s = open(os.path.join(dp, f), errors="ignore").read()
                assert "pyoracle" not in s and "pm_oracle" not in s.replace("oracle/pm_oracle.cpp", "") and "libpm_oracle" not in s, f


def test_the_libraries_read_no_environment_variable():
    """Every route of the engines is chosen by the input or through the ABI (pmhip_set_tuning, sgmhip_set_sub_group_kernels): a switch read from the
    environment is one no test of this suite can flip inside its process."""
    for d in (os.path.join(ROOT, "openmvs_amd", "csrc"), os.path.join(ROOT, "include")):
        for dp, _, fs in os.walk(d):
            for f in fs:
                assert "getenv" not in open(os.path.join(dp, f), errors="ignore").read(), os.path.join(dp, f)
