"""The image and PLY outputs of csrc/pm_export.hip on the CPU: the product's sources compiled against the wave64 emulator (tests/emu.py), every entry point of
include/pmhip_export.h on the cases of tests/map_export_cases.py against the numpy statements of openmvs_amd/mapexport.py, bit for bit; the kernel cases again with
lanes and workgroups executed in reverse; the PLY and PNG writers against bytes written out by hand; then the routes that use them: `densify.dense_reconstruction` with
`export_level=5` and `ply_out`, and `export_mesh_depth_maps` to a PNG.  The cases are those of tests/test_zz_gpu_map_export.py."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from openmvs_amd import mapexport as mx
from openmvs_amd import patchmatch, plyio
from tests import emu
from tests import map_export_cases as cases

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


@pytest.fixture(scope="module")
def emulated():
    with emu.emulated(patchmatch, "PMHIP_LIB", "libpmhip_emu.so"):
        yield lambda: patchmatch.PatchMatchHIP(0)


@pytest.fixture(scope="module")
def engine(emulated):
    e = emulated()
    yield e
    e.close()


def test_the_emulated_library_exports_every_entry_point(emulated):
    import ctypes as C
    import re
    lib = patchmatch.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pmhip_export.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(pmhip_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted(patchmatch.EXPORT_EXPORTS) and len(names) == 8 and "pmhip_scene_cloud_scale" in names
    assert all(hasattr(lib, n) and getattr(lib, n).argtypes is not None and getattr(lib, n).restype is C.c_int for n in names) and hasattr(lib, "hipemu_counters")
    assert '#include "pmhip_export.h"' in open(os.path.join(root, "include", "pmhip.h")).read()
    assert len(lib.pmhip_scene_view_cloud.argtypes) == 6 and lib.pmhip_scene_view_cloud.argtypes[0] is C.c_void_p and lib.pmhip_scene_view_cloud.argtypes[4] is C.c_uint64
    assert len(lib.pmhip_depth_image.argtypes) == 8 and lib.pmhip_depth_image.argtypes[4] is C.c_float


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65])
def test_kernel_selection_small_counts(engine, n):
    cases.count_case(engine, n)


def test_kernel_selection_counts_around_the_quantum(engine):
    for n in cases.quantum_counts(engine):
        cases.count_case(engine, n)


def test_kernel_selection_past_the_grid_cap(engine):
    cases.past_the_grid_cap(engine)


def test_kernel_selection_value_patterns(engine):
    cases.pattern_cases(engine)


def test_kernel_selection_infinite_median_is_pinned(engine):
    cases.infinite_median_is_pinned(engine)


def test_kernel_selection_without_a_valid_value(engine):
    cases.no_valid_value(engine, patchmatch.PatchMatchError)


@pytest.mark.parametrize("h,w", cases.COLOUR_SIZES)
def test_kernel_colour_map(engine, h, w):
    cases.colour_map_case(engine, h, w)


def test_kernel_colour_map_without_a_valid_pixel(engine):
    cases.no_valid_pixel(engine)


def test_kernel_colour_map_equal_range_is_pinned(engine):
    cases.equal_range_is_pinned(engine)


def test_kernel_normal_image(engine):
    cases.normal_image_cases(engine)


def test_kernel_confidence_image(engine):
    cases.conf_image_cases(engine)


def test_kernel_confidence_image_equal_range_is_pinned(engine):
    cases.equal_confidence_is_pinned(engine)


@pytest.mark.parametrize("w", cases.CLOUD_WIDTHS)
def test_kernel_view_cloud(engine, w):
    cases.view_cloud_case(engine, w, patchmatch.PatchMatchError)


def test_kernel_view_cloud_without_a_valid_pixel(engine, tmp_path):
    cases.empty_view_cloud(engine, tmp_path)


def test_kernel_point_scales(engine):
    cases.scale_cases(engine)
    cases.scale_tie_case(engine)


def test_refusals_leave_the_engine_usable(engine):
    cases.error_cases(engine, patchmatch.PatchMatchError)
    cases.scale_needs_a_cloud_and_cameras(engine, patchmatch.PatchMatchError)


@pytest.mark.parametrize("order", ["reverse"])
def test_kernel_results_do_not_depend_on_the_execution_order(order):
    """Every kernel case again with the lanes of every workgroup and the workgroups of every grid executed in reverse (HIPEMU_ORDER): the histogram's atomics are integer
    sums and every other output has one writer, so the bits must not move."""
    if os.environ.get("HIPEMU_ORDER"):
        pytest.skip("already inside a permuted run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_kernel_ and not execution_order"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPEMU_ORDER=order), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


# ---- the writers (host only) -----------------------------------------------------------------------------------------------------------------------------------
def _cloud():
    return dict(nPoints=2, points=np.array([[1, 2, 3], [4, 5, 6]], np.float32), viewStart=np.array([0, 2, 3], np.uint32), views=np.array([0, 3, 1], np.uint32),
                weights=np.array([0.5, 2.0, 1.5], np.float32), colors=np.array([[10, 20, 30], [40, 50, 60]], np.uint8), normals=np.array([[0, 0, -1], [0, 1, 0]], np.float32))


HEAD = b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
XYZ = b"property float32 x\nproperty float32 y\nproperty float32 z\n"
RGB = b"property uint8 red\nproperty uint8 green\nproperty uint8 blue\n"
NRM = b"property float32 nx\nproperty float32 ny\nproperty float32 nz\n"
END = b"end_header\n"


def test_save_point_cloud_plain(tmp_path):
    p = str(tmp_path / "a" / "plain.ply")                                 # (the folder is made, Util::ensureFolder)
    c = dict(_cloud(), colors=None, normals=None)
    assert plyio.save_point_cloud(p, c, views=False) is True
    assert open(p, "rb").read() == HEAD % 2 + XYZ + END + struct.pack("<3f", 1, 2, 3) + struct.pack("<3f", 4, 5, 6)
    assert plyio.save_point_cloud(str(tmp_path / "none.ply"), dict(c, nPoints=0, points=np.zeros((0, 3), np.float32), viewStart=np.zeros(1, np.uint32))) is False
    assert not os.path.exists(str(tmp_path / "none.ply"))


def test_save_point_cloud_with_views_and_weights(tmp_path):
    p = str(tmp_path / "views.ply")
    assert plyio.save_point_cloud(p, _cloud())
    want = (HEAD % 2 + XYZ + RGB + NRM + b"property list uint8 uint32 view_indices\nproperty list uint8 float32 view_weights\n" + END
            + struct.pack("<3f3B3f", 1, 2, 3, 30, 20, 10, 0, 0, -1) + struct.pack("<B2I", 2, 0, 3) + struct.pack("<B2f", 2, 0.5, 2.0)
            + struct.pack("<3f3B3f", 4, 5, 6, 60, 50, 40, 0, 1, 0) + struct.pack("<BI", 1, 1) + struct.pack("<Bf", 1, 1.5))
    assert open(p, "rb").read() == want
    assert plyio.save_point_cloud(p, dict(_cloud(), weights=None))        # a cloud without weights: the indices only
    assert b"view_indices" in open(p, "rb").read() and b"view_weights" not in open(p, "rb").read()
    back = plyio.load_point_cloud(p)
    assert back["view_indices"][0].tolist() == [2, 1] and back["view_indices"][1].tolist() == [0, 3, 1] and back["red"].tolist() == [30, 60]


def test_save_point_cloud_min_views(tmp_path):
    p = str(tmp_path / "two.ply")
    assert plyio.save_point_cloud(p, _cloud(), min_views=2)
    assert open(p, "rb").read() == HEAD % 1 + XYZ + RGB + NRM + END + struct.pack("<3f3B3f", 1, 2, 3, 30, 20, 10, 0, 0, -1)
    assert plyio.save_point_cloud(p, dict(_cloud(), colors=None, normals=None), min_views=1)          # white without colours
    assert open(p, "rb").read() == HEAD % 2 + XYZ + RGB + END + struct.pack("<3f3B", 1, 2, 3, 255, 255, 255) + struct.pack("<3f3B", 4, 5, 6, 255, 255, 255)
    assert plyio.save_point_cloud(str(tmp_path / "three.ply"), _cloud(), min_views=3) is False and not os.path.exists(str(tmp_path / "three.ply"))


def test_save_point_cloud_with_scales(tmp_path):
    p = str(tmp_path / "scale.ply")
    assert plyio.save_point_cloud(p, _cloud(), scales=(np.array([0.25, 0.5], np.float32), np.array([2.0, 1.5], np.float32)))
    want = (HEAD % 2 + XYZ + RGB + NRM + b"property float32 confidence\nproperty float32 value\n" + END
            + struct.pack("<3f3B3f2f", 1, 2, 3, 30, 20, 10, 0, 0, -1, 2.0, 0.25) + struct.pack("<3f3B3f2f", 4, 5, 6, 60, 50, 40, 0, 1, 0, 1.5, 0.5))
    assert open(p, "rb").read() == want


def test_save_view_cloud_both_layouts(tmp_path):
    K = np.array([[10.0, 0, 1], [0, 10.0, 1], [0, 0, 1]]); R = np.eye(3); C = np.zeros(3)
    d = np.array([[0, 2.0], [4.0, 0]], np.float32)
    n = np.zeros((2, 2, 3), np.float32); n[..., 2] = -1
    bgr = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    rec = mx.view_point_cloud(K, R, C, d, n, bgr)
    p = str(tmp_path / "n.ply")
    assert plyio.save_view_cloud(p, rec, True)
    want = HEAD % 2 + XYZ + NRM + RGB + END + struct.pack("<6f3B", 0, -0.2, 2, 0, 0, -1, 5, 4, 3) + struct.pack("<6f3B", -0.4, 0, 4, 0, 0, -1, 8, 7, 6)
    assert open(p, "rb").read() == want
    rec = mx.view_point_cloud(K, R, C, d, None, None)
    assert plyio.save_view_cloud(p, rec, False)
    assert open(p, "rb").read() == HEAD % 2 + XYZ + RGB + END + struct.pack("<3f3B", 0, -0.2, 2, 255, 255, 255) + struct.pack("<3f3B", -0.4, 0, 4, 255, 255, 255)
    assert plyio.save_view_cloud(p, rec.view(np.uint8), False) and len(open(p, "rb").read()) == len(HEAD % 2 + XYZ + RGB + END) + 30       # raw bytes are taken as records


def test_pngs_reread_to_the_twins_arrays(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    d = rng.uniform(0, 5, (9, 14)).astype(np.float32); d[d < 1] = 0
    rgb = mx.depth_map_to_image(d)[0]
    gray = mx.conf_map_to_image(d)[0]
    mx.save_image(str(tmp_path / "d.png"), rgb); mx.save_image(str(tmp_path / "c.png"), gray)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "d.png"))), rgb) and np.array_equal(np.asarray(Image.open(str(tmp_path / "c.png"))), gray)
    assert Image.open(str(tmp_path / "d.png")).mode == "RGB" and Image.open(str(tmp_path / "c.png")).mode == "L"


def test_twins_on_values_worked_by_hand():
    v = np.array([3.0, 0.0, 1.0, -2.0, 2.0, np.nan, 10.0], np.float32)       # valid 1 2 3 10: index 2 is 3; |v - 3| = 0 2 1 7 -> sorted 0 1 2 7, index 2 is 2
    assert mx.x84_threshold(v) == (3.0, np.float32(5.2) * np.float32(2), 1.0, 10.0)
    assert mx.x84_threshold(np.zeros(4, np.float32)) is None
    K = np.array([[100.0, 0, 5], [0, 100.0, 5], [0, 0, 1]])
    s = mx.footprint_world(K, np.eye(3), np.zeros(3), np.array([[0.0, 0.0, 4.0]]))          # x = (0, 0): 4 / sqrt(100^2 + 5^2 + 5^2)
    assert s[0] == 4.0 / np.sqrt(100.0 * 100.0 + (25.0 + 25.0))


# ---- the routes ----------------------------------------------------------------------------------------------------------------------------------------------
def test_dense_reconstruction_writes_the_verbose_files_and_the_ply(emulated, tmp_path):
    e = emulated()
    try:
        cases.dense_reconstruction_case(e, SCENE, tmp_path)
    finally:
        e.close()


def test_export_mesh_depth_maps_writes_colour_mapped_pngs(emulated, tmp_path):
    e = emulated()
    try:
        cases.mesh_png_case(e, SCENE, tmp_path)
    finally:
        e.close()


def test_export_archive_clouds(emulated, tmp_path):
    """`--export-number-views` and `--estimate-scale` on an existing dense archive: `_Nviews.ply` holds the points with that many views, `_scale.ply` the scales of
    `mapexport.point_scales` with the archive's cameras and its weights."""
    from openmvs_amd import densify, mvsi
    e = emulated()
    try:
        dense = str(tmp_path / "scene_dense.mvs")
        _, cloud = densify.dense_reconstruction(e, SCENE, dense, cases.route_options(), seed=3)
        base = str(tmp_path / "out")
        assert densify.dense_reconstruction(e, dense, None, ply_out=base, export_number_views=3, estimate_scale=1.7) == (None, None)
    finally:
        e.close()
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("out")) == ["out_3views.ply", "out_scale.ply"]
    cnt = np.diff(cloud["viewStart"].astype(np.int64))
    nv = plyio.load_point_cloud(base + "_3views.ply")
    assert 0 < len(nv["x"]) == int((cnt >= 3).sum()) < cloud["nPoints"]
    cases.same_bits(nv["x"], cloud["points"][cnt >= 3, 0], "_3views.ply")
    sc = mvsi.load(dense)
    cams = [sc.camera(i) for i in range(len(sc.images))]
    want = mx.point_scales(cloud["points"], cloud["viewStart"], cloud["views"], cloud["weights"], [c[0] for c in cams], [c[1] for c in cams], [c[2] for c in cams], 1.7)
    got = plyio.load_point_cloud(base + "_scale.ply")
    cases.same_bits(got["value"], want[0], "_scale.ply scales"); cases.same_bits(got["confidence"], want[1], "_scale.ply confidences")
    assert list(got)[-2:] == ["confidence", "value"] and "view_indices" not in got and (want[0] > 0).all()
