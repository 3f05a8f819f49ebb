"""The SGM modes of `sgm_pipeline.dense_reconstruction` on a scene whose images differ in size (views "may differ in size everywhere"), CPU only,
on the oracle backend: tests/data/scene with image 1 delivered at 3/4 of its size.  Rectification absorbs the difference -- each image has its own homography and
both rectified images share one size -- and everything behind it is per image already.  Bounds: those of tests/test_sgm_real.py::test_sgm_modes_of_dense_reconstruction."""
import os

import numpy as np

from openmvs_amd import dmap, mvsi, optdense, sgm_pipeline
from tests.tsgm_backends import OracleBackend

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "data", "scene")


def test_sgm_modes_on_a_scene_with_images_of_different_sizes(tmp_path):
    from PIL import Image
    mvs = os.path.join(SCENE, "scene.mvs")
    sc = mvsi.load(mvs)
    small = os.path.basename(sc.images[1].name)

    def loader(p):
        with Image.open(p) as im:
            a = np.asarray(im.convert("RGB"))
        if os.path.basename(p) == small:
            H, W = a.shape[:2]
            a = np.asarray(Image.fromarray(a).resize((W * 3 // 4, H * 3 // 4)))
        return a

    opt = optdense.defaults()
    opt.nResolutionLevel = 2; opt.nMinResolution = 80; opt.nNumViews = 2; opt.nEstimateNormals = 2; opt.fViewMinScore = 0.0
    d = str(tmp_path / "sgm")
    be = OracleBackend()
    done = sgm_pipeline.dense_reconstruction(be, mvs, d, -1, opt, image_loader=loader, min_resolution=40)
    assert len(done) == 4 and sorted(os.listdir(d)) == sorted(sgm_pipeline.pair_file_name(a, b) for a, b in done)
    assert any(1 in p for p in done) and not any((b, a) in done for a, b in done)            # the small image takes part, on either side of a pair
    for a, b in done:
        g = dmap.load_dimap(os.path.join(d, sgm_pipeline.pair_file_name(a, b)))
        assert tuple(g["image_size"]) == ((120, 90) if a == 1 else (160, 120))            # the left image's own size
    fused = sgm_pipeline.dense_reconstruction(be, mvs, d, -2, opt, image_loader=loader)
    assert sorted(fused) == [0, 1, 2, 3]
    for i in fused:
        w, h = (120, 90) if i == 1 else (160, 120)
        f = dmap.load(os.path.join(d, "depth%04d.dmap" % i))
        depth, normal, conf = fused[i]
        assert depth.shape == (h, w) and f["depth_map"].shape == (h, w)
        assert np.array_equal(f["depth_map"], depth) and np.array_equal(f["normal_map"], normal) and np.array_equal(f["confidence_map"], conf)
        assert f["depth_min"] == np.float32(1e-4) and f["reference_view_id"] == i
        K, R, C, _, _ = sc.camera(i, (w, h))
        X = sc.vertices.astype(np.float64)
        cx = (X - C) @ R.T
        u = np.rint(K[0, 2] + K[0, 0] * cx[:, 0] / cx[:, 2]).astype(int); v = np.rint(K[1, 2] + K[1, 1] * cx[:, 1] / cx[:, 2]).astype(int)
        m = (cx[:, 2] > 0) & (u >= 0) & (v >= 0) & (u < w) & (v < h)
        dm = depth[v[m], u[m]]; ok = dm > 0
        rel = np.abs(dm[ok] - cx[m][ok, 2]) / cx[m][ok, 2]
        print(i, (w, h), "coverage %.3f  SfM points hit %.3f  median relative error %.4f" % ((depth > 0).mean(), ok.mean(), np.median(rel)))
        assert (depth > 0).mean() > 0.2 and ok.mean() > 0.3 and np.median(rel) < 2e-2, (i, (depth > 0).mean(), ok.mean(), np.median(rel))
