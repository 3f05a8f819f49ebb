"""`sgm_pipeline.match_scene` builds the seed's mesh once per (image, size) however many pairs an image has, and hands every pair of the image the same mesh (a
backend that seeds on the device) and the depth map rasterised from it (any other).  The matching itself is stubbed: the case is about who triangulates when."""
import os

import numpy as np

from openmvs_amd import densify, mvsi, optdense, sgm_pipeline, views

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "scene", "scene.mvs")


def test_match_scene_triangulates_an_image_once(tmp_path, monkeypatch):
    opt = optdense.defaults()
    opt.nResolutionLevel = 3; opt.nMinResolution = 40; opt.nNumViews = 3; opt.fViewMinScore = 0.0
    sv = densify.load_scene(SCENE, opt=opt)
    sc = mvsi.load(SCENE)
    cams = views.Cameras(sc, sv.sizes[:len(sc.images)])
    nbs = {i: sv.all_view_scores[i] for i in sv.ids}
    built, pairs = [], []
    real = views.triangulate_points

    def counted(K, P, X, w, h, avg_depth=None):
        built.append((w, h, len(X)))
        return real(K, P, X, w, h, avg_depth)
    monkeypatch.setattr(views, "triangulate_points", counted)

    def stub(be, bgrA, camA, bgrB, camB, X, min_resolution=320, subpixel_steps=4, seed_depth=None, image_ids=None, seed_mesh=None):
        assert seed_depth is not None and seed_mesh is not None
        got = []
        for size in ((20, 15), (40, 30), (20, 15)):                              # a size asked twice is built once
            proj, z, faces = seed_mesh(*size)
            depth = seed_depth(*size)
            assert depth.shape == size[::-1] and np.array_equal(depth, views.raster_faces_depth_map(proj, z, faces, *size)) and (depth > 0).all()
            got.append((proj, z, faces, depth))
        assert got[0][0] is got[2][0] and got[0][3] is got[2][3]
        pairs.append(got[0])
        return dict(disparity=np.zeros((2, 3), np.int16), cost=np.zeros((2, 3), np.uint16), H=np.eye(3), Q=np.eye(4), image_size=(bgrA.shape[1], bgrA.shape[0]), subpixel_steps=subpixel_steps)
    monkeypatch.setattr(sgm_pipeline, "match_pair", stub)
    done = sgm_pipeline.match_scene(object(), sc, cams, sv.bgr, nbs, str(tmp_path), n_views=3, f_min_score=0.0, min_resolution=40, avg_depth=sv.avg_depth)
    images = sorted({i for i, _ in done})
    assert len(done) > len(images) >= 3, done                                    # some image has several pairs
    assert len(built) == 2 * len(images), (built, done)                          # two sizes per image, whatever its number of pairs
    first = {}
    for (i, j), mesh in zip(done, pairs):
        if i in first:
            assert all(a is b for a, b in zip(mesh, first[i])), "the pairs of image %d share one mesh and one map" % i
        first.setdefault(i, mesh)
