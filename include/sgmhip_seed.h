/* sgmhip_seed.h -- the tSGM loop's seed made and kept on the device: the rough depth map of an image's sparse points rasterised from their mesh
 * (csrc/seed_raster.hip), converted to the first level's initial disparities and consumed by the loop without crossing to the host.  Part of the C ABI of libsgmhip.so.
 *
 * A companion of include/sgmhip.h, which includes it at its end, exactly as sgmhip_plain.h is: a host that includes sgmhip.h has these functions, and this header may
 * also be included on its own.  They are declared here and not in sgmhip.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the
 * Python bindings read every companion header (openmvs_amd/sgm.py).  Conventions, error codes and the engine handle are sgmhip.h's.
 *
 * The three steps replace TriangulatePoints2DepthMap (depth only, libs/MVS/DepthMap.cpp:1225-1249) on the host, sgmhip_depth2disparity_map and the
 * initLeftDisparity argument of sgmhip_tsgm_match_rectified; each gives the same bits as the step it replaces. */
#ifndef SGMHIP_SEED_H_
#define SGMHIP_SEED_H_
#include "sgmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The faces of a point mesh (proj 2 * nVerts floats, z nVerts depths, faces 3 * nFaces vertex indices: mvsf_point_mesh, include/mvsfront_mesh.h) rasterised in the
 * order given into a w x h depth map, as pmhip_seed_raster does in its faces mode without normals (include/pmhip_seed.h: a later face overwrites an earlier one; 0
 * where no face is).  The map stays resident as the engine's seed and is also written to depthOut (w * h floats) when that is not NULL.  nVerts == 0 or nFaces == 0
 * gives an all-zero seed.  SGMHIP_E_ARG with the reason in sgmhip_last_error, the engine staying usable and the seed held before staying: w or h < 1, more than
 * INT_MAX pixels, a NULL array with a non-zero count, a face index >= nVerts, a non-finite coordinate or depth, a depth <= 0, a coordinate whose floor or ceil
 * leaves int.  Blocking. */
int sgmhip_seed_raster(sgmhip_engine* e, int w, int h, const float* proj, const float* z, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces, float* depthOut);
/* sgmhip_depth2disparity_map on the resident seed: a w x h disparity map from the seed depth map through invH (9 doubles) and invQ (16 doubles).  The result stays
 * resident as the initial left disparity of sgmhip_tsgm_match_rectified_seeded and is also written to disparityOut (w * h values) when that is not NULL.
 * SGMHIP_E_ARG without a seed, with a NULL matrix or w or h < 1.  Blocking. */
int sgmhip_seed_disparity(sgmhip_engine* e, const double invH[9], const double invQ[16], int subpixelSteps, int w, int h, int16_t* disparityOut);
/* sgmhip_tsgm_match_rectified with the resident initial disparity in the place of its host pointer.  For plain SGM (minResolution == 0) the seed's values are brought
 * back for sgmhip_plain_range: the range, the errors and the messages are those of sgmhip_tsgm_match_rectified.  A missing seed disparity, or one whose size is not
 * that of the first level's seed grid, is SGMHIP_E_ARG. */
int sgmhip_tsgm_match_rectified_seeded(sgmhip_engine* e, unsigned minResolution, int nSpeckleSize, int subpixelMode, int subpixelSteps,
                                       uint16_t P1, const uint16_t P2s[256], int16_t* disparity, uint16_t* cost, int* numLevels);
/* Frees the seed, its disparity and the rasteriser's working buffers; sgmhip_scene_clear and sgmhip_destroy do the same. */
int sgmhip_seed_clear(sgmhip_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* SGMHIP_SEED_H_ */
