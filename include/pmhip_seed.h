/* pmhip_seed.h -- the rough depth and normal maps of an image's sparse points rasterised on the device (csrc/seed_raster.hip), part of the C ABI of libpmhip.so.
 *
 * A companion of include/pmhip.h, which includes it at its end, exactly as pmhip_mesh.h is: a host that includes pmhip.h has these functions, and this header may
 * also be included on its own.  They are declared here and not in pmhip.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the
 * Python bindings read every companion header (openmvs_amd/patchmatch.py).  Conventions, error codes and the engine handle are pmhip.h's.  New functions only:
 * PMHIP_ABI_VERSION stays 7.
 *
 * What is computed is the map part of TriangulatePoints2DepthMap (libs/MVS/DepthMap.cpp:1117-1251) bit for bit from the point mesh the host triangulated
 * (mvsf_point_mesh, include/mvsfront_mesh.h): proj 2 * nVerts floats (pixel coordinates), z nVerts floats (camera-space depths), normals 3 * nVerts floats or NULL
 * (depth only), faces 3 * nFaces vertex indices.
 *   PMHIP_SEED_FACES   the maps are zeroed and the faces drawn in the order given (TImage::RasterizeTriangleBary with the RasterDepth functor): a face is rejected
 *                      when its box misses the image or its area is <= 0; every pixel of the clipped box floor(min) .. ceil(max) whose three barycentrics are >= 0
 *                      receives the perspective-correct depth and the normalised interpolated normal.  A later face overwrites an earlier one, so a pixel holds
 *                      the values of the highest-numbered face that covers it.
 *   PMHIP_SEED_POINTS  vertex i writes z[i] and normals[i] to the pixels floor(proj[i]) + {(0,0),(1,0),(0,1),(1,1)} inside the image; a later vertex overwrites an
 *                      earlier one.  faces are not read.
 * nVerts == 0 or, with PMHIP_SEED_FACES, nFaces == 0 gives all-zero maps and is no error.
 * PMHIP_E_ARG, with the reason in pmhip_last_error and the engine staying usable: an unknown mode, w or h < 1, more than INT_MAX pixels, a NULL array with a non-zero
 * count, a face index >= nVerts, a non-finite coordinate or depth, a depth <= 0 (the reference asserts z > 0), a coordinate whose floor or ceil leaves int.  Everything
 * is checked before anything is uploaded or written. */
#ifndef PMHIP_SEED_H_
#define PMHIP_SEED_H_
#include "pmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PMHIP_SEED_POINTS = 0, PMHIP_SEED_FACES = 1 };

/* Host arrays in, host arrays out, blocking; needs no scene.  depthOut receives w * h floats; normalOut 3 * w * h floats, or NULL.  With normals == NULL a normalOut
 * is left as it is. */
int pmhip_seed_raster(pmhip_engine* e, int mode, int w, int h, const float* proj, const float* z, const float* normals, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces,
                      float* depthOut, float* normalOut);
/* The same maps written into the resident depth and normal map of scene view `view`, at that view's own size: the scene is left exactly as pmhip_scene_set_maps(view,
 * depth, normal) would leave it with the maps of pmhip_seed_raster; with normals == NULL as that call does with a NULL normal map (the resident normal map stays).
 * Only the mesh crosses to the device.  Blocking.  A view outside the scene is PMHIP_E_ARG. */
int pmhip_scene_seed_view(pmhip_engine* e, int view, int mode, const float* proj, const float* z, const float* normals, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces);
/* How the faces are mapped; the maps never depend on it.  boxPixels: a face whose clipped bounding box holds more pixels than this is rasterised by a workgroup
 * instead of one lane (> 0; 0 keeps the value, < 0 restores the default). */
int pmhip_seed_set_tuning(pmhip_engine* e, int boxPixels);
/* Four numbers.  out[0] faces the last call gave to the workgroup route, out[1] boxPixels in force, out[2] microseconds the device spent on the last call's clears
 * and kernels (HIP events; uploads and downloads not included), out[3] bytes of mesh the last call uploaded. */
int pmhip_seed_get_stats(pmhip_engine* e, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PMHIP_SEED_H_ */
