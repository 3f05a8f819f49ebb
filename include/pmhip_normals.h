/* pmhip_normals.h -- normal maps from depth maps alone (csrc/pm_normal.hip), part of the C ABI of libpmhip.so.
 *
 * A companion of include/pmhip.h, which includes it at its end: a host that includes pmhip.h has these two functions, and this header may also be included on its
 * own.  They are declared here and not in pmhip.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the Python bindings read
 * both headers (openmvs_amd/patchmatch.py).  Conventions, error codes and the engine handle are pmhip.h's.  New functions only: PMHIP_ABI_VERSION stays 7. */
#ifndef PMHIP_NORMALS_H_
#define PMHIP_NORMALS_H_
#include "pmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MVS::EstimateNormalMap (libs/MVS/DepthMap.cpp:1522-1613) for these views, on the device: the normal map of each becomes EstimateNormalMap(its K, its resident
 * depth map), in place, at the view's own size; depth and confidence are not touched.  What the reference does for a depth map that comes without normals: a .dmap
 * stored without them (DepthMapsData::InitViews, SceneDensify.cpp:411-414), FuseDepthMaps (:1426-1427), and every image of --fusion-mode -2 (:2053-2055).  Bit for bit
 * mvsf_estimate_normal_map (include/mvsfront.h).  Asynchronous on the engine stream, like the per-map filters' kernels.  nViews == 0 is a no-op.  An id outside the
 * scene is PMHIP_E_ARG, a view without a camera or without a depth map (pmhip_scene_maps_updated's notion) PMHIP_E_STATE: the reason is in pmhip_last_error, nothing
 * was launched, and the engine stays usable. */
int pmhip_scene_estimate_normals(pmhip_engine* e, const int32_t* viewIds, int nViews);
/* The same on host buffers, without a scene: depth w*h floats in, normal w*h*3 floats out (every pixel is written).  Blocking.  For a host that resumes .dmap files
 * one by one; w <= 0, h <= 0 or a NULL pointer is PMHIP_E_ARG. */
int pmhip_estimate_normal_map(pmhip_engine* e, const double K[9], const float* depth, int w, int h, float* normal);

#ifdef __cplusplus
}
#endif
#endif /* PMHIP_NORMALS_H_ */
