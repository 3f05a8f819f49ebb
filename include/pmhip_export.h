/* pmhip_export.h -- the reference's image and PLY outputs from the resident scene (csrc/pm_export.hip), part of the C ABI of libpmhip.so.
 *
 * A companion of include/pmhip.h, which includes it at its end, like pmhip_normals.h and pmhip_mesh.h: pmhip.h's own prototype list is pinned by number
 * (tests/test_abi.py); the Python bindings read every header (openmvs_amd/patchmatch.py).  Conventions, error codes and the engine handle are pmhip.h's.  New functions
 * only: PMHIP_ABI_VERSION stays 7.
 *
 * Every call is blocking and returns host data: an image (3 bytes or 1 byte per pixel) or packed records, never the float maps.  Each result equals its numpy statement
 * in openmvs_amd/mapexport.py bit for bit.  An id outside the scene or a NULL pointer is PMHIP_E_ARG, a view without a depth map (pmhip_scene_maps_updated's notion)
 * PMHIP_E_STATE; the reason is in pmhip_last_error and the engine stays usable.
 *
 * Where the reference's own result is not defined by the language, the engine's is:
 *   - ROUND2INT of a NaN or of a value outside int is INT_MIN, which clamps to 0 (pmfu_round2int / pmfu_toU8 of csrc/pm_fuse.h): a NaN normal component is 0;
 *   - the confidence image's (uint8_t) cast of a NaN -- 0 / 0 when maxConf == minConf and a confidence equals both -- is 0;
 *   - minDepth == maxDepth (one valid depth, or all equal) makes sclDepth infinite: the arithmetic is carried out as IEEE 754 has it, so a depth equal to the range is
 *     0 * inf = NaN, which fails every comparison of gray2color and is black; a nearer depth is gray 1, a farther one gray 0;
 *   - a median of +inf makes |v - median| a NaN for every infinite v; such a NaN ranks above +inf in the second selection. */
#ifndef PMHIP_EXPORT_H_
#define PMHIP_EXPORT_H_
#include "pmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ComputeX84Threshold<float,float> (libs/Common/Util.inl:1001-1024) and GetMinMax (libs/Common/List.h:700) over the values > 0 of a host array (zeros, negatives, -0 and
 * NaN do not count): out = { median, mul * MAD, min, max }, the median being the element at index n/2 of the sorted valid values and the MAD the element at the same index
 * of |v - median| (float).  Exact.  No valid value: PMHIP_E_ARG. */
int pmhip_x84_threshold(pmhip_engine* e, const float* values, uint64_t n, float mul, float out[4]);
/* DepthMap2Image (libs/MVS/DepthMap.cpp:1662-1690) of view idx's resident depth map: rgb gets w*h*3 bytes, red first, at the view's own size.  minDepth == FLT_MAX and
 * maxDepth == 0 ask for the range of the X84 rule (as the reference's defaults do); otherwise the given range is used.  range, if not NULL, gets the range in use:
 * (FLT_MAX, 0) when it was asked for and no depth is valid -- the image is black then. */
int pmhip_scene_depth_image(pmhip_engine* e, int idx, float minDepth, float maxDepth, uint8_t* rgb, float range[2]);
/* The same of a depth map on the host (a rendered mesh, pmhip_mesh_project): depth w*h floats in.  Needs no scene. */
int pmhip_depth_image(pmhip_engine* e, const float* depth, int w, int h, float minDepth, float maxDepth, uint8_t* rgb, float range[2]);
/* The pixel rule of ExportNormalMap (DepthMap.cpp:1700-1715) on view idx's resident normal map: rgb gets w*h*3 bytes, red first. */
int pmhip_scene_normal_image(pmhip_engine* e, int idx, uint8_t* rgb);
/* ExportConfidenceMap (DepthMap.cpp:1721-1749) of view idx's resident confidence map: gray gets w*h bytes, range (if not NULL) minConf and maxConf after the 0.1 / 30
 * floors.  No confidence > 0 (the reference returns false and writes nothing): *empty = 1, gray is all 0, range is not written, and the call returns 0. */
int pmhip_scene_conf_image(pmhip_engine* e, int idx, uint8_t* gray, float range[2], int* empty);
/* MVS::ExportPointCloud (DepthMap.cpp:1753-1870) of view idx: one record per pixel with depth > 0, in row-major order, in the reference's packed vertex layout --
 * float x, y, z, uint8 r, g, b (15 bytes), or with withNormals != 0 float x, y, z, nx, ny, nz, uint8 r, g, b (27 bytes), N = R^T n.  The colour is the view's resident
 * colour image (pmhip_scene_set_color) at the same pixel, white without one.  *count gets the number of records; capacity (in records) too small: PMHIP_E_ARG, *count is
 * the number needed and nothing is written.  records may be NULL when capacity is 0.  The view needs its camera (pmhip_scene_set_view). */
int pmhip_scene_view_cloud(pmhip_engine* e, int idx, int withNormals, void* records, uint64_t capacity, uint64_t* count);
/* The per-point rule of PointCloud::SaveWithScale (libs/MVS/PointCloud.cpp:504-531) on the resident cloud (pmhip_scene_fuse, pmhip_scene_cloud_set / _load) with K, R, C
 * of the scene's views: scale and confidence get one float per point.  A cloud without weights (set or loaded with weights == NULL, or merged with nMinViewsFuse < 2):
 * the smallest Camera::GetFootprintWorld over the point's views and the number of views; with weights: the scale whose scale / weight is smallest and that weight.
 * scale is multiplied by scaleMult.  A point that lists a view without a camera: PMHIP_E_STATE. */
int pmhip_scene_cloud_scale(pmhip_engine* e, float scaleMult, float* scale, float* confidence);
/* out[0] values (pixels) per workgroup and trip of the selection and image kernels, out[1] their grid cap in workgroups, out[2] pixels per scan tile of the view cloud,
 * out[3] kernels launched by the last call above, out[4] the time in microseconds between the HIP events that bracket its kernels and its download, out[5 .. 7] 0. */
int pmhip_export_get_stats(pmhip_engine* e, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PMHIP_EXPORT_H_ */
