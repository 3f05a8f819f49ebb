/* mvsfront_mesh.h -- the point mesh behind the sparse depth initialisation, part of the C ABI of libmvsfront.so.
 *
 * A companion of include/mvsfront.h, which includes it at its end: a host that includes mvsfront.h has this function, and this header may also be included on its own.
 * It is declared here and not in mvsfront.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the Python binding reads the companion
 * header too (openmvs_amd/mvsfront.py).  Conventions and error codes are mvsfront.h's. */
#ifndef MVSFRONT_MESH_H_
#define MVSFRONT_MESH_H_
#include "mvsfront.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mesh that mvsf_init_depth_map / mvsf_init_depth_map_dense (addCorners = 0) and mvsf_triangulate_depth_map rasterise, before they do: TriangulatePointsDelaunay of
 * the sparse points `points` in image idx at w x h (libs/MVS/DepthMap.cpp:1019-1115) -- what pmhip_scene_seed_view / pmhip_seed_raster (include/pmhip_seed.h) and
 * sgmhip_seed_raster (include/sgmhip_seed.h) take, so that a host hands the device a few thousand vertices instead of whole maps.
 *   proj     2 floats per vertex: the pixel coordinates
 *   z        1 float per vertex: the camera-space depth
 *   normals  3 floats per vertex, or NULL: Mesh::ComputeNormalVertices of the mesh (the area-weighted normals the initial normal map is made of), their float sums
 *            in the order of openmvs_amd.views.point_mesh (the faces' first corners, then their second, then their third), so that a C++ host seeds the device with
 *            the bits the Python front end does; mvsf_init_depth_map sums face by face, which may differ in the last bits of a normal
 *   faces    3 vertex indices per face, in the order the rasterisers draw them (a later face overwrites an earlier one)
 * The vertices are the points in the order given; with addCorners != 0 and at least 3 points the four image corners follow them, at depths extrapolated from the
 * neighbouring faces around avgDepth (:1050-1107).  *nVerts and *nFaces always receive the counts.  With vertCap == 0 and faceCap == 0 nothing else is written (the
 * call that sizes the arrays); otherwise vertCap >= *nVerts and faceCap >= *nFaces are needed (-2 when not) and the arrays are filled.
 * dMin / dMax (either may be NULL): the depth bounds of the points themselves, as mvsf_triangulate_depth_map returns them (FLT_MAX and 0 without points); the caller
 * applies the 0.9 / 1.1 of DepthMapsData::InitViews.  0 on success, -1 for a bad argument, -3 when the image has no camera at that size. */
int mvsf_point_mesh(const mvsf_scene* s, int idx, int w, int h, const uint32_t* points, int nPoints, int addCorners, float avgDepth, float* proj, float* z, float* normals,
                    int vertCap, int* nVerts, uint32_t* faces, int faceCap, int* nFaces, float* dMin, float* dMax);

#ifdef __cplusplus
}
#endif
#endif /* MVSFRONT_MESH_H_ */
