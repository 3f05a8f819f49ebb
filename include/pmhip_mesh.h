/* pmhip_mesh.h -- a triangle mesh rendered into depth and normal maps (csrc/pm_mesh.hip), part of the C ABI of libpmhip.so.
 *
 * A companion of include/pmhip.h, which includes it at its end, exactly as pmhip_normals.h is: a host that includes pmhip.h has these functions, and this header may
 * also be included on its own.  They are declared here and not in pmhip.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the
 * Python bindings read every companion header (openmvs_amd/patchmatch.py).  Conventions, error codes and the engine handle are pmhip.h's.  New functions only:
 * PMHIP_ABI_VERSION stays 7.
 *
 * What is computed is Mesh::Project (libs/MVS/Mesh.cpp:3874-3968) bit for bit: a face is drawn when its three vertices have z > 0 and project inside the image with
 * a border of 3 pixels (nothing is clipped), back faces and empty faces are dropped, a pixel whose centre lies on an edge belongs to both faces, and a pixel ends
 * with the smallest z of the faces that cover it, the lowest face index among equal z.  The mesh is independent of the scene: pmhip_scene_create leaves it alone. */
#ifndef PMHIP_MESH_H_
#define PMHIP_MESH_H_
#include "pmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mesh becomes resident: vertices 3 * nVertices floats, faces 3 * nFaces vertex indices.  vertexNormals 3 * nVertices floats, or NULL: they are computed as
 * Mesh::ComputeNormalVertices does (libs/MVS/Mesh.cpp:356-371: float sums of the faces' unnormalised cross products in face order, normalised; a vertex without a
 * non-degenerate face keeps a zero normal).  A mesh set before is replaced.  nVertices == 0, nFaces == 0, a NULL array or a face index >= nVertices is PMHIP_E_ARG,
 * checked before anything is uploaded: the mesh set before stays. */
int pmhip_mesh_set(pmhip_engine* e, const float* vertices, uint32_t nVertices, const uint32_t* faces, uint32_t nFaces, const float* vertexNormals);
/* The resident vertex normals, 3 * nVertices floats: those passed in, or those computed.  PMHIP_E_STATE without a mesh. */
int pmhip_mesh_get_vertex_normals(pmhip_engine* e, float* out);
/* Mesh::Project for nViews cameras in one call, each at its own size: K9, R9 nine doubles per view (row-major), C3 three, wh two ints (width, height).  depthOut[i]
 * receives w_i * h_i floats (0 where no face is).  normalOut NULL, or normalOut[i] NULL: depth only for every / that view; else normalOut[i] receives 3 * w_i * h_i
 * floats, R_float * normalized(interpolated vertex normal) of the winning face, zeros where no face is.  Blocking.  The engine renders as many views at a time as its
 * memory budget holds (pmhip_mesh_set_tuning).  nViews == 0 is a no-op.  A NULL table, w_i or h_i <= 0, more than INT_MAX pixels or a NULL depthOut[i] is PMHIP_E_ARG,
 * a call without a mesh PMHIP_E_STATE: every view is checked before the first launch, the reason is in pmhip_last_error, and the engine stays usable. */
int pmhip_mesh_project(pmhip_engine* e, int nViews, const double* K9, const double* R9, const double* C3, const int32_t* wh, float* const* depthOut, float* const* normalOut);
/* The visibility test of Scene::SampleMeshWithVisibility (libs/MVS/Scene.cpp:656-667) for every (vertex, view): the depth-only maps are rendered internally and nothing
 * but the bitset comes back.  bitsOut holds ceil(nViews / 32) words per vertex, vertex-major; bit (i & 31) of word i / 32 is set when the vertex lies in front of
 * the camera, projects inside view i with a border of 1 and z * thFrontDepth < depth map at the rounded projection (0.985 in the reference); the unused high bits of
 * the last word are 0.  Errors as for pmhip_mesh_project. */
int pmhip_mesh_visibility(pmhip_engine* e, int nViews, const double* K9, const double* R9, const double* C3, const int32_t* wh, uint32_t* bitsOut, float thFrontDepth);
/* Frees the mesh and its working buffers; without a mesh a no-op.  pmhip_release and pmhip_destroy do the same. */
int pmhip_mesh_release(pmhip_engine* e);
/* How the work is mapped; the results never depend on it.  boxPixels: a face whose clipped bounding box holds more pixels than this is rasterised by a workgroup
 * instead of one lane (> 0; 0 keeps the value, < 0 restores the default).  batchBytes: device memory one batch of views may use for its vertex records, keys and
 * maps; at least one view is always rendered (0 keeps the value). */
int pmhip_mesh_set_tuning(pmhip_engine* e, int boxPixels, uint64_t batchBytes);
/* Five numbers.  Of the last pmhip_mesh_project / pmhip_mesh_visibility call: out[0] batches, out[1] (view, face) pairs rasterised by a workgroup; out[2] boxPixels
 * in force, out[3] batchBytes in force; out[4] microseconds the device spent on that call's clears and kernels (HIP events; uploads and downloads not included). */
int pmhip_mesh_get_stats(pmhip_engine* e, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PMHIP_MESH_H_ */
