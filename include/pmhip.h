/* pmhip.h -- C ABI of the MI355X-native PatchMatch depth-map engine (libpmhip.so).
 *
 * Drop-in boundary: the reference dispatches every depth-map estimation through
 *     if (pmCUDA) { pmCUDA->EstimateDepthMap(arrDepthData[idxImage]); return true; }
 * (libs/MVS/SceneDensify.cpp:618-623); the plug-in object has four methods
 * (libs/MVS/PatchMatchCUDA.inl:102-108): ctor(device), Init(bGeomConsistency), Release(),
 * EstimateDepthMap(DepthData&), and is created / re-initialised at
 * libs/MVS/SceneDensify.cpp:1872-1881 and :1910-1916.  Section 1 mirrors exactly that surface
 * with plain pointers and sizes.  Section 2 is the HBM-resident scene interface the reference
 * reaches through files (depthNNNN.dmap written per view and re-read by the geometric rounds,
 * libs/MVS/SceneDensify.cpp:378-414,2095-2117): all images, cameras and depth maps stay on the
 * device and many reference views are estimated concurrently -- this is what fills the GPU.
 *
 * Algorithm = the reference's *CPU* estimator (libs/MVS/DepthMap.cpp:415-971 driven by
 * libs/MVS/SceneDensify.cpp:490-805), not its CUDA variant; see DESIGN.md.
 * All functions return 0 on success, a negative PMHIP_E_* code otherwise; none ever exits.
 * A handle is single-caller (the reference serialises calls with a semaphore,
 * SceneDensify.cpp:2041-2059) but may be used from different host threads sequentially.
 */
#ifndef PMHIP_H_
#define PMHIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMHIP_MAX_SOURCES 16 /* >= OPTDENSE::nMaxViews (12), libs/MVS/DepthMap.cpp:76 */

enum {
	PMHIP_OK = 0,
	PMHIP_E_ARG = -1,      /* bad argument */
	PMHIP_E_SIZE = -2,     /* views differ in size, or image too small for the requested sub-resolution levels */
	PMHIP_E_HIP = -3,      /* HIP runtime error (see pmhip_last_error) */
	PMHIP_E_STATE = -4,    /* call out of order (e.g. estimate before init) */
	PMHIP_E_NODEVICE = -5  /* no usable GPU: the adapter falls back like SceneDensify.cpp:1876-1877 */
};

typedef struct pmhip_engine pmhip_engine;

/* OPTDENSE subset consumed by the estimator; defaults = libs/MVS/DepthMap.cpp:69-114. */
typedef struct PMHipParams {
	uint32_t nSubResolutionLevels;      /* 2 */
	uint32_t nEstimationIters;          /* 3 */
	uint32_t nEstimationGeometricIters; /* 2 (only decides the finalize threshold x1.333, SceneDensify.cpp:774-776) */
	uint32_t nRandomIters;              /* 6 */
	float fEstimationGeometricWeight;   /* 0.1 */
	float fRandomDepthRatio;            /* 0.003 */
	float fRandomAngle1Range;           /* 16 deg */
	float fRandomAngle2Range;           /* 10 deg */
	float fRandomSmoothDepth;           /* 0.02 */
	float fRandomSmoothNormal;          /* 13 deg */
	float fRandomSmoothBonus;           /* 0.93 */
	float fNCCThresholdKeep;            /* 0.9 */
	float fDescriptorMinMagnitudeThreshold; /* 0.02 */
	uint32_t seed;                      /* counter-based RNG seed (the reference seeds from random_device) */
} PMHipParams;

/* DepthData::ViewData (libs/MVS/DepthMap.h:158-205) as plain data; images are contiguous
 * row-major float gray in [0,1] (cv::Mat1f), cameras are x_cam = R (X - C). */
typedef struct PMHipView {
	const float* image;       /* host pointer, w*h floats */
	int32_t w, h;
	double K[9], R[9], C[3];
	const float* depth;       /* nullable; known depth-map of this source view => geometric pass */
	double Kd[9], Rd[9], Cd[3]; /* camera stored with that depth-map (cameraDepthMap); all zero = the view's own camera */
	uint32_t id;              /* global view ID (mixed into the RNG key for views[0]) */
	int32_t dw, dh;           /* size of that depth-map; 0, 0 = w, h.  The map is addressed through Kd/Rd/Cd, so it need not have the image's size */
} PMHipView;

/* DepthData (libs/MVS/DepthMap.h:157-271): views[0] is the reference view. depthMap/normalMap
 * are in/out (zero depth / zero normal == "unset", randomised in the init pass exactly like
 * ScoreDepthMapTmp, SceneDensify.cpp:505-512); confMap is out ([0,1], 1 best); all caller-owned. */
typedef struct PMHipDepthData {
	const PMHipView* views;
	int32_t nViews;           /* 1 + number of source views, 2..1+PMHIP_MAX_SOURCES */
	float* depthMap;          /* w*h */
	float* normalMap;         /* w*h*3, camera space */
	float* confMap;           /* w*h */
	float dMin, dMax;
} PMHipDepthData;

/* ---- 1. PatchMatchCUDA-shaped interface -------------------------------------------------- */
int pmhip_default_params(PMHipParams* p);
/* PatchMatchCUDA::PatchMatchCUDA(int device), PatchMatchCUDA.cpp:46-51 */
int pmhip_create(int device, pmhip_engine** out);
/* PatchMatchCUDA::~PatchMatchCUDA, PatchMatchCUDA.cpp:53-56 */
void pmhip_destroy(pmhip_engine* e);
/* PatchMatchCUDA::Init(bool bGeomConsistency), PatchMatchCUDA.cpp:97-106 */
int pmhip_init(pmhip_engine* e, int bGeomConsistency);
/* PatchMatchCUDA::Release(), PatchMatchCUDA.cpp:58-81 */
int pmhip_release(pmhip_engine* e);
/* PatchMatchCUDA::EstimateDepthMap(DepthData&), PatchMatchCUDA.cpp:174-416; semantics of
 * DepthMapsData::EstimateDepthMap(idx, nGeometricIter), SceneDensify.cpp:616-805:
 * nGeometricIter < 0 -> photometric pass over the pyramid; >= 0 -> that geometric round
 * (requires pmhip_init(e,1) and views[1..].depth). Blocking.
 * views[1..] may have any size (the reference rescales a neighbour whose scale differs by >= 15 %, ViewData::ScaleImage, DepthMap.h:194-204,
 * SceneDensify.cpp:325-349; the resampling itself -- INTER_AREA / INTER_CUBIC -- stays with the caller, as there): every source view is
 * projected into with its own K and sampled within its own bounds, at every pyramid level (ScaleDepthData scales each image by 1/2^l). */
int pmhip_estimate_depth_map(pmhip_engine* e, PMHipDepthData* dd, const PMHipParams* p, int nGeometricIter);
/* The same with DepthData::mask (libs/MVS/DepthMap.h:211): mask = w*h bytes, 0 = the pixel is ignored (see pmhip_scene_set_mask), or NULL.
 * maskOption != 0 says that OPTDENSE::nIgnoreMaskLabel is set even though this view has no mask: the level hand-off then resizes the depth map
 * with INTER_NEAREST as the reference does whenever the option is on (SceneDensify.cpp:661). */
int pmhip_estimate_depth_map_masked(pmhip_engine* e, PMHipDepthData* dd, const unsigned char* mask, int maskOption, const PMHipParams* p, int nGeometricIter);
const char* pmhip_last_error(pmhip_engine* e);

/* ---- 2. HBM-resident scene interface ------------------------------------------------------ */
/* Allocate device storage for nImages views of w x h (image pyramids, depth/normal/conf maps,
 * the previous-round depth snapshot).  Replaces Scene images + depthNNNN.dmap files. */
int pmhip_scene_create(pmhip_engine* e, int nImages, int w, int h, int nLevels);
/* Upload (onDevice == 0) or adopt-by-copy (onDevice != 0, device pointer) one view.
 * neighbors: global IDs of its source views, best first (ViewScore order, DepthMap.h:209). */
int pmhip_scene_set_view(pmhip_engine* e, int idx, const float* gray, int onDevice,
                         const double K[9], const double R[9], const double C[3],
                         float dMin, float dMax, const int32_t* neighbors, int nNeighbors);
/* The identity under which slot idx draws its random numbers (the Philox key of a view is derived from it; default: idx).  A process that holds only PART of a scene
 * -- a rank of the multi-GPU driver keeps its block of reference views and their neighbours in a compact scene of local slots -- gives every slot the view's index in
 * the whole scene, so that the depth maps do not depend on how the scene was split (openmvs_amd/distributed.py; the reference seeds per estimator, DepthMap.cpp:370-372). */
int pmhip_scene_set_view_id(pmhip_engine* e, int idx, uint32_t viewID);
/* The same for a view whose image has its own size w x h (the reference sizes every DepthData on its own image, DepthMapsData::InitViews,
 * libs/MVS/SceneDensify.cpp:306-459; also a neighbour rescaled by ViewData::ScaleImage): it keeps its own pyramid and its own depth / normal /
 * confidence maps of that size, and is a view like any other -- source view, reference view (a batch is swept one size class after the other),
 * per-map filters, cross-view filter and fusion against neighbours of other sizes.  pmhip_scene_get_maps / set_maps / set_conf / set_color of such
 * a view (and its ignore mask, pmhip_scene_set_mask) have w*h entries; pmhip_scene_device_ptr returns its own buffers.  gray is required. */
int pmhip_scene_set_view_sized(pmhip_engine* e, int idx, const float* gray, int w, int h, int onDevice,
                               const double K[9], const double R[9], const double C[3],
                               float dMin, float dMax, const int32_t* neighbors, int nNeighbors);
/* Known depth-map of view idx (host pointer, dw*dh floats) for the geometric rounds in which it is a source view, with the camera it was stored
 * with (DepthData::ViewData::depthMap / cameraDepthMap, loaded from the neighbour's .dmap at SceneDensify.cpp:378-393).  While installed it is
 * read instead of the scene's snapshot of that view; depth == NULL removes it. */
int pmhip_scene_set_source_depth(pmhip_engine* e, int idx, const float* depth, int dw, int dh,
                                 const double Kd[9], const double Rd[9], const double Cd[3]);
/* Estimate the depth maps of viewIds[0..nViews) concurrently (one EstimateDepthMap per view,
 * SceneDensify.cpp:616-805).  nGeometricIter < 0: photometric; >= 0: geometric round reading the
 * snapshot taken by pmhip_scene_commit_round.  Asynchronous on the engine stream unless sync != 0. */
int pmhip_scene_estimate(pmhip_engine* e, const int32_t* viewIds, int nViews, const PMHipParams* p,
                         int nGeometricIter, int sync);
/* End of a round: snapshot depth maps of all views as the "saved .dmap" the next geometric round
 * reads (the reference renames depthNNNN.geo.dmap -> .dmap, SceneDensify.cpp:1943-1950). */
int pmhip_scene_commit_round(pmhip_engine* e);
/* Clear a view's maps to "unset" (InitViews with an empty point cloud, SceneDensify.cpp:417-425). */
int pmhip_scene_reset_view(pmhip_engine* e, int idx);
/* Provide an initial depth/normal estimate (host pointers, nullable each). */
int pmhip_scene_set_maps(pmhip_engine* e, int idx, const float* depth, const float* normal);
/* Ignore mask of a view (OPTDENSE::nIgnoreMaskLabel, DepthEstimator::ImportIgnoreMask, DepthMap.cpp:296-323): w*h bytes at image
 * resolution, 0 = the pixel is ignored -- not estimated at any pyramid level, depth / normal / confidence 0 -- exactly like the masked
 * MapMatrix2ZigzagIdx + DepthData::ApplyIgnoreMask (SceneDensify.cpp:679-683); level masks are INTER_NEAREST resamples.  NULL removes it.
 * While masks are in use the level hand-off resizes depth maps with INTER_NEAREST as the reference does (:661);
 * pmhip_scene_set_mask_mode forces that on (1) / off (0) for scenes where the option is set but no view has a mask file; -1 = automatic. */
int pmhip_scene_set_mask(pmhip_engine* e, int idx, const unsigned char* mask);
int pmhip_scene_set_mask_mode(pmhip_engine* e, int mode);
/* Install a confidence map (host pointer), e.g. one read back from a .dmap before filtering / fusing without re-estimating. */
int pmhip_scene_set_conf(pmhip_engine* e, int idx, const float* conf);
/* Download maps (any pointer may be NULL); a view with its own size returns maps of that size. */
int pmhip_scene_get_maps(pmhip_engine* e, int idx, float* depth, float* normal, float* conf);
/* Device pointers for collectives (RCCL all-gather of the snapshot / broadcast of images).
 * what: 0 image level 0, 1 depth, 2 normal, 3 conf, 4 snapshot depth.  The per-kind arrays are
 * single contiguous allocations ordered by view index, so idx 0 addresses the whole set (views with their own size live outside them: their
 * pointer addresses that view alone, and pmhip_scene_copy takes them one by one).  After writing images call pmhip_scene_images_updated,
 * after writing depth maps pmhip_scene_maps_updated: the engine cannot see writes through these pointers. */
void* pmhip_scene_device_ptr(pmhip_engine* e, int what, int idx);
/* DepthMapsData::FilterDepthMap (SceneDensify.cpp:1050-1299) for each view of viewIds against its first <= 8 neighbours
 * (Scene::DenseReconstructionFilter, :2136-2170): cross-view splat + z-test, then the confidence-weighted fusion
 * (bAdjust != 0, OPTDENSE::bFilterAdjust) or the strict agreement test.  Defaults: nMinViewsFilter 2, nMinViewsFilterAdjust 1,
 * fDepthDiffThreshold 0.01 (DepthMap.cpp:77-78,91).  Results are staged until pmhip_scene_filter_commit, because every view
 * must be filtered against the unfiltered maps of its neighbours (:2183-2210). */
int pmhip_scene_filter(pmhip_engine* e, const int32_t* viewIds, int nViews, int bAdjust, uint32_t nMinViewsFilter,
                       uint32_t nMinViewsFilterAdjust, float fDepthDiffThreshold, int sync);
int pmhip_scene_filter_commit(pmhip_engine* e);
/* DepthMapsData::RemoveSmallSegments (SceneDensify.cpp:809-900; OPTDENSE::nSpeckleSize 100, fDepthDiffThreshold 0.01): invalidates
 * depth segments smaller than nSpeckleSize pixels, in place on the device; same result as the sequential region growing. */
int pmhip_scene_remove_small_segments(pmhip_engine* e, const int32_t* viewIds, int nViews, uint32_t nSpeckleSize, float fDepthDiffThreshold);
/* DepthMapsData::GapInterpolation (SceneDensify.cpp:904-1045; OPTDENSE::nIpolGapSize 7, fDepthDiffThreshold 0.01): fills row then
 * column gaps of the depth / normal / confidence maps of these views, in place on the device. */
int pmhip_scene_gap_interpolation(pmhip_engine* e, const int32_t* viewIds, int nViews, uint32_t nIpolGapSize, float fDepthDiffThreshold);
/* MVS::EstimateNormalMap on the resident depth maps and on host buffers: include/pmhip_normals.h, included at the end of this header. */
/* DepthMapsData::FuseDepthMaps (SceneDensify.cpp:1372-1650) over the resident depth / normal / confidence maps: every unclaimed depth
 * seeds a 3D point, claims the agreeing pixels of the view's neighbours (depth within fDepthDiffThreshold, normals within
 * fNormalDiffThreshold degrees), is kept if it gathered nMinViewsFuse views and then zeroes the neighbour depths it occludes.
 * `order` lists the views to fuse, best connected first (the reference sorts by Image::neighbors.size(), :1423-1450); each view uses
 * the neighbour list given to pmhip_scene_set_view (the IDs stored in its .dmap).  Runs on working copies: the scene's maps are not
 * modified.  Point order, views, weights, positions, colours and normals equal the sequential reference (see csrc/pm_fuse.h).
 * nMinViewsFuse < 2 selects DepthMapsData::MergeDepthMaps instead (:1305-1368, as Scene::DenseReconstruction does, :1695-1698): every valid
 * depth becomes a single-view point (pass the views in index order; weights come back 0, the reference produces none).
 * Defaults (DepthMap.cpp:75,92,93,101,102): nMinViewsFuse 2, fDepthDiffThreshold 0.01, fNormalDiffThreshold 25, colours and normals on. */
typedef struct PMHipFuseParams {
	uint32_t nMinViewsFuse;
	float fDepthDiffThreshold;
	float fNormalDiffThreshold;   /* degrees */
	int32_t bEstimateColor;       /* needs pmhip_scene_set_color for every view */
	int32_t bEstimateNormal;
} PMHipFuseParams;
/* 8-bit BGR image of view idx at depth-map resolution (Image::image, read at SceneDensify.cpp:1529,1567), host pointer, w*h*3 bytes. */
int pmhip_scene_set_color(pmhip_engine* e, int idx, const unsigned char* bgr);
int pmhip_scene_fuse(pmhip_engine* e, const int32_t* order, int nOrder, const PMHipFuseParams* params,
                     uint64_t* nPoints, uint64_t* nViews, uint64_t* nDepths);
/* Download the fused cloud (PointCloud::points / pointViews / pointWeights / colors / normals, libs/MVS/PointCloud.h): points 3*nPoints
 * floats, viewStart nPoints+1 offsets into views / weights / projs (nViews entries; projs = x,y of the pixel each view contributed),
 * colors 3*nPoints BGR bytes, normals 3*nPoints floats.  Any pointer may be NULL. */
int pmhip_scene_fuse_get(pmhip_engine* e, float* points, uint32_t* viewStart, uint32_t* views, float* weights, uint16_t* projs,
                         unsigned char* colors, float* normals);
/* Reservation rounds the last pmhip_scene_fuse needed, summed over its views (diagnostic). */
uint64_t pmhip_scene_fuse_rounds(pmhip_engine* e);
/* The last block of Scene::DenseReconstruction on the resident cloud (SceneDensify.cpp:1724-1737), in the reference's order: crop to the ROI
 * (PointCloud::RemovePointsOutside, the backward swap-remove order of PointCloud.cpp:82-87 reproduced exactly for points, views, weights,
 * projections, colours and normals), colours (EstimatePointColors, DepthMap.cpp:1429-1465, bit-exact; needs pmhip_scene_set_color for every
 * view a point lists) when the cloud has none, and PCA normals over the nNeighbors nearest points (EstimatePointNormals, DepthMap.cpp:1469-1519;
 * the point itself is one of them, distance ties go to the lower index) when it has none.  Works on the cloud of the last pmhip_scene_fuse or
 * pmhip_scene_cloud_set; pmhip_scene_fuse_get returns the result.  nPoints / nViews: the sizes after the crop (either may be NULL). */
typedef struct PMHipCloudParams {
	int32_t bCrop;                           /* RemovePointsOutside(ROI); the caller tests Scene::IsBounded */
	float obbRot[9], obbPos[3], obbExt[3];   /* TOBB<float,3> after Set(rot, ptMin, ptMax): row-major rotation, centre, half-extents */
	float fBorderROI;                        /* > 0: extents multiplied (EnlargePercent), < 0: -fBorderROI added (Enlarge), 0: as is (SceneDensify.cpp:1728) */
	int32_t bEstimateColor;                  /* EstimatePointColors, if the cloud has no colours */
	int32_t bEstimateNormal;                 /* EstimatePointNormals, if the cloud has no normals */
	int32_t nNeighbors;                      /* k of the PCA (16), 1..32 */
} PMHipCloudParams;
int pmhip_scene_cloud_finish(pmhip_engine* e, const PMHipCloudParams* p, uint64_t* nPoints, uint64_t* nViews);
/* Replace the resident cloud with a host cloud (an archive's points, a test cloud): points 3*nPoints floats, viewStart nPoints+1 offsets,
 * views (image indices of the loaded scene, at least one per point), weights (may be NULL: zeros).  The cloud has no colours, normals or projections. */
int pmhip_scene_cloud_set(pmhip_engine* e, const float* points, const uint32_t* viewStart, const uint32_t* views, const float* weights, uint64_t nPoints);
/* Diagnostic, also what the tests check: the nNeighbors (1..32) indices of each listed query point, nearest first, as the normals use them
 * (out: nQueries*nNeighbors; entries beyond the cloud's size are 0xFFFFFFFF). */
int pmhip_scene_cloud_knn(pmhip_engine* e, int nNeighbors, const uint32_t* queries, uint32_t nQueries, uint32_t* out);
/* Milliseconds of the steps of the last pmhip_scene_cloud_finish, each ended by a stream synchronisation: crop, grid build, k-NN + PCA, colours. */
int pmhip_scene_cloud_times(pmhip_engine* e, double ms[4]);
/* Scene::PointCloudFilter(thRemove) (--filter-point-cloud, SceneDensify.cpp:2225-2359) and PointCloud::RemoveMinViews (--export-number-views -N,
 * PointCloud.cpp:88-93) on the resident cloud.  nMinViews > 0 first removes the points with fewer views; bVisibility then votes on what is left: for
 * every point i and every view v it lists, the cone from Cast<float>(C_v) through the point with half-angle angle_v and height 1.02 x distance
 * classifies EVERY point j of the cloud (TConeIntersect::Classify in float, not depth-similar within 1 %): visibility[j] += views(j) behind the point,
 * -= views(i) in front of it; points with visibility <= thRemove are removed.  Both removals are the reference's backward swap-remove loop, for
 * points, views, weights, projections, colours and normals.  The vote is the sum over all points j (the reference's octree computes that sum up to the
 * float rounding of its conservative cell pruning); the angular bins it runs on never change it (csrc/pm_cloud_filter.hip).
 * camC (3 doubles per camera) / camAngle (radians per camera), nCams of each, or both NULL: the loaded scene's C and 2 atan(w / (2 K00)) / w at each
 * view's own width.  Nothing else of a scene is read, so with them the call works in an engine that holds no images.  A new struct beside the others:
 * PMHIP_ABI_VERSION stays 7. */
typedef struct PMHipCloudFilterParams {
	int32_t bVisibility;                     /* run the visibility vote and remove visibility <= thRemove */
	int32_t thRemove;                        /* the application passes it only when negative; any value here */
	uint32_t nMinViews;                      /* > 0: RemoveMinViews(nMinViews) first */
	int32_t nCams;                           /* cameras in camC / camAngle */
	const double* camC; const float* camAngle;
} PMHipCloudFilterParams;
/* pmhip_scene_cloud_set with optional colours (3 bytes BGR per point) and normals (3 floats per point), either may be NULL; nCams > 0 replaces the
 * loaded scene's image count in the range check of the view indices, so that an archive's cloud can be installed in an engine without a scene. */
int pmhip_scene_cloud_load(pmhip_engine* e, const float* points, const uint32_t* viewStart, const uint32_t* views, const float* weights,
                           const unsigned char* colors, const float* normals, uint64_t nPoints, int32_t nCams);
/* nPoints / nViews: the sizes after the removal (either may be NULL); pmhip_scene_fuse_get returns the cloud.  An empty cloud is a no-op; a point
 * that lists a view outside the cameras is PMHIP_E_STATE. */
int pmhip_scene_cloud_filter(pmhip_engine* e, const PMHipCloudFilterParams* p, uint64_t* nPoints, uint64_t* nViews);
/* The votes of the last filter, indexed as the cloud was before the visibility removal (n = that size; after nMinViews, if given). */
int pmhip_scene_cloud_visibility(pmhip_engine* e, int32_t* out, uint64_t n);
/* The cone constants the last filter used, per camera: angle, cosAngleSq = SQUARE(cosf(angle)) (cosf on the host); 0, 0 for a view that is not set. */
int pmhip_scene_cloud_filter_cones(pmhip_engine* e, float* out /* nCams x 2 */);
/* Milliseconds of the last filter, each part ended by a stream synchronisation and summed over the views: binning, cone pass, removal. */
int pmhip_scene_cloud_filter_times(pmhip_engine* e, double ms[3]);
/* Diagnostic: the cones of the last filter ((point, view) pairs) and the candidates classified against them, summed. */
int pmhip_scene_cloud_filter_counts(pmhip_engine* e, uint64_t out[2]);
/* Device-to-device copy between a caller buffer (e.g. a torch tensor used for an RCCL collective)
 * and `count` consecutive views of one per-kind array, starting at view firstIdx; `what` as above.
 * toEngine != 0 copies caller -> engine.  Asynchronous on the engine stream. */
int pmhip_scene_copy(pmhip_engine* e, int what, int firstIdx, int count, void* devPtr, int toEngine);
/* Rebuild image pyramids after image level 0 was written through pmhip_scene_device_ptr. */
int pmhip_scene_images_updated(pmhip_engine* e);
/* Depth maps of views [firstIdx, firstIdx + count) were written through pmhip_scene_device_ptr(e, 1, ...) (e.g. by an RCCL all-gather straight
 * into the depth array): marks them as holding a depth map, which pmhip_scene_filter / pmhip_scene_fuse require of a neighbour before they use it
 * (DepthData::IsValid(), SceneDensify.cpp:2150-2163).  pmhip_scene_estimate, _set_maps and _copy(what == 1, toEngine) do this themselves; a raw
 * pointer write cannot, and such neighbours would be skipped without this call. */
int pmhip_scene_maps_updated(pmhip_engine* e, int firstIdx, int count);
/* ---- 2b. the image store: working-resolution images made on the device from decoded 8-bit images -------------------------------------
 * The caller hands a decoded image at its stored size over once; the device produces what Image::ResizeImage (libs/MVS/Image.cpp:139-155: cv::resize INTER_AREA,
 * shrinking only) and TImage::toGray (libs/Common/Types.inl:2377-2425) produce -- the 8-bit BGR image and the gray float image at the working size -- and the
 * resampled neighbour copies of DepthData::ViewData::ScaleImage (libs/MVS/DepthMap.h:193-204: INTER_AREA below 1, INTER_CUBIC above).  A scene view adopts an
 * entry by a device-to-device copy.  The store is independent of the scene: pmhip_scene_create leaves it alone (images are prepared before the scene's slot count
 * is known) and pmhip_scene_bytes does not count it; pmhip_image_drop, pmhip_release and pmhip_destroy free it.  New functions and a new struct beside the others:
 * PMHIP_ABI_VERSION stays 7.  A refused call returns PMHIP_E_ARG with the reason in pmhip_last_error and leaves the engine and the store as they were. */
/* The working size of a W0 x H0 image: TImage::computeMaxResolution (Types.inl:2459-2477) with OPTDENSE::nResolutionLevel / nMinResolution / nMaxResolution, then
 * Image::ResizeImage's size rule (double arithmetic, round half to even).  Needs no engine. */
int pmhip_working_size(int W0, int H0, unsigned nResolutionLevel, unsigned nMinResolution, unsigned nMaxResolution, int* w, int* h);
/* DepthData::ViewData::NeedScaleImage / ScaleImage's size: returns 0 when fabsf(scale - 1.f) < 0.15f (in float: the image is used as it is), else 1 with
 * w, h = rint(W * scale), rint(H * scale). */
int pmhip_scaled_size(int W, int H, float scale, int* w, int* h);
/* Entry `key` (any int >= 0; a repeated key replaces the entry) gets the BGR u8 and gray f32 images at w x h of the decoded image img: W0*H0*3 bytes, host pointer,
 * channelOrder 0 = B,G,R, 1 = R,G,B.  w == W0 and h == H0 only converts; enlarging (w > W0 or h > H0) is refused.  Blocking: img may be freed on return. */
int pmhip_image_prepare(pmhip_engine* e, int key, const unsigned char* img, int W0, int H0, int channelOrder, int w, int h);
/* Entry `key` gets ScaleImage(gray of entry srcKey, scale), gray only; w, h (nullable) receive its size.  A scale within 15 % of 1 is refused. */
int pmhip_image_scale(pmhip_engine* e, int key, int srcKey, float scale, int* w, int* h);
/* Download an entry: its size, gray (w*h floats), bgr (w*h*3 bytes); any pointer may be NULL, bgr must be NULL for a gray-only entry. */
int pmhip_image_get(pmhip_engine* e, int key, int* w, int* h, float* gray, unsigned char* bgr);
/* Free an entry; key < 0: all of them.  The store's working buffers (staging, tables) go with the last entry. */
int pmhip_image_drop(pmhip_engine* e, int key);
/* Device memory the store holds right now: entries, the staging of the last decoded image, the uploaded tables. */
uint64_t pmhip_image_bytes(pmhip_engine* e);
/* Since the engine was created or the last reset: images prepared and resampled, bytes of decoded images uploaded, the kernels' time by HIP events and the
 * uploads' time on the host clock (each upload is waited for). */
typedef struct PMHipImageStats {
	uint64_t nPrepared, nScaled, bytesUploaded;
	double kernelMs, uploadMs;
} PMHipImageStats;
int pmhip_image_stats_get(pmhip_engine* e, PMHipImageStats* out, int reset);
/* pmhip_scene_set_view (the entry has the scene's size) or pmhip_scene_set_view_sized (any other size) with the stored gray image of entry `key`, read on the
 * device, and pmhip_scene_set_color when the entry has a colour image.  The view holds copies: the entry may be dropped afterwards. */
int pmhip_scene_set_view_stored(pmhip_engine* e, int idx, int key, const double K[9], const double R[9], const double C[3],
                                float dMin, float dMax, const int32_t* neighbors, int nNeighbors);
/* Device memory the resident scene holds right now, in bytes (images with their layouts, maps, masks, filter staging, batch scratch; not the fusion's working buffers). */
uint64_t pmhip_scene_bytes(pmhip_engine* e);
int pmhip_sync(pmhip_engine* e);
/* Engine stream (hipStream_t) so callers can bracket work with their own events. */
void* pmhip_stream(pmhip_engine* e);

/* Timing of the dominant kernel (the diagonal sweep) measured with HIP events on the streams the
 * launches go to, since the last reset: number of launches, summed milliseconds (sweepMs / sweepLaunches
 * == the kernel's average duration as rocprofv3 reports it, also when view groups run concurrently),
 * summed algorithmic bytes (SURVEY.md 8d model) and pixel-updates. */
typedef struct PMHipKernelStats {
	uint64_t sweepLaunches; double sweepMs; double sweepBytes; uint64_t sweepPixels;
	uint64_t initLaunches; double initMs;
	double sweepWallMs; /* wall time of the passes (hand-off, init, sweeps, finalize of all view groups, which overlap); sweepMs sums the per-stream times of the sweeps alone */
	double sweepHostMs; /* host time spent enqueueing the passes (a few per cent of sweepWallMs: one thread enqueues a launch in ~3 us, profiles/r04_call9_launch_rate.log) */
} PMHipKernelStats;
int pmhip_stats_reset(pmhip_engine* e, int enableEvents);
int pmhip_stats_get(pmhip_engine* e, PMHipKernelStats* out);

/* How the engine maps a batch onto the GPU -- never WHAT it computes: every setting gives the same bits.  pmhip_create fills the defaults (the measured choices of
 * csrc/pm_engine.hip); 0 in a field of pmhip_set_tuning keeps the current value.  The library reads no environment variable. */
typedef struct PMHipTuning {
	int32_t viewGroups;      /* view groups of a batch; each runs its whole pass (every level's hand-off, init, sweeps, finalize) on its own stream, the groups meet at the end of the call (2) */
	int32_t wideMaxViews;    /* batches of at most this many reference views use the speculative sweep kernels for every launch (32); -1 = no speculative kernels at all (also clears widePixels / wide8Pixels unless set in the same call) */
	int32_t wideHyps;        /* hypotheses per round of the speculative kernel: 8, 4 or 2; -1 = by batch size (8 for one or two views, else 2) */
	int32_t sweepLanes;      /* lanes per pixel of pm_sweep2_kernel: 4, 8 or 16; -1 = by batch size */
	int32_t quadBuffer;      /* 1: tap rows address the level's quad images as one buffer, 2: through each view's pointer */
	int32_t widePixels;      /* larger batches: a diagonal launch of at most this many pixels (diagonal length x views of the group) uses the two-wide speculative kernel (20000); -1 = none */
	int32_t wide8Pixels;     /* ... and one of at most this many pixels the eight-wide speculative kernel; -1 = none */
	int32_t reserved0;       /* ignored by pmhip_set_tuning, 0 from pmhip_get_tuning (`launchThreads` until round 4, absent in round 5: the struct is 32 bytes again -- PMHIP_ABI_VERSION) */
} PMHipTuning;
/* OPT-IN, NOT the reference's estimator: tiled sweeps.  The pixels that take part in the estimation are cut into tileW x tileH tiles; a sweep (DepthMap.cpp:329-356 order)
 * runs inside every tile, and a neighbour in another tile is read as the previous sweep left it.  The tiles of a sweep are independent, so a sweep is tileW + tileH - 1
 * launches that each cover every tile of every view instead of w + h launches of one anti-diagonal: what a small batch (one depth map per call, a rank of an 8-GPU split)
 * needs to fill the GPU.  The result is deterministic and equals oracle/pm_oracle.cpp with Opt::tileW / tileH bit for bit, but it is NOT the sequential sweep's: against
 * that it differs like two runs of the reference differ from each other.  0, 0 = off (the default: the reference's sweep, bit for bit). */
int pmhip_set_sweep_tiles(pmhip_engine* e, int tileW, int tileH);
/* The layout of the structs of this header as a number: a host program compares pmhip_abi_version() with the PMHIP_ABI_VERSION it was compiled against before it hands the
 * library a struct (6: PMHipTuning is 32 bytes again -- reserved0; pmhip_set_sweep_tiles; 7: PMHipCloudParams). */
#define PMHIP_ABI_VERSION 7u
uint32_t pmhip_abi_version(void);
int pmhip_get_tuning(pmhip_engine* e, PMHipTuning* out);
int pmhip_set_tuning(pmhip_engine* e, const PMHipTuning* t);

/* ---- 3. self-test hooks (used by tests/, no oracle involved) ------------------------------ */
/* Evaluate csrc/pm_math.h on the device: kind 0 exp, 1 acos, 2 atan2(a,b), 3 sin, 4 cos, 5 sqrt, 6 a/b, 7 (float)sqrt((double)a*a+(double)b*b). */
int pmhip_math_eval(pmhip_engine* e, int kind, const float* a, const float* b, float* out, size_t n);
/* Per-phase cycle counters of the sweep kernel (all zero unless the library was built with -DPM_PROFILE). */
int pmhip_prof_get(pmhip_engine* e, unsigned long long out16[16], int reset);
/* Device resampling kernels on host buffers: kind 0 area (factor f = arg), 1 linear x2, 2 nearest x2. */
int pmhip_resize(pmhip_engine* e, int kind, const float* src, int w, int h, int arg, float* dst);
/* Any resampler of csrc/pm_kernels.hip, launched once through the helper the estimation launches it with (same grid, same block cap), on host buffers and at any
 * size: sw x sh -> dw x dh.  dst is uploaded before the launch and read back whole, so entries the kernel does not write keep the caller's bytes.  Row-major,
 * float unless said otherwise; P = w * h of the side in question.
 *   AREA          src nImg images -> dst nImg images; arg = integer factor f, dw x dh = cvRound(sw / f) x cvRound(sh / f)
 *   UPSAMPLE      src = depth[P] normal[3P] -> dst = depth[P] normal[3P] prior[P]; arg != 0: the depth is taken INTER_NEAREST too (nearestDepth)
 *   NEAREST_DOWN  src = depth[P] normal[3P] -> dst = depth[P] normal[3P]; arg = f, sizes as for AREA
 *   NEAREST_UP    one image, INTER_NEAREST
 *   MASK_LEVEL    one 8-bit image, INTER_NEAREST
 *   SKEW          nImg images -> the folded anti-diagonal-major copy, same size
 *   QUAD          nImg images -> nImg quad images of (w + h - 1) * h float4 entries, same size
 *   DEPTH_QUADS   one depth map (w, h >= 2) -> the quad copy the geometric rounds derive of a source depth map: w * h float4 entries, entry (lx, ly) =
 *                 {D(lx,ly), D(lx+1,ly), D(lx,ly+1), D(lx+1,ly+1)} as bit patterns at ((lx + ly) mod w) * h + ly, 0 for texels the map does not have
 * nImg = 1 except where it is named.  PMHIP_E_SIZE for sizes the kind does not take. */
enum { PMHIP_RESAMPLE_AREA = 0, PMHIP_RESAMPLE_UPSAMPLE = 1, PMHIP_RESAMPLE_NEAREST_DOWN = 2, PMHIP_RESAMPLE_NEAREST_UP = 3, PMHIP_RESAMPLE_MASK_LEVEL = 4,
       PMHIP_RESAMPLE_SKEW = 5, PMHIP_RESAMPLE_QUAD = 6, PMHIP_RESAMPLE_DEPTH_QUADS = 7 };
int pmhip_resample(pmhip_engine* e, int kind, const void* src, int sw, int sh, void* dst, int dw, int dh, int arg, int nImg);

#ifdef __cplusplus
}
#endif
#include "pmhip_normals.h"
#include "pmhip_mesh.h"
#include "pmhip_export.h"
#include "pmhip_seed.h"
#endif /* PMHIP_H_ */
