// pm_engine.hip -- host side of libpmhip.so: the extern "C" boundary declared in include/pmhip.h.
//
// Mirrors the reference's GPU plug-in boundary (PatchMatchCUDA, libs/MVS/PatchMatchCUDA.inl:102-108)
// and the pass structure of DepthMapsData::EstimateDepthMap (libs/MVS/SceneDensify.cpp:616-805):
// per pyramid level {level hand-off, init-score pass, nEstimationIters sweeps}, then finalize.
// Everything stays in HBM between passes; one stream; no host sync inside a call.
#include "../../include/pmhip.h"
#include "pm_kernels.hip"
#include "pm_band.hip"
#include "pm_wide_n.hip"
#include "pm_filter.hip"
#include "pm_fuse.hip"
#include "pm_cloud.hip"
#include "pm_cloud_filter.hip"
#include "pm_image.hip"
#include "pm_normal.hip"
#include "pm_mesh.hip"
#include "pm_export.hip"
#include "seed_raster.hip"
#include "hip_buf.h"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <set>
#include <string>
#include <vector>

#ifndef PMHIP_DEFAULT_WIDE_PIXELS
#define PMHIP_DEFAULT_WIDE_PIXELS 20000   // larger batches: diagonal launches of at most this many pixels (diagonal length x views of the group) use the two-wide speculative
                                         // kernel -- the ramps of the fine level and all of the coarse ones.  profiles/r04_call9_lanes_100.log (100 views, Mpix/s): none 46.4,
                                         // <= 8000: 48.1, <= 16000: 48.6, <= 24000: 48.6; 50 views: 43.4 against 42.7 with the two-wide kernel everywhere
#define PMHIP_DEFAULT_WIDE8_PIXELS 0     // ... and of at most this many pixels the eight-wide one (no effect measured at 13 / 100 views: off)
#endif
#ifndef PMHIP_WIDE_DIAGONAL
#define PMHIP_WIDE_DIAGONAL 400   // ... and of at most this many pixels per view of the group
#endif
#ifndef PMHIP_DEFAULT_WIDE
#define PMHIP_DEFAULT_WIDE 32   // batches of at most this many reference views use the speculative kernels: eight hypotheses per round (one wave per pixel) for 1-2 views, two per round
                                // (four pixels per wave, pm_wide_n.hip) from 3 views on.  Measured in round 4 (profiles/r04_call7_lanes_*.log, full schedule at 1920x1080, Mpix/s;
                                // two-wide / pm_sweep2_kernel): 13 views 26.8 / 19.7, 25: 37.5 / 31.2, 50: 41.0 / 39.3, 100: 42.6 / 44.9 (<4,2>)
#endif
#ifndef PMHIP_DEFAULT_LANES
#define PMHIP_DEFAULT_LANES 0    // sweep kernel: lanes per pixel; 0 = by batch size (one view per lane for small batches, four lanes and two views per lane
                                 // from PMHIP_LANES4_FROM reference views on: measured 41.2 vs 39.7 Mpix/s at 100 views, 11.5 vs 16.6 at 13, profiles/r03_variants_call6_sweep2.log)
#ifndef PMHIP_LANES4_FROM
#define PMHIP_LANES4_FROM 80     // measured (profiles/r03_variants_call21_mid_batches.log): one view per lane wins up to 70 reference views (25: 28.2 vs 21.2, 50: 36.8 vs 33.3, 70: 38.9 vs 38.2 Mpix/s), two per lane at 100 (42.9 vs 41.5)
#endif
#endif
#ifndef PMHIP_DEFAULT_GROUPS
#define PMHIP_DEFAULT_GROUPS 2
#endif
namespace {

#define HIPCHK(e, call) do { hipError_t _r = (call); if (_r != hipSuccess) { (e)->err = std::string(#call) + ": " + hipGetErrorString(_r); return PMHIP_E_HIP; } } while (0)

// The storage of a view whose image has another size than the scene's (the reference sizes every DepthData on its own, DepthMapsData::InitViews, SceneDensify.cpp:306-459; a
// neighbour rescaled by ViewData::ScaleImage, DepthMap.h:194-204): it keeps its own pyramid and its own maps here.  sw == 0: image and maps live in the scene arrays.
struct SideStorage {
	int sw = 0, sh = 0;
	DevBuf<float> oDepth, oNormal, oConf, oSnap;   // sw x sh (x 3): depth, normal, confidence (cost), previous round's depth
	DevBuf<float> oFDepth, oFConf;                 // staged results of the cross-view filter (pmhip_scene_filter / _commit)
	DevBuf<uint8_t> oBgr;                          // its 8-bit BGR image (pmhip_scene_set_color), sw x sh x 3
	DevBuf<unsigned char> oMask[4];                // its ignore mask per pyramid level (pmhip_scene_set_mask)
	DevBuf<float> sImg[4], sImgS[4];
	DevBuf<float4> sImgQ[4];
	bool sideDirty = false;
};
struct SceneView : SideStorage {
	double K[9], R[9], C[3];
	float dMin = 0, dMax = 0;
	int nNb = 0; int nb[PM_MAX_SRC];
	uint32_t id = 0;
	bool set = false;
	bool hasMaps = false;   // a depth map exists for this view (estimated, uploaded or copied in): DepthData::IsValid() of the reference's filter / fuse loops
	// A known depth-map of this view to be read by geometric rounds instead of the scene's snapshot, of its own size and with the camera it
	// was stored with (DepthData::ViewData::depthMap / cameraDepthMap, filled from the neighbour's .dmap at SceneDensify.cpp:378-393)
	DevBuf<float> sDepth; int dw = 0, dh = 0; double Kd[9], Rd[9], Cd[3];
	void resetSide() { static_cast<SideStorage&>(*this) = SideStorage{}; }   // (the known depth-map stays)
};
static int lvlSize(int n, int l) { return (int)nearbyint((double)n / (double)(1 << l)); }   // cvRound(size / 2^l), ties to even

// cv::Matx product convention (accumulate from 0, left to right)
void mul33(const double* a, const double* b, double* c) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += a[i*3+k] * b[k*3+j]; c[i*3+j] = s; }
}
void mul31(const double* a, const double* v, double* c) {
	for (int i = 0; i < 3; ++i) { double s = 0; for (int k = 0; k < 3; ++k) s += a[i*3+k] * v[k]; c[i] = s; }
}
void transp33(const double* a, double* t) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) t[j*3+i] = a[i*3+j]; }
// cv::Matx<double,3,3>::inv(): adjugate / determinant (OpenCV matx.hpp, Matx_FastInvOp<_Tp,3,3>)
void inv33(const double* a, double* b) {
	double d = a[0]*(a[4]*a[8] - a[7]*a[5]) - a[1]*(a[3]*a[8] - a[6]*a[5]) + a[2]*(a[3]*a[7] - a[6]*a[4]);
	d = 1 / d;
	b[0] = (a[4]*a[8] - a[5]*a[7]) * d; b[1] = (a[2]*a[7] - a[1]*a[8]) * d; b[2] = (a[1]*a[5] - a[2]*a[4]) * d;
	b[3] = (a[5]*a[6] - a[3]*a[8]) * d; b[4] = (a[0]*a[8] - a[2]*a[6]) * d; b[5] = (a[2]*a[3] - a[0]*a[5]) * d;
	b[6] = (a[3]*a[7] - a[4]*a[6]) * d; b[7] = (a[1]*a[6] - a[0]*a[7]) * d; b[8] = (a[0]*a[4] - a[1]*a[3]) * d;
}
// Camera::InvK, libs/MVS/Camera.h:176-185
void invK(const double* K, double* o) {
	for (int i = 0; i < 9; ++i) o[i] = (i % 4 == 0) ? 1.0 : 0.0;
	o[0] = 1.0 / K[0]; o[4] = 1.0 / K[4]; o[2] = -K[2] * o[0]; o[5] = -K[5] * o[4];
}
// Camera::ScaleK(K, size, newSize), libs/MVS/Camera.h:160-170
void scaleK(const double* K, int w, int h, int nw, int nh, double* o) {
	const double sx = (double)nw / (double)w, sy = (double)nh / (double)h;
	o[0] = K[0]*sx; o[1] = K[1]*sx; o[2] = (K[2]+0.5)*sx-0.5;
	o[3] = 0;       o[4] = K[4]*sy; o[5] = (K[5]+0.5)*sy-0.5;
	o[6] = 0; o[7] = 0; o[8] = 1;
}

} // namespace

// The fused cloud: seven arrays of one capacity.  fu.out is the resident cloud, cl.alt the target of a removal (swapped afterwards).
struct CloudBufs {
	DevBuf<float> points; DevBuf<uint32_t> viewStart, views; DevBuf<float> weights; DevBuf<uint16_t> projs; DevBuf<uint8_t> colors; DevBuf<float> normals;
	size_t cap = 0;
	// all arrays anew when the capacity grows (exactly to `c`), colours / normals on demand at the current capacity
	hipError_t reserve(size_t c, bool wantColor, bool wantNormal) {
		hipError_t r = hipSuccess;
		if (cap < c) {
			*this = CloudBufs{};
			if ((r = points.alloc(3 * c)) != hipSuccess || (r = viewStart.alloc(c + 1)) != hipSuccess || (r = views.alloc(c)) != hipSuccess ||
			    (r = weights.alloc(c)) != hipSuccess || (r = projs.alloc(2 * c)) != hipSuccess) { *this = CloudBufs{}; return r; }
			cap = c;
		}
		if (wantColor && !colors) r = colors.alloc(3 * cap);
		if (r == hipSuccess && wantNormal && !normals) r = normals.alloc(3 * cap);
		return r;
	}
	PMFuseOut view(bool color = true, bool normal = true) const { return PMFuseOut{points, viewStart, views, weights, projs, color ? colors.p : nullptr, normal ? normals.p : nullptr}; }
};
// FuseDepthMaps state (pm_fuse.hip).  The working buffers are sized by the largest image (slab) and start over when one grows; the rest lives until the scene is released
struct FuseWork {
	DevBuf<float> depth; DevBuf<uint32_t> claimed, resv; DevBuf<PMFuseCam> cams;
	DevBuf<uint8_t> recN, recColor; DevBuf<float> recX, recWeight, recNormal; DevBuf<uint32_t> recView, recProj;
	DevBuf<uint32_t> pend[2], counters; DevBuf<unsigned long long> nDepthsDev;
	DevBuf<uint2> tileSums, tileOff;
	PinBuf<uint32_t> pin;
	size_t slab = 0;                       // pixels per image the buffers above were allocated for
	// scenes whose views differ in size: every image's normal / confidence / colour gathered into [nImages][slab] arrays, and the sizes
	DevBuf<float> normalS, confS; DevBuf<uint8_t> bgrS; DevBuf<int> dims;
};
struct Fuse : FuseWork {
	DevBuf<uint8_t> bgr; CloudBufs out;
	std::vector<unsigned char> hasBgr;
	uint64_t nPoints = 0, nViews = 0, nDepths = 0, rounds = 0; bool haveColor = false, haveNormal = false;
	bool haveWeight = false;   // the cloud carries view weights (PointCloud::pointWeights not empty): fused with nMinViewsFuse >= 2, or set / loaded with weights
};
// the finishing steps on the fused cloud (pm_cloud.hip): grow-only working buffers, freed with the scene
struct Cloud {
	CloudBufs alt;                                           // the crop's target, swapped with fu.out afterwards
	DevBuf<uint8_t> hole; DevBuf<uint32_t> nxt, cellOf; DevBuf<float4> spts;
	DevBuf<uint2> tileSums, tileOff;
	DevBuf<uint32_t> counts, cellStart;
	DevBuf<PMFuseCam> cams; DevBuf<PMClImg> imgs; DevBuf<uint32_t> used;
	DevBuf<uint32_t> qbuf, obuf;
	DevBuf<uint32_t> misc; DevBuf<float> sample;             // misc: scan totals [0..3], jump flag [4], bounding box [8..13]
	double ms[4] = {0, 0, 0, 0};
	// the visibility filter (pm_cloud_filter.hip): votes of the last filter (indexed as the cloud was before its removal), views in use, cone constants, step times
	DevBuf<int> vis; uint64_t visN = 0; DevBuf<uint32_t> fused;
	std::vector<float> cones; double fms[3] = {0, 0, 0}; DevBuf<unsigned long long> fstats; uint64_t fcount[2] = {0, 0};
};

// What a scene owns (HBM resident, and the pinned staging): pmhip_scene_create and pmhip_release start over from a fresh one
struct SceneMem {
	int nImages = 0;
	DevBuf<float> d_img[4];
	DevBuf<float> d_imgS[4];   // folded anti-diagonal-major copies (PMTask::refS: the reference patch of a sweep visit), w_l*h_l floats per image
	DevBuf<float4> d_imgQ[4];  // anti-diagonal-major quad images (PMSrcView::imgQ): texel (u,v)'s entry at (u+v)*h_l + v, (w_l+h_l-1)*h_l entries of 16 bytes per image
	DevBuf<float> d_depth, d_normal, d_conf, d_snap;
	// geometric rounds: the quad copies (PMSrcView::dqBase) of the depth maps the running call reads as sources, one after the other, 16 bytes per pixel (grow only).
	// The row-major maps stay the truth -- callers write them through pmhip_scene_device_ptr too -- so the copies are derived at the head of every geometric call.
	DevBuf<float4> d_geoQ;
	// ignore masks (nIgnoreMaskLabel): per level [nImages][P_l] bytes, allocated with the first mask; maskMode -1 = on iff a mask is set
	DevBuf<unsigned char> d_mask[4]; std::vector<unsigned char> hasMask; bool maskDirty = false; int maskMode = -1;
	// FilterDepthMap staging: filtered depth/conf of every view (committed after all views are filtered) and splat buffers
	DevBuf<float> d_fdepth, d_fconf; DevBuf<unsigned char> d_fvalid;
	DevBuf<unsigned long long> d_splat; int splatCap = 0; size_t splatPix = 0; DevBuf<PMFTask> d_ftasks; PinBuf<PMFTask> h_ftasks;
	std::vector<SceneView> views;
	Fuse fu;
	Cloud cl;
	// batch scratch (grow only)
	int batchCap = 0;
	int batchW = 0, batchH = 0;   // size the batch scratch was allocated for
	DevBuf<float> d_lvl[4]; // level l>=1: [batch][6][h_l*w_l]; level 0: prior [batch][h*w]
	DevBuf<float> d_old[4]; // tiled sweeps only: [batch][5][h_l*w_l] -- depth, normal, conf as the running sweep found them (PMTask::depthOld ...)
	int oldCap = 0, oldW = 0, oldH = 0;
	DevBuf<PMTask> d_tasks; PinBuf<PMTask> h_tasks;     // [4 levels][batchCap]
	DevBuf<PMUpTask> d_ups; PinBuf<PMUpTask> h_ups;     // [4][batchCap]
};

// The image store (pm_host_image.hip): working-resolution images made on the device from decoded 8-bit images, by caller-chosen key.  Independent of the scene -- images
// are prepared before the scene's slot count is known, so pmhip_scene_create leaves it alone; pmhip_image_drop, pmhip_release and pmhip_destroy free it.
struct ImgEntry { int w = 0, h = 0; DevBuf<uint8_t> bgr; DevBuf<float> gray; };   // bgr: w*h*3 or none (a resampled copy is gray only)
struct ImageStore {
	struct AreaTab { DevBuf<int> ofs, si; DevBuf<float> al; };
	struct CubicTab { DevBuf<int> idx; DevBuf<float> c; };
	std::map<int, ImgEntry> entries;
	DevBuf<uint8_t> src;                          // staging of the decoded image (grow only)
	AreaTab u8x, u8y, fx, fy; CubicTab cx, cy;    // the uploaded tables (grow only); the 8-bit resize keeps its pair while the sizes repeat
	PMImgTab u8tx{}, u8ty{}; int u8Key[4] = {0, 0, 0, 0};
	PMHipImageStats stats{};
};

// The resident mesh (pm_host_mesh.hip) and the working buffers of its renders (grow only, freed with the mesh).  Independent of the scene, like the image store.
#ifndef PM_MESH_BOX_PIXELS
#define PM_MESH_BOX_PIXELS 64          // a face whose clipped box holds more pixels goes to the workgroup route (pmhip_mesh_set_tuning; chosen by tools/mesh_project_bench.py)
#endif
#ifndef PM_MESH_BATCH_BYTES
#define PM_MESH_BATCH_BYTES (4ull << 30)   // device memory of one batch of views: vertex records, face lists, keys and maps
#endif
#define PM_MESH_MAX_BLOCKS 16384       // grid.x of the strided kernels
#define PM_MESH_LARGE_BLOCKS 2048      // workgroups per view that share the listed faces
struct MeshMem {
	DevBuf<float> verts, normals; DevBuf<uint32_t> faces;
	uint32_t nV = 0, nF = 0; bool set = false;
	int boxMax = PM_MESH_BOX_PIXELS; uint64_t batchBytes = PM_MESH_BATCH_BYTES;
	DevBuf<PMMeshView> views; DevBuf<PMMeshVert> rec; DevBuf<unsigned long long> keys; DevBuf<float> depth, normal;
	DevBuf<uint32_t> largeCount, largeList, bits;
	uint64_t statBatches = 0, statLarge = 0; double statMs = 0;
	hipEvent_t ev[2] = {nullptr, nullptr};                   // bracket the clears and kernels of a batch (pmhip_mesh_get_stats)
};

// The image and PLY outputs (pm_host_export.hip): grow-only working buffers, independent of the scene like the image store, and the statistics of the last call
struct ExportMem {
	DevBuf<uint32_t> st;                                     // the selection's state and histogram (PMEX_WORDS)
	DevBuf<float> stage;                                     // values / a depth map from the host
	DevBuf<uint8_t> image, flags, records;                   // the image being made (whole words of four pixels); valid flags and packed records of a view's cloud
	DevBuf<uint2> tileSums, tileOff; DevBuf<uint32_t> totals;
	DevBuf<PMFuseCam> cams; DevBuf<float> scale;
	hipEvent_t ev[2] = {nullptr, nullptr};
	uint64_t launches = 0, us = 0;
};

struct pmhip_engine : SceneMem {
	int device = 0;
	ImageStore img;
	MeshMem mesh;
	ExportMem ex;
	SeedWork seed; DevBuf<float> seedDepth, seedNormal;   // the seed rasteriser (pm_host_seed.hip): its mesh and keys, and the maps of pmhip_seed_raster; independent of the scene
	hipEvent_t imgEv[2] = {nullptr, nullptr};     // bracket every kernel of the store (PMHipImageStats::kernelMs)
	hipStream_t stream = nullptr;
	// view groups of a batch sweep on their own streams so that the tail of one group's diagonal launch
	// overlaps the next launch of another group (views are independent; diagonals of one view are not)
	int nGroups = 1;
	int wideHyps = 0;                        // hypotheses per round of the speculative kernel: 0 = by batch size (8 for one or two views, else 2); PMHipTuning::wideHyps = 8 / 4 / 2 fixes it
	int wideMaxViews = PMHIP_DEFAULT_WIDE;   // batches of at most this many views use the one-wave-per-pixel sweep kernel (PMHIP_WIDE)
	int widePixels = PMHIP_DEFAULT_WIDE_PIXELS;     // in larger batches: a diagonal launch of at most this many pixels (diagonal length x views of the group) uses the two-wide speculative kernel (PMHIP_WIDE_PIXELS)
	int wide8Pixels = PMHIP_DEFAULT_WIDE8_PIXELS;   // ... and one of at most this many pixels the eight-wide one (PMHIP_WIDE8_PIXELS)
	int sweepLanes = PMHIP_DEFAULT_LANES;   // lanes per pixel of the sweep kernel (PMHIP_LANES); the rest of a view's sources go to views-per-lane
	int quadBuffer = 1;                     // tap rows address the level's quad images as one buffer (entry index); 0 = through each view's own pointer (PMHipTuning::quadBuffer; forced for
	                                        // batches that read a source view with its own image size, which lives outside the level's buffer)
	hipStream_t gstream[16] = {};
	hipEvent_t forkEv = nullptr, joinEv[16] = {};
	bool inited = false, geom = false;
	std::string err;
	int w = 0, h = 0, nLevels = 0; // the scene's image size; nLevels = sub-resolution levels available (pyramid has nLevels+1 entries)
	size_t skewPitch(int l) const { return (size_t)(lw(l) + lh(l) - 1) * lh(l); }
	bool pyramidDirty = true;
	int tileW = 0, tileH = 0;                                // pmhip_set_sweep_tiles: 0 = the reference's sweep
	// stats
	bool statsOn = false;
	struct Ev { hipEvent_t a, b; int kind; };
	std::vector<Ev> events;
	PMHipKernelStats stats{};
	// cv::resize(img, img, Size(), 1/2^l, 1/2^l): output size = cvRound(size / 2^l), ties to even (ScaleDepthData, SceneDensify.cpp:586)
	int lw(int l) const { return (int)nearbyint((double)w / (double)(1 << l)); }
	int lh(int l) const { return (int)nearbyint((double)h / (double)(1 << l)); }
	// a view's own size and maps (a view with its own size keeps them itself, SceneView::sw)
	int vw(int i) const { return views[i].sw ? views[i].sw : w; }
	int vh(int i) const { return views[i].sw ? views[i].sh : h; }
	size_t vpix(int i) const { return (size_t)vw(i) * vh(i); }
	float* depthOf(int i) const { return views[i].sw ? views[i].oDepth : d_depth + (size_t)w * h * i; }
	float* normalOf(int i) const { return views[i].sw ? views[i].oNormal : d_normal + (size_t)w * h * 3 * i; }
	float* confOf(int i) const { return views[i].sw ? views[i].oConf : d_conf + (size_t)w * h * i; }
	float* snapOf(int i) const { return views[i].sw ? views[i].oSnap : d_snap + (size_t)w * h * i; }
};

// every buffer of the scene is freed here, by its owner: callers have made the device current and synchronised the stream
static void freeScene(pmhip_engine* e) {
	hipSetDevice(e->device);
	static_cast<SceneMem&>(*e) = SceneMem{};
}

// ... and every buffer of the image store here (its statistics stay)
static void freeImages(pmhip_engine* e) {
	hipSetDevice(e->device);
	const PMHipImageStats kept = e->img.stats;
	e->img = ImageStore{};
	e->img.stats = kept;
}

// ... and the mesh with its working buffers (the tuning is the engine's and stays)
static void freeMesh(pmhip_engine* e) {
	hipSetDevice(e->device);
	const int box = e->mesh.boxMax; const uint64_t bytes = e->mesh.batchBytes;
	for (hipEvent_t ev : e->mesh.ev) if (ev) hipEventDestroy(ev);
	e->mesh = MeshMem{};
	e->mesh.boxMax = box; e->mesh.batchBytes = bytes;
}

// ... and the seed rasteriser's buffers (the tuning stays)
static void freeSeed(pmhip_engine* e) {
	hipSetDevice(e->device);
	e->seed.free(); e->seedDepth.release(); e->seedNormal.release();
}

// ... and the working buffers of the image and PLY outputs
static void freeExport(pmhip_engine* e) {
	hipSetDevice(e->device);
	for (hipEvent_t ev : e->ex.ev) if (ev) hipEventDestroy(ev);
	e->ex = ExportMem{};
}

#include "pm_host_estimate.hip"

static int collectStats(pmhip_engine* e) {
	if (e->events.empty()) return 0;
	HIPCHK(e, hipStreamSynchronize(e->stream));
	for (auto& ev : e->events) {
		float ms = 0; hipEventElapsedTime(&ms, ev.a, ev.b);
		if (ev.kind == 0) e->stats.sweepMs += ms; else if (ev.kind == 2) e->stats.sweepWallMs += ms; else e->stats.initMs += ms;
		hipEventDestroy(ev.a); hipEventDestroy(ev.b);
	}
	e->events.clear();
	return 0;
}

extern "C" {

int pmhip_default_params(PMHipParams* p) {
	if (!p) return PMHIP_E_ARG;
	// libs/MVS/DepthMap.cpp:69-114
	p->nSubResolutionLevels = 2; p->nEstimationIters = 3; p->nEstimationGeometricIters = 2; p->nRandomIters = 6;
	p->fEstimationGeometricWeight = 0.1f; p->fRandomDepthRatio = 0.003f; p->fRandomAngle1Range = 16.f; p->fRandomAngle2Range = 10.f;
	p->fRandomSmoothDepth = 0.02f; p->fRandomSmoothNormal = 13.f; p->fRandomSmoothBonus = 0.93f; p->fNCCThresholdKeep = 0.9f;
	p->fDescriptorMinMagnitudeThreshold = 0.02f; p->seed = 0;
	return 0;
}

int pmhip_create(int device, pmhip_engine** out) {
	if (!out) return PMHIP_E_ARG;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PMHIP_E_NODEVICE;
	if (device < 0) device = 0; // "-1 = best device" (DensifyPointCloud.cpp:112): one GPU per process here
	if (device >= n) return PMHIP_E_NODEVICE;
	pmhip_engine* e = new pmhip_engine();
	e->device = device;
	if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return PMHIP_E_HIP; }
	e->nGroups = PMHIP_DEFAULT_GROUPS;   // (every mapping choice is PMHipTuning's: the library reads no environment)
	for (int g = 0; g < e->nGroups; ++g)
		if (hipStreamCreateWithFlags(&e->gstream[g], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e->joinEv[g], hipEventDisableTiming) != hipSuccess) { delete e; return PMHIP_E_HIP; }
	if (hipEventCreateWithFlags(&e->forkEv, hipEventDisableTiming) != hipSuccess) { delete e; return PMHIP_E_HIP; }
	*out = e;
	return 0;
}

void pmhip_destroy(pmhip_engine* e) {
	if (!e) return;
	hipSetDevice(e->device);
	if (e->stream) hipStreamSynchronize(e->stream);
	for (auto& ev : e->events) { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
	freeScene(e);
	freeImages(e);
	freeMesh(e);
	freeExport(e);
	freeSeed(e);
	for (hipEvent_t ev : e->imgEv) if (ev) hipEventDestroy(ev);
	for (int g = 0; g < 16; ++g) { if (e->gstream[g]) hipStreamDestroy(e->gstream[g]); if (e->joinEv[g]) hipEventDestroy(e->joinEv[g]); }
	if (e->forkEv) hipEventDestroy(e->forkEv);
	if (e->stream) hipStreamDestroy(e->stream);
	delete e;
}

int pmhip_init(pmhip_engine* e, int bGeomConsistency) {
	if (!e) return PMHIP_E_ARG;
	e->inited = true; e->geom = bGeomConsistency != 0;
	return 0;
}

int pmhip_release(pmhip_engine* e) {
	if (!e) return PMHIP_E_ARG;
	hipSetDevice(e->device);
	hipStreamSynchronize(e->stream);
	freeScene(e);
	freeImages(e);
	freeMesh(e);
	freeExport(e);
	freeSeed(e);
	e->inited = false;
	return 0;
}

const char* pmhip_last_error(pmhip_engine* e) { return e ? e->err.c_str() : "null engine"; }

int pmhip_scene_create(pmhip_engine* e, int nImages, int w, int h, int nLevels) {
	if (!e || nImages < 2 || w < 2 * PM_HW + 1 || h < 2 * PM_HW + 1 || nLevels < 0 || nLevels > 3) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	freeScene(e);
	e->nImages = nImages; e->w = w; e->h = h; e->nLevels = nLevels;
	const size_t P0 = (size_t)w * h;
	for (int l = 0; l <= nLevels; ++l) {
		HIPCHK(e, e->d_img[l].alloc((size_t)e->lw(l) * e->lh(l) * nImages));
		HIPCHK(e, e->d_imgS[l].alloc((size_t)e->lw(l) * e->lh(l) * nImages));
		HIPCHK(e, e->d_imgQ[l].alloc(e->skewPitch(l) * nImages));
	}
	HIPCHK(e, e->d_depth.alloc(P0 * nImages));
	HIPCHK(e, e->d_normal.alloc(P0 * 3 * nImages));
	HIPCHK(e, e->d_conf.alloc(P0 * nImages));
	HIPCHK(e, e->d_snap.alloc(P0 * nImages));
	HIPCHK(e, hipMemsetAsync(e->d_depth, 0, sizeof(float) * P0 * nImages, e->stream));
	HIPCHK(e, hipMemsetAsync(e->d_normal, 0, sizeof(float) * P0 * 3 * nImages, e->stream));
	HIPCHK(e, hipMemsetAsync(e->d_conf, 0, sizeof(float) * P0 * nImages, e->stream));
	HIPCHK(e, hipMemsetAsync(e->d_snap, 0, sizeof(float) * P0 * nImages, e->stream));
	e->views.clear(); e->views.resize(nImages);
	for (int i = 0; i < nImages; ++i) e->views[i].id = (uint32_t)i;
	e->pyramidDirty = true;
	return 0;
}

int pmhip_scene_set_view(pmhip_engine* e, int idx, const float* gray, int onDevice, const double K[9], const double R[9], const double C[3],
		float dMin, float dMax, const int32_t* neighbors, int nNeighbors) {
	if (!e || idx < 0 || idx >= e->nImages || !K || !R || !C || nNeighbors < 0 || nNeighbors > PM_MAX_SRC) return PMHIP_E_ARG;
	if (!(dMin > 0) || !(dMin < dMax)) { e->err = "need 0 < dMin < dMax"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	SceneView& v = e->views[idx];
	memcpy(v.K, K, 72); memcpy(v.R, R, 72); memcpy(v.C, C, 24);
	v.dMin = dMin; v.dMax = dMax; v.nNb = nNeighbors;
	for (int k = 0; k < nNeighbors; ++k) v.nb[k] = neighbors[k];
	v.set = true;
	if (gray) {
		if (v.sw) {   // the view goes back to the scene's size: its own pyramid is not needed any more
			HIPCHK(e, hipStreamSynchronize(e->stream));
			v.resetSide(); v.hasMaps = false;
			if (!e->hasMask.empty()) e->hasMask[idx] = 0;
			if (!e->fu.hasBgr.empty()) e->fu.hasBgr[idx] = 0;      // (its colour image went with the side storage)
			// its maps in the scene arrays: "unset", like after pmhip_scene_create (whatever the slot held before the view carried its own size is not an estimate of this image)
			const size_t Ps = (size_t)e->w * e->h;
			HIPCHK(e, hipMemsetAsync(e->d_depth + Ps * idx, 0, sizeof(float) * Ps, e->stream)); HIPCHK(e, hipMemsetAsync(e->d_normal + Ps * 3 * idx, 0, sizeof(float) * Ps * 3, e->stream));
			HIPCHK(e, hipMemsetAsync(e->d_conf + Ps * idx, 0, sizeof(float) * Ps, e->stream)); HIPCHK(e, hipMemsetAsync(e->d_snap + Ps * idx, 0, sizeof(float) * Ps, e->stream));
		}
		const size_t P0 = (size_t)e->w * e->h;
		HIPCHK(e, hipMemcpyAsync(e->d_img[0] + P0 * idx, gray, sizeof(float) * P0, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
		if (!onDevice) HIPCHK(e, hipStreamSynchronize(e->stream)); // caller may free the host buffer
		e->pyramidDirty = true;
	}
	return 0;
}

int pmhip_scene_images_updated(pmhip_engine* e) { if (!e) return PMHIP_E_ARG; e->pyramidDirty = true; return 0; }
uint32_t pmhip_abi_version(void) { return PMHIP_ABI_VERSION; }
int pmhip_get_tuning(pmhip_engine* e, PMHipTuning* out) {
	if (!e || !out) return PMHIP_E_ARG;
	out->viewGroups = e->nGroups; out->wideMaxViews = e->wideMaxViews > 0 ? e->wideMaxViews : -1; out->wideHyps = e->wideHyps > 0 ? e->wideHyps : -1;
	out->sweepLanes = e->sweepLanes > 0 ? e->sweepLanes : -1; out->quadBuffer = e->quadBuffer ? 1 : 2;
	out->widePixels = e->widePixels > 0 ? e->widePixels : -1; out->wide8Pixels = e->wide8Pixels > 0 ? e->wide8Pixels : -1;
	out->reserved0 = 0;
	return 0;
}
int pmhip_set_tuning(pmhip_engine* e, const PMHipTuning* t) {
	if (!e || !t) return PMHIP_E_ARG;
	if (t->viewGroups < 0 || t->viewGroups > 16 || (t->wideHyps > 0 && t->wideHyps != 8 && t->wideHyps != 4 && t->wideHyps != 2) ||
	    (t->sweepLanes > 0 && t->sweepLanes != 4 && t->sweepLanes != 8 && t->sweepLanes != 16) || t->quadBuffer < 0 || t->quadBuffer > 2) { e->err = "pmhip_set_tuning: value out of range"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	if (t->viewGroups > 0) {
		for (int g = e->nGroups; g < t->viewGroups; ++g) if (!e->gstream[g]) {   // streams of the additional view groups
			if (hipStreamCreateWithFlags(&e->gstream[g], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e->joinEv[g], hipEventDisableTiming) != hipSuccess) { e->err = "pmhip_set_tuning: stream"; return PMHIP_E_HIP; }
		}
		e->nGroups = t->viewGroups;
	}
	if (t->wideMaxViews != 0) { e->wideMaxViews = t->wideMaxViews < 0 ? 0 : t->wideMaxViews; if (t->wideMaxViews < 0) e->widePixels = e->wide8Pixels = 0; }   // "never" = no speculative kernels at all, unless this call sets the per-launch rule
	if (t->wideHyps != 0) e->wideHyps = t->wideHyps < 0 ? 0 : t->wideHyps;
	if (t->sweepLanes != 0) e->sweepLanes = t->sweepLanes < 0 ? 0 : t->sweepLanes;
	if (t->quadBuffer != 0) e->quadBuffer = t->quadBuffer == 1;
	if (t->widePixels != 0) e->widePixels = t->widePixels < 0 ? 0 : t->widePixels;
	if (t->wide8Pixels != 0) e->wide8Pixels = t->wide8Pixels < 0 ? 0 : t->wide8Pixels;
	return 0;
}
int pmhip_set_sweep_tiles(pmhip_engine* e, int tileW, int tileH) {
	if (!e || tileW < 0 || tileH < 0 || (tileW > 0) != (tileH > 0) || (tileW > 0 && (tileW < 8 || tileH < 8))) { if (e) e->err = "pmhip_set_sweep_tiles: 0 x 0 (off) or at least 8 x 8"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device)); HIPCHK(e, hipStreamSynchronize(e->stream));
	e->tileW = tileW; e->tileH = tileH;
	return 0;
}
int pmhip_scene_set_view_id(pmhip_engine* e, int idx, uint32_t viewID) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	e->views[idx].id = viewID;
	return 0;
}
int pmhip_scene_maps_updated(pmhip_engine* e, int firstIdx, int count) {
	if (!e || firstIdx < 0 || count < 0 || firstIdx + count > e->nImages) return PMHIP_E_ARG;
	for (int i = firstIdx; i < firstIdx + count; ++i) e->views[i].hasMaps = true;
	return 0;
}


// A source view whose image has its own size (see SceneView::sw): same as pmhip_scene_set_view otherwise.
int pmhip_scene_set_view_sized(pmhip_engine* e, int idx, const float* gray, int w, int h, int onDevice, const double K[9], const double R[9], const double C[3],
		float dMin, float dMax, const int32_t* neighbors, int nNeighbors) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	if (w == e->w && h == e->h) return pmhip_scene_set_view(e, idx, gray, onDevice, K, R, C, dMin, dMax, neighbors, nNeighbors);
	if (!gray || w < 3 || h < 3) { e->err = "a view with its own size needs its image and at least 3 x 3 pixels"; return PMHIP_E_ARG; }
	int rc = pmhip_scene_set_view(e, idx, nullptr, 0, K, R, C, dMin, dMax, neighbors, nNeighbors);
	if (rc) return rc;
	SceneView& v = e->views[idx];
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (v.sw != w || v.sh != h) {
		v.resetSide();
		for (int l = 0; l <= e->nLevels; ++l) {
			const int lw = lvlSize(w, l), lh = lvlSize(h, l);
			if (lw < 1 || lh < 1) break;
			HIPCHK(e, v.sImg[l].alloc((size_t)lw * lh));
			HIPCHK(e, v.sImgS[l].alloc((size_t)lw * lh));
			HIPCHK(e, v.sImgQ[l].alloc((size_t)(lw + lh - 1) * lh));
		}
		// its own maps (DepthData::depthMap / normalMap / confMap of its own size), "unset" like the scene's after pmhip_scene_create
		const size_t P = (size_t)w * h;
		HIPCHK(e, v.oDepth.alloc(P)); HIPCHK(e, v.oNormal.alloc(P * 3));
		HIPCHK(e, v.oConf.alloc(P)); HIPCHK(e, v.oSnap.alloc(P));
		HIPCHK(e, hipMemsetAsync(v.oDepth, 0, sizeof(float) * P, e->stream)); HIPCHK(e, hipMemsetAsync(v.oNormal, 0, sizeof(float) * P * 3, e->stream));
		HIPCHK(e, hipMemsetAsync(v.oConf, 0, sizeof(float) * P, e->stream)); HIPCHK(e, hipMemsetAsync(v.oSnap, 0, sizeof(float) * P, e->stream));
		v.sw = w; v.sh = h; v.hasMaps = false;
		if (!e->hasMask.empty()) e->hasMask[idx] = 0;     // (a mask of the previous size went with the side storage)
	}
	HIPCHK(e, hipMemcpyAsync(v.sImg[0], gray, sizeof(float) * (size_t)w * h, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
	if (!onDevice) HIPCHK(e, hipStreamSynchronize(e->stream));
	v.sideDirty = true;
	return 0;
}

// Known depth-map of view idx for the geometric rounds in which it is a SOURCE view, with the camera it was stored with and its own size
// (DepthData::ViewData::depthMap + cameraDepthMap, SceneDensify.cpp:378-393).  While installed it is read instead of the scene's snapshot of that
// view; depth == NULL removes it.
int pmhip_scene_set_source_depth(pmhip_engine* e, int idx, const float* depth, int dw, int dh, const double Kd[9], const double Rd[9], const double Cd[3]) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	SceneView& v = e->views[idx];
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (!depth) { v.sDepth.release(); v.dw = v.dh = 0; return 0; }
	if (dw < 3 || dh < 3 || !Kd || !Rd || !Cd) return PMHIP_E_ARG;
	if (v.dw != dw || v.dh != dh || !v.sDepth) {
		HIPCHK(e, v.sDepth.alloc((size_t)dw * dh));
		v.dw = dw; v.dh = dh;
	}
	HIPCHK(e, hipMemcpyAsync(v.sDepth, depth, sizeof(float) * (size_t)dw * dh, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	memcpy(v.Kd, Kd, 72); memcpy(v.Rd, Rd, 72); memcpy(v.Cd, Cd, 24);
	return 0;
}

int pmhip_scene_estimate(pmhip_engine* e, const int32_t* viewIds, int nViews, const PMHipParams* p, int nGeometricIter, int sync) {
	if (!e || !viewIds || !p || nViews < 0) return PMHIP_E_ARG;
	if (!e->inited) { e->err = "pmhip_init not called"; return PMHIP_E_STATE; }
	HIPCHK(e, hipSetDevice(e->device));
	int rc = estimateBatch(e, viewIds, nViews, *p, nGeometricIter);
	if (rc) return rc;
	if (sync) HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int pmhip_scene_commit_round(pmhip_engine* e) {
	if (!e || !e->d_snap) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipMemcpyAsync(e->d_snap, e->d_depth, sizeof(float) * (size_t)e->w * e->h * e->nImages, hipMemcpyDeviceToDevice, e->stream));
	for (const SceneView& v : e->views) if (v.sw) HIPCHK(e, hipMemcpyAsync(v.oSnap, v.oDepth, sizeof(float) * (size_t)v.sw * v.sh, hipMemcpyDeviceToDevice, e->stream));
	return 0;
}

int pmhip_scene_reset_view(pmhip_engine* e, int idx) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = e->vpix(idx);
	HIPCHK(e, hipMemsetAsync(e->depthOf(idx), 0, sizeof(float) * P0, e->stream));
	HIPCHK(e, hipMemsetAsync(e->normalOf(idx), 0, sizeof(float) * P0 * 3, e->stream));
	HIPCHK(e, hipMemsetAsync(e->confOf(idx), 0, sizeof(float) * P0, e->stream));
	e->views[idx].hasMaps = false;
	return 0;
}

int pmhip_scene_set_maps(pmhip_engine* e, int idx, const float* depth, const float* normal) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = e->vpix(idx);
	if (depth) HIPCHK(e, hipMemcpyAsync(e->depthOf(idx), depth, sizeof(float) * P0, hipMemcpyHostToDevice, e->stream));
	if (normal) HIPCHK(e, hipMemcpyAsync(e->normalOf(idx), normal, sizeof(float) * P0 * 3, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (depth) e->views[idx].hasMaps = true;
	return 0;
}

int pmhip_scene_set_mask(pmhip_engine* e, int idx, const unsigned char* mask) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = (size_t)e->w * e->h;
	if (e->hasMask.empty()) e->hasMask.assign(e->nImages, 0);
	if (!mask) { e->hasMask[idx] = 0; return 0; }
	if (e->views[idx].sw) {                       // a view with its own size keeps its own masks
		SceneView& v = e->views[idx];
		for (int l = 0; l <= e->nLevels; ++l) {
			const int mlw = lvlSize(v.sw, l), mlh = lvlSize(v.sh, l);
			if (mlw < 1 || mlh < 1) break;
			if (!v.oMask[l]) HIPCHK(e, v.oMask[l].alloc((size_t)mlw * mlh));
		}
		HIPCHK(e, hipMemcpyAsync(v.oMask[0], mask, (size_t)v.sw * v.sh, hipMemcpyHostToDevice, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		e->hasMask[idx] = 1; e->maskDirty = true;
		return 0;
	}
	if (!e->d_mask[0]) for (int l = 0; l <= e->nLevels; ++l) HIPCHK(e, e->d_mask[l].alloc((size_t)e->lw(l) * e->lh(l) * e->nImages));
	HIPCHK(e, hipMemcpyAsync(e->d_mask[0] + P0 * idx, mask, P0, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	e->hasMask[idx] = 1; e->maskDirty = true;
	return 0;
}
int pmhip_scene_set_mask_mode(pmhip_engine* e, int mode) {
	if (!e || mode < -1 || mode > 1) return PMHIP_E_ARG;
	e->maskMode = mode;
	return 0;
}

int pmhip_scene_set_conf(pmhip_engine* e, int idx, const float* conf) {
	if (!e || !conf || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = e->vpix(idx);
	HIPCHK(e, hipMemcpyAsync(e->confOf(idx), conf, sizeof(float) * P0, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int pmhip_scene_get_maps(pmhip_engine* e, int idx, float* depth, float* normal, float* conf) {
	if (!e || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = e->vpix(idx);   // (a view with its own size returns maps of that size)
	if (depth) HIPCHK(e, hipMemcpyAsync(depth, e->depthOf(idx), sizeof(float) * P0, hipMemcpyDeviceToHost, e->stream));
	if (normal) HIPCHK(e, hipMemcpyAsync(normal, e->normalOf(idx), sizeof(float) * P0 * 3, hipMemcpyDeviceToHost, e->stream));
	if (conf) HIPCHK(e, hipMemcpyAsync(conf, e->confOf(idx), sizeof(float) * P0, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

void* pmhip_scene_device_ptr(pmhip_engine* e, int what, int idx) {
	if (!e || idx < 0 || idx >= e->nImages) return nullptr;
	const size_t P0 = (size_t)e->w * e->h;
	switch (what) {
	case 0: return e->views[idx].sw ? e->views[idx].sImg[0] : e->d_img[0] + P0 * idx;
	case 1: return e->depthOf(idx);
	case 2: return e->normalOf(idx);
	case 3: return e->confOf(idx);
	case 4: return e->snapOf(idx);
	default: return nullptr;
	}
}

int pmhip_scene_copy(pmhip_engine* e, int what, int firstIdx, int count, void* devPtr, int toEngine) {
	if (!e || !devPtr || count <= 0 || firstIdx < 0 || firstIdx + count > e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	char* base = (char*)pmhip_scene_device_ptr(e, what, firstIdx);
	if (!base) return PMHIP_E_ARG;
	bool sized = false;
	for (int i = firstIdx; i < firstIdx + count; ++i) sized = sized || e->views[i].sw;
	if (sized && count > 1) { e->err = "pmhip_scene_copy: a range that contains a view with its own size must be copied view by view"; return PMHIP_E_SIZE; }
	const size_t bytes = sizeof(float) * (sized ? e->vpix(firstIdx) : (size_t)e->w * e->h * count) * (what == 2 ? 3 : 1);
	if (sized && toEngine && what == 0) e->views[firstIdx].sideDirty = true;
	HIPCHK(e, hipMemcpyAsync(toEngine ? (void*)base : devPtr, toEngine ? devPtr : (void*)base, bytes, hipMemcpyDeviceToDevice, e->stream));
	if (toEngine && what == 0) e->pyramidDirty = true;
	if (toEngine && what == 1) for (int i = firstIdx; i < firstIdx + count; ++i) e->views[i].hasMaps = true;   // depth maps gathered from other ranks
	return 0;
}

// HBM the scene holds right now: image pyramids with their quad layouts, the four map arrays, masks, the filter's staging, the batch scratch of the largest batch estimated
// so far, and the own storage of views that carry their own size.  Not the working buffers of pmhip_scene_fuse (they live only during fusion and its download).
uint64_t pmhip_scene_bytes(pmhip_engine* e) {
	if (!e || e->nImages <= 0) return 0;
	const size_t N = (size_t)e->nImages, P0 = (size_t)e->w * e->h;
	size_t b = 0;
	for (int l = 0; l <= e->nLevels; ++l) {
		if (e->d_img[l]) b += sizeof(float) * (size_t)e->lw(l) * e->lh(l) * N * 2;   // row-major + folded anti-diagonal-major
		if (e->d_imgQ[l]) b += sizeof(float4) * e->skewPitch(l) * N;
		if (e->d_mask[l]) b += (size_t)e->lw(l) * e->lh(l) * N;
	}
	if (e->d_depth) b += sizeof(float) * P0 * N * 6;                       // depth, normal (3), confidence, previous round's depth
	b += sizeof(float4) * e->d_geoQ.n;                                     // quad copies of the source depth maps of the geometric rounds
	if (e->d_fdepth) b += sizeof(float) * P0 * N * 2 + P0 * N;             // FilterDepthMap staging
	if (e->d_splat) b += sizeof(unsigned long long) * e->splatPix * PMF_MAXN * (size_t)e->splatCap;
	if (e->batchCap) {
		b += sizeof(float) * (size_t)e->batchCap * e->batchW * e->batchH;
		for (int l = 1; l <= e->nLevels; ++l) b += sizeof(float) * (size_t)e->batchCap * 6 * lvlSize(e->batchW, l) * lvlSize(e->batchH, l);
		b += (sizeof(PMTask) + sizeof(PMUpTask)) * 4 * (size_t)e->batchCap;
	}
	for (const SceneView& v : e->views) {
		if (v.sDepth) b += sizeof(float) * (size_t)v.dw * v.dh;
		if (!v.sw) continue;
		const size_t P = (size_t)v.sw * v.sh;
		b += sizeof(float) * P * 6 + (v.oFDepth ? sizeof(float) * P * 2 : 0) + (v.oBgr ? 3 * P : 0);
		for (int l = 0; l <= e->nLevels; ++l) {
			const size_t lw = (size_t)lvlSize(v.sw, l), lh = (size_t)lvlSize(v.sh, l);
			if (v.sImg[l]) b += sizeof(float) * lw * lh * 2;
			if (v.sImgQ[l]) b += sizeof(float4) * (lw + lh - 1) * lh;
			if (v.oMask[l]) b += lw * lh;
		}
	}
	return (uint64_t)b;
}

int pmhip_sync(pmhip_engine* e) { if (!e) return PMHIP_E_ARG; HIPCHK(e, hipSetDevice(e->device)); HIPCHK(e, hipStreamSynchronize(e->stream)); return 0; }
void* pmhip_stream(pmhip_engine* e) { return e ? (void*)e->stream : nullptr; }

int pmhip_stats_reset(pmhip_engine* e, int enableEvents) {
	if (!e) return PMHIP_E_ARG;
	hipSetDevice(e->device);
	collectStats(e);
	memset(&e->stats, 0, sizeof(e->stats));
	e->statsOn = enableEvents != 0;
	return 0;
}
int pmhip_stats_get(pmhip_engine* e, PMHipKernelStats* out) {
	if (!e || !out) return PMHIP_E_ARG;
	hipSetDevice(e->device);
	int rc = collectStats(e); if (rc) return rc;
	*out = e->stats;
	return 0;
}

// PatchMatchCUDA::EstimateDepthMap(DepthData&), libs/MVS/PatchMatchCUDA.cpp:174-416 -- host buffers in, host buffers out.
int pmhip_estimate_depth_map(pmhip_engine* e, PMHipDepthData* dd, const PMHipParams* p, int nGeometricIter) {
	return pmhip_estimate_depth_map_masked(e, dd, nullptr, 0, p, nGeometricIter);
}
// ... with DepthData::mask (libs/MVS/DepthMap.h:211; filled by DepthEstimator::ImportIgnoreMask, applied in SceneDensify.cpp:656-683)
int pmhip_estimate_depth_map_masked(pmhip_engine* e, PMHipDepthData* dd, const unsigned char* mask, int maskOption, const PMHipParams* p, int nGeometricIter) {
	if (!e || !dd || !p || !dd->views || dd->nViews < 2 || dd->nViews > 1 + PM_MAX_SRC || !dd->depthMap || !dd->normalMap || !dd->confMap) return PMHIP_E_ARG;
	if (!e->inited) { e->err = "pmhip_init not called"; return PMHIP_E_STATE; }
	const int w = dd->views[0].w, h = dd->views[0].h, n = dd->nViews;
	for (int i = 0; i < n; ++i) {
		if (!dd->views[i].image || dd->views[i].w < 3 || dd->views[i].h < 3) return PMHIP_E_ARG;
		if (nGeometricIter >= 0 && i > 0 && !dd->views[i].depth) { e->err = "geometric round needs views[i].depth"; return PMHIP_E_ARG; }
	}
	const int S = (int)p->nSubResolutionLevels;
	if (S > 3) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	// keep device buffers between calls; re-allocate only when geometry changes (reference: PatchMatchCUDA.cpp:264-322)
	if (e->nImages != n || e->w != w || e->h != h || e->nLevels < S) {
		int rc = pmhip_scene_create(e, n, w, h, std::max(S, e->nImages == n && e->w == w && e->h == h ? e->nLevels : 0));
		if (rc) return rc;
	}
	const size_t P0 = (size_t)w * h;
	int32_t nb[PM_MAX_SRC];
	for (int i = 1; i < n; ++i) nb[i - 1] = i;
	for (int i = 0; i < n; ++i) {
		const PMHipView& v = dd->views[i];
		// source views may come in any size (neighbours rescaled by ViewData::ScaleImage, DepthMap.h:194-204): they keep their own pyramid
		int rc = pmhip_scene_set_view_sized(e, i, v.image, v.w, v.h, 0, v.K, v.R, v.C, dd->dMin, dd->dMax, nb, i == 0 ? n - 1 : 0);
		if (rc) return rc;
		e->views[i].id = v.id;
		if (i == 0) continue;
		if (nGeometricIter < 0) { if (e->views[i].sDepth) { rc = pmhip_scene_set_source_depth(e, i, nullptr, 0, 0, nullptr, nullptr, nullptr); if (rc) return rc; } continue; }
		// the known depth-map is read with the camera stored next to it (cameraDepthMap) and has its own size; an all-zero Kd / Rd means
		// "not filled in" and stands for the view's own camera
		bool zero = true; for (int k = 0; k < 9; ++k) zero = zero && v.Kd[k] == 0.0 && v.Rd[k] == 0.0;
		const int dw = v.dw > 0 ? v.dw : v.w, dh = v.dh > 0 ? v.dh : v.h;
		const bool own = zero || (!memcmp(v.Kd, v.K, 72) && !memcmp(v.Rd, v.R, 72) && !memcmp(v.Cd, v.C, 24));
		if (own && dw == w && dh == h && v.w == w && v.h == h) {
			if (e->views[i].sDepth) { rc = pmhip_scene_set_source_depth(e, i, nullptr, 0, 0, nullptr, nullptr, nullptr); if (rc) return rc; }
			HIPCHK(e, hipMemcpyAsync(e->d_snap + P0 * i, v.depth, sizeof(float) * P0, hipMemcpyHostToDevice, e->stream));
		} else {
			rc = pmhip_scene_set_source_depth(e, i, v.depth, dw, dh, zero ? v.K : v.Kd, zero ? v.R : v.Rd, zero ? v.C : v.Cd);
			if (rc) return rc;
		}
	}
	int rc = pmhip_scene_set_maps(e, 0, dd->depthMap, dd->normalMap);
	if (rc) return rc;
	// the engine is reused between calls: install this call's mask state and leave none behind
	rc = pmhip_scene_set_mask(e, 0, mask);
	if (rc) return rc;
	const int savedMode = e->maskMode;
	e->maskMode = mask ? -1 : (maskOption ? 1 : 0);
	const int32_t id0 = 0;
	rc = estimateBatch(e, &id0, 1, *p, nGeometricIter);
	e->maskMode = savedMode;
	if (mask) pmhip_scene_set_mask(e, 0, nullptr);
	if (rc) return rc;
	return pmhip_scene_get_maps(e, 0, dd->depthMap, dd->normalMap, dd->confMap);
}

// in-kernel phase counters (only populated by -DPM_PROFILE builds); reset != 0 clears them after reading
int pmhip_prof_get(pmhip_engine* e, unsigned long long out16[16], int reset) {
	if (!e || !out16) return PMHIP_E_ARG;
#ifdef PM_PROFILE
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpyFromSymbol(out16, HIP_SYMBOL(pm_prof), sizeof(unsigned long long) * 16));
	if (reset) { unsigned long long z[16] = {0}; HIPCHK(e, hipMemcpyToSymbol(HIP_SYMBOL(pm_prof), z, sizeof(z))); }
	return 0;
#else
	for (int i = 0; i < 16; ++i) out16[i] = 0;
	return 0;
#endif
}

#ifdef PM_PROFILE
// (profile builds only, tools/phase_prof.py) histogram of pm_visit's trips by the number of pixels of the wave that take part
int pmhip_prof_hist(pmhip_engine* e, unsigned long long out17[17], int reset) {
	if (!e || !out17) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpyFromSymbol(out17, HIP_SYMBOL(pm_hist), sizeof(unsigned long long) * 17));
	if (reset) { unsigned long long z[17] = {0}; HIPCHK(e, hipMemcpyToSymbol(HIP_SYMBOL(pm_hist), z, sizeof(z))); }
	return 0;
}
#endif

int pmhip_math_eval(pmhip_engine* e, int kind, const float* a, const float* b, float* out, size_t n) {
	if (!e || !a || !out || n == 0) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	DevBuf<float> da, db, dout;
	HIPCHK(e, da.alloc(n)); HIPCHK(e, db.alloc(n)); HIPCHK(e, dout.alloc(n));
	HIPCHK(e, hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice));
	HIPCHK(e, hipMemcpy(db, b ? b : a, n * 4, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(pm_math_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, e->stream, kind, da, db, dout, n);
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
	return 0;
}

int pmhip_resize(pmhip_engine* e, int kind, const float* src, int w, int h, int arg, float* dst) {
	if (!e || !src || !dst || w <= 0 || h <= 0) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t ns = (size_t)w * h;
	int dw, dh;
	if (kind == 0) { if (arg < 1) return PMHIP_E_SIZE; dw = (int)nearbyint((double)w / arg); dh = (int)nearbyint((double)h / arg); } else { dw = w * 2; dh = h * 2; }
	const size_t nd = (size_t)dw * dh;
	DevBuf<float> ds, dd, dn, dn2, dp; DevBuf<PMUpTask> du;
	HIPCHK(e, ds.alloc(ns)); HIPCHK(e, dd.alloc(nd));
	HIPCHK(e, hipMemcpy(ds, src, ns * 4, hipMemcpyHostToDevice));
	if (kind == 0) {
		launchArea(e->stream, ds, dd, w, h, dw, dh, arg, 1);
	} else if (kind == 1) {
		HIPCHK(e, dn.alloc(ns * 3)); HIPCHK(e, dn2.alloc(nd * 3)); HIPCHK(e, dp.alloc(nd)); HIPCHK(e, du.alloc(1));
		HIPCHK(e, hipMemset(dn, 0, ns * 12));
		PMUpTask u{ds, dn, dd, dn2, dp};
		HIPCHK(e, hipMemcpy(du, &u, sizeof(u), hipMemcpyHostToDevice));
		launchUpsample(e->stream, du, 1, w, h, dw, dh, 0);
	} else {
		launchNearestUpF(e->stream, ds, dd, w, h, dw, dh);
	}
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpy(dst, dd, nd * 4, hipMemcpyDeviceToHost));
	return 0;
}

// One resampler once, on host buffers, through the launch helper the estimation uses (pm_host_estimate.hip).  The destination is uploaded before the launch and
// read back whole, so whatever the caller put into the entries a kernel does not write (a quad image's unused corners) comes back untouched -- or not.
int pmhip_resample(pmhip_engine* e, int kind, const void* src, int sw, int sh, void* dst, int dw, int dh, int arg, int nImg) {
	if (!e || !src || !dst) return PMHIP_E_ARG;
	if (kind < PMHIP_RESAMPLE_AREA || kind > PMHIP_RESAMPLE_DEPTH_QUADS) { e->err = "pmhip_resample: unknown kind"; return PMHIP_E_ARG; }
	if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || nImg < 1) { e->err = "pmhip_resample: empty image"; return PMHIP_E_SIZE; }
	const bool factor = kind == PMHIP_RESAMPLE_AREA || kind == PMHIP_RESAMPLE_NEAREST_DOWN, same = kind == PMHIP_RESAMPLE_SKEW || kind == PMHIP_RESAMPLE_QUAD || kind == PMHIP_RESAMPLE_DEPTH_QUADS;
	if (factor && (arg < 1 || dw != (int)nearbyint((double)sw / arg) || dh != (int)nearbyint((double)sh / arg))) { e->err = "pmhip_resample: the destination is not cvRound(size / factor)"; return PMHIP_E_SIZE; }
	if (same && (dw != sw || dh != sh)) { e->err = "pmhip_resample: skew and quad keep the size"; return PMHIP_E_SIZE; }
	if (kind == PMHIP_RESAMPLE_DEPTH_QUADS && (nImg != 1 || sw < 2 || sh < 2)) { e->err = "pmhip_resample: one depth map of at least 2 x 2"; return PMHIP_E_SIZE; }
	if (nImg != 1 && !(kind == PMHIP_RESAMPLE_AREA || same)) { e->err = "pmhip_resample: one image for this kind"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	const size_t ps = (size_t)sw * sh, pd = (size_t)dw * dh;
	// bytes of the two buffers, by kind (include/pmhip.h)
	size_t bs = ps * 4 * nImg, bd = pd * 4 * nImg;
	switch (kind) {
	case PMHIP_RESAMPLE_UPSAMPLE: bs = ps * 16; bd = pd * 20; break;
	case PMHIP_RESAMPLE_NEAREST_DOWN: bs = ps * 16; bd = pd * 16; break;
	case PMHIP_RESAMPLE_MASK_LEVEL: bs = ps; bd = pd; break;
	case PMHIP_RESAMPLE_QUAD: bd = (size_t)(dw + dh - 1) * dh * 16 * nImg; break;
	case PMHIP_RESAMPLE_DEPTH_QUADS: bd = pd * 16; break;
	default: break;
	}
	DevBuf<unsigned char> ds, dd; DevBuf<PMUpTask> du;
	HIPCHK(e, ds.alloc(bs)); HIPCHK(e, dd.alloc(bd));
	HIPCHK(e, hipMemcpy(ds, src, bs, hipMemcpyHostToDevice));
	HIPCHK(e, hipMemcpy(dd, dst, bd, hipMemcpyHostToDevice));
	const float* fs = (const float*)(const unsigned char*)ds; float* fd = (float*)(unsigned char*)dd;
	switch (kind) {
	case PMHIP_RESAMPLE_AREA: launchArea(e->stream, fs, fd, sw, sh, dw, dh, arg, nImg); break;
	case PMHIP_RESAMPLE_UPSAMPLE: case PMHIP_RESAMPLE_NEAREST_DOWN: {
		PMUpTask u{fs, fs + ps, fd, fd + pd, kind == PMHIP_RESAMPLE_UPSAMPLE ? fd + pd * 4 : nullptr};
		HIPCHK(e, du.alloc(1));
		HIPCHK(e, hipMemcpy(du, &u, sizeof(u), hipMemcpyHostToDevice));
		if (kind == PMHIP_RESAMPLE_UPSAMPLE) launchUpsample(e->stream, du, 1, sw, sh, dw, dh, arg ? 1 : 0);
		else launchNearestDown(e->stream, du, 1, sw, sh, dw, dh, arg);
	} break;
	case PMHIP_RESAMPLE_NEAREST_UP: launchNearestUpF(e->stream, fs, fd, sw, sh, dw, dh); break;
	case PMHIP_RESAMPLE_MASK_LEVEL: launchMaskLevel(e->stream, ds, dd, sw, sh, dw, dh); break;
	case PMHIP_RESAMPLE_SKEW: launchSkew(e->stream, fs, fd, sw, sh, nImg); break;
	case PMHIP_RESAMPLE_DEPTH_QUADS: launchDepthQuads(e->stream, fs, (float4*)fd, sw, sh); break;
	default: launchQuad(e->stream, fs, (float4*)fd, sw, sh, nImg); break;
	}
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpy(dst, dd, bd, hipMemcpyDeviceToHost));
	return 0;
}

} // extern "C"

#include "pm_host_filter.hip"
#include "pm_host_fuse.hip"
#include "pm_host_cloud.hip"
#include "pm_host_image.hip"
#include "pm_host_normal.hip"
#include "pm_host_mesh.hip"
#include "pm_host_export.hip"
#include "pm_host_seed.hip"
