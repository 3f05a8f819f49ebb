// DenseDepthMapsHIP.hpp -- header-only C++ driver of the HBM-resident scene interface (include/pmhip.h, section 2) with the shape of
// Scene::ComputeDepthMaps + Scene::DenseReconstruction (libs/MVS/SceneDensify.cpp:1754-1982, :1655-1750): upload the views once, estimate ALL
// depth maps of a round concurrently (that is what fills an MI355X: the per-view seam at SceneDensify.cpp:618-623 hands the GPU one depth
// map at a time), keep every map on the device between the photometric pass, the geometric-consistency rounds, the per-map post-filters,
// the cross-view filter and the fusion, and come back to the host only with what the caller asks for (maps, .dmap files, the fused cloud).
//
// The reference's loop and what replaces it (see INTEGRATION.md section 1b for the call-site patch):
//   :1884-1905  photometric pass, one EstimateDepthMap per image on a worker queue      -> Estimate(-1)            (one pmhip_scene_estimate)
//   :1906-1953  for each geometric iteration: re-load neighbours' .dmap, estimate, save  -> CommitRound(); Estimate(iter)
//   :1884-1886,1919-1920 + :2069-2093  nOptimize: REMOVE_SPECKLES, FILL_GAPS             -> PostFilter()
//   :1955-1980 / :2136-2222  ADJUST_FILTER: DenseReconstructionFilter                    -> FilterDepthMaps()
//   :1695-1712 / :1372-1650  FuseDepthMaps (or MergeDepthMaps when nMinViewsFuse < 2)    -> FuseDepthMaps()
//   :411-414    a .dmap stored without normals: EstimateNormalMap from its depths         -> SetDepthMap(); EstimateMissingNormals()
//   Mesh::Project (Mesh.cpp:3874-3968) of --mesh-file / --export-depth-maps-name          -> SetMesh(); ProjectMesh(); ReleaseMesh()
//   DepthData::Save (DepthMap.cpp:234-252)                                                -> SaveDepthMaps() through include/dmapio.h
//   :2099-2110, :2201-2206  the images and clouds of verbosity 3 and above                -> DepthImage(); ConfImage(); NormalImage(); ViewCloud()
//   PointCloud::Save / SaveNViews / SaveWithScale (PointCloud.cpp:361-539)                 -> SavePointCloud()
//
// Needs nothing of OpenMVS / OpenCV: views are described by plain pointers (an OpenMVS caller fills them from MVS::Image / DepthData,
// libs/MVS/DepthMap.h:157-271).  Throws std::runtime_error with the engine's message on any error, like PatchMatchHIP.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cfloat>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "pmhip.h"

namespace MVS {

class DenseDepthMapsHIP {
public:
	// OPTDENSE::DepthFlags, libs/MVS/DepthMap.h:87-92
	enum DepthFlags { REMOVE_SPECKLES = 1, FILL_GAPS = 2, ADJUST_FILTER = 4, OPTIMIZE = REMOVE_SPECKLES | FILL_GAPS | ADJUST_FILTER };

	struct Options : PMHipParams {
		// defaults of libs/MVS/DepthMap.cpp:69-114
		unsigned nOptimize = OPTIMIZE;
		unsigned nSpeckleSize = 100, nIpolGapSize = 7;
		float fDepthDiffThreshold = 0.01f, fNormalDiffThreshold = 25.f;
		unsigned nMinViewsFilter = 2, nMinViewsFilterAdjust = 1, nMinViewsFuse = 2;
		bool bFilterAdjust = true, bEstimateColor = true, bEstimateNormal = true;
		// the finishing steps after the fusion (FinishPointCloud, SceneDensify.cpp:1733-1736): EstimatePointColors / EstimatePointNormals when the cloud has
		// none -- OPTDENSE::nEstimateColors == 1 / nEstimateNormals == 1; nNeighbors = the k of the PCA normals
		bool bPointColors = false, bPointNormals = false;
		int nNeighbors = 16;
		Options() { pmhip_default_params(this); }
	};

	// one calibrated image (MVS::Image + the DepthData the reference builds for it in InitViews, SceneDensify.cpp:273-460)
	struct View {
		int w = 0, h = 0;                       // this image's own size; 0 = the size given to LoadScene (the reference sizes every DepthData on its image, SceneDensify.cpp:306-459)
		const float* gray = nullptr;            // w*h, gray in [0,1] (Image::toGray), row-major
		const unsigned char* bgr = nullptr;     // w*h*3 or null (needed for FuseDepthMaps with bEstimateColor)
		const unsigned char* mask = nullptr;    // w*h or null: 0 = ignored pixel (--ignore-mask-label, DepthMap.cpp:296-323)
		// Instead of `gray` and `bgr`: the decoded 8-bit image at its stored size, W0*H0*3 bytes, channelOrder 0 = B,G,R / 1 = R,G,B.  The device brings it to this view's
		// working size (Image::ResizeImage; see WorkingSize) and converts it (TImage::toGray) through the engine's image store: a host without OpenMVS needs neither
		// (pmhip_image_prepare, pmhip_scene_set_view_stored).  The image is read during LoadScene only.
		const unsigned char* image8 = nullptr; int W0 = 0, H0 = 0, channelOrder = 0;
		double K[9], R[9], C[3];                // pixel camera of this image: x = K R (X - C)
		float dMin = 0, dMax = 0;               // depth range of the sparse points seen by the view (DepthData::dMin/dMax)
		std::vector<int32_t> neighbors;         // indices into the view array, best first (DepthData::neighbors after SelectViews)
		const float* initDepth = nullptr;       // optional initial estimate (InitDepthMap, SceneDensify.cpp:418-460), w*h
		const float* initNormal = nullptr;      // w*h*3
		uint32_t ID = 0;                        // Image::ID as stored in the .dmap (the engine numbers views by their index in the array)
		float connections = -1.f;               // Image::neighbors.size() (all scored neighbours): fusion order; < 0 = use neighbors.size()
		std::string name;                       // image file name as stored in the .dmap
	};

	struct PointCloud {                         // MVS::PointCloud (libs/MVS/PointCloud.h): CSR view lists
		std::vector<float> points, weights, normals;
		std::vector<uint32_t> viewStart, views;
		std::vector<uint16_t> projs;
		std::vector<unsigned char> colors;
		size_t size() const { return points.size() / 3; }
	};

	explicit DenseDepthMapsHIP(int device = 0) : e_(nullptr), w_(0), h_(0) {
		if (pmhip_create(device, &e_) != PMHIP_OK) e_ = nullptr;   // IsValid() == false -> the caller keeps the CPU path (SceneDensify.cpp:1876-1877)
	}
	~DenseDepthMapsHIP() { if (e_) pmhip_destroy(e_); }
	DenseDepthMapsHIP(const DenseDepthMapsHIP&) = delete;
	DenseDepthMapsHIP& operator=(const DenseDepthMapsHIP&) = delete;
	bool IsValid() const { return e_ != nullptr; }

	// Upload the scene: every image once, for all rounds (the reference re-reads images and neighbours' depth maps per depth map).
	void LoadScene(const std::vector<View>& views, int w, int h, const Options& opt) {
		views_ = views; w_ = w; h_ = h; opt_ = opt;
		const int n = (int)views.size();
		check(pmhip_init(e_, 0));
		check(pmhip_scene_create(e_, n, w, h, (int)opt.nSubResolutionLevels));
		bool anyMask = false;
		for (int i = 0; i < n; ++i) {
			const View& v = views[i];
			if (v.image8) {                                                     // decoded image -> store entry i -> the view's own copies; the entry goes at once
				check(pmhip_image_prepare(e_, i, v.image8, v.W0, v.H0, v.channelOrder, v.w > 0 ? v.w : w, v.h > 0 ? v.h : h));
				check(pmhip_scene_set_view_stored(e_, i, i, v.K, v.R, v.C, v.dMin, v.dMax, v.neighbors.data(), (int)v.neighbors.size()));
				check(pmhip_image_drop(e_, i));
				if (v.mask) { check(pmhip_scene_set_mask(e_, i, v.mask)); anyMask = true; }
				continue;
			}
			if (!v.gray) throw std::runtime_error("DenseDepthMapsHIP: view without an image");
			if (v.w > 0 && v.h > 0 && (v.w != w || v.h != h))
				check(pmhip_scene_set_view_sized(e_, i, v.gray, v.w, v.h, 0, v.K, v.R, v.C, v.dMin, v.dMax, v.neighbors.data(), (int)v.neighbors.size()));
			else
				check(pmhip_scene_set_view(e_, i, v.gray, 0, v.K, v.R, v.C, v.dMin, v.dMax, v.neighbors.data(), (int)v.neighbors.size()));
			if (v.mask) { check(pmhip_scene_set_mask(e_, i, v.mask)); anyMask = true; }
			if (v.bgr) check(pmhip_scene_set_color(e_, i, v.bgr));
		}
		(void)anyMask;
		ids_.resize((size_t)n);
		for (int i = 0; i < n; ++i) ids_[(size_t)i] = i;
		noNormals_.clear();
	}

	// The size Image::ResizeImage brings a W0 x H0 image to under OPTDENSE::nResolutionLevel / nMinResolution / nMaxResolution (pmhip_working_size): View::w, View::h of
	// a view given as image8, and the size its camera is scaled to (Image::UpdateCamera; mvsf_camera of include/mvsfront.h)
	static void WorkingSize(int W0, int H0, unsigned nResolutionLevel, unsigned nMinResolution, unsigned nMaxResolution, int& w, int& h) {
		if (pmhip_working_size(W0, H0, nResolutionLevel, nMinResolution, nMaxResolution, &w, &h) != PMHIP_OK) throw std::runtime_error("DenseDepthMapsHIP: bad image size");
	}

	// Scene::ComputeDepthMaps: all rounds for all views, then the post-filters the option bits ask for.  Returns the number of depth maps.
	size_t ComputeDepthMaps() {
		const int n = (int)ids_.size();
		const unsigned G = opt_.nEstimationGeometricIters;
		check(pmhip_init(e_, 0));
		for (int i = 0; i < n; ++i) {
			check(pmhip_scene_reset_view(e_, i));
			const View& v = views_[(size_t)i];
			if (v.initDepth) check(pmhip_scene_set_maps(e_, i, v.initDepth, v.initNormal));
		}
		check(pmhip_scene_estimate(e_, ids_.data(), n, &opt_, -1, 0));                // photometric pass, SceneDensify.cpp:1884-1905
		if (G == 0) PostFilter();
		for (unsigned g = 0; g < G; ++g) {                                             // :1906-1953
			check(pmhip_scene_commit_round(e_));                                       // "save depthNNNN.dmap, reload as neighbour"
			check(pmhip_init(e_, 1));                                                  // pmCUDA->Release(); Init(true), :1910-1916
			check(pmhip_scene_estimate(e_, ids_.data(), n, &opt_, (int)g, 0));
			if (g + 1 == G) PostFilter();
		}
		if (opt_.nOptimize & ADJUST_FILTER) FilterDepthMaps();                         // :1955-1980
		check(pmhip_sync(e_));
		return (size_t)n;
	}

	// nOptimize bits applied to every depth map after the last estimation round (:1884-1886, :1919-1920, :2069-2093)
	void PostFilter() {
		const int n = (int)ids_.size();
		if (opt_.nOptimize & REMOVE_SPECKLES) check(pmhip_scene_remove_small_segments(e_, ids_.data(), n, opt_.nSpeckleSize, opt_.fDepthDiffThreshold));
		if (opt_.nOptimize & FILL_GAPS) check(pmhip_scene_gap_interpolation(e_, ids_.data(), n, opt_.nIpolGapSize, opt_.fDepthDiffThreshold));
	}
	// Scene::DenseReconstructionFilter, :2136-2222: every map against the unfiltered maps of its neighbours, then all replaced at once
	void FilterDepthMaps() {
		check(pmhip_scene_filter(e_, ids_.data(), (int)ids_.size(), opt_.bFilterAdjust ? 1 : 0, opt_.nMinViewsFilter, opt_.nMinViewsFilterAdjust, opt_.fDepthDiffThreshold, 1));
		check(pmhip_scene_filter_commit(e_));
	}

	// DepthMapsData::FuseDepthMaps, :1372-1650 (MergeDepthMaps when nMinViewsFuse < 2): images best connected first (:1423-1450)
	void FuseDepthMaps(PointCloud& pc) { FuseOn(e_, views_, opt_, pc); }
	// the same on any engine that holds the final maps of all views (the multi-device host fuses on one device after a gather)
	static void FuseOn(pmhip_engine* e, const std::vector<View>& views, const Options& opt, PointCloud& pc) {
		auto chk = [e](int rc) { if (rc != PMHIP_OK) throw std::runtime_error(std::string("pmhip: ") + pmhip_last_error(e)); };
		auto score = [&views](int32_t i) { const View& v = views[(size_t)i]; return v.connections < 0 ? (float)v.neighbors.size() : v.connections; };
		std::vector<int32_t> order;
		for (int32_t i = 0; i < (int32_t)views.size(); ++i) if (opt.nMinViewsFuse < 2 || score(i) > 0) order.push_back(i);     // connections with score <= 0 are dropped (:1451-1452)
		if (opt.nMinViewsFuse >= 2)
			std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return score(a) > score(b); });   // ties in index order
		PMHipFuseParams fp;
		fp.nMinViewsFuse = opt.nMinViewsFuse; fp.fDepthDiffThreshold = opt.fDepthDiffThreshold; fp.fNormalDiffThreshold = opt.fNormalDiffThreshold;
		bool haveColor = opt.bEstimateColor;
		for (const View& v : views) haveColor = haveColor && (v.bgr != nullptr || v.image8 != nullptr);   // (an image8 view got its colour image from the store)
		fp.bEstimateColor = haveColor ? 1 : 0; fp.bEstimateNormal = opt.bEstimateNormal ? 1 : 0;
		uint64_t nP = 0, nV = 0, nD = 0;
		chk(pmhip_scene_fuse(e, order.data(), (int)order.size(), &fp, &nP, &nV, &nD));
		pc.points.assign((size_t)nP * 3, 0.f); pc.viewStart.assign((size_t)nP + 1, 0u); pc.views.assign((size_t)nV, 0u); pc.weights.assign((size_t)nV, 0.f);
		pc.projs.assign((size_t)nV * 2, (uint16_t)0);
		pc.colors.assign(haveColor ? (size_t)nP * 3 : 0, (unsigned char)0); pc.normals.assign(opt.bEstimateNormal ? (size_t)nP * 3 : 0, 0.f);
		chk(pmhip_scene_fuse_get(e, pc.points.data(), pc.viewStart.data(), pc.views.data(), pc.weights.data(), pc.projs.data(),
		                         haveColor ? pc.colors.data() : nullptr, opt.bEstimateNormal ? pc.normals.data() : nullptr));
	}

	// TOBB<float,3> after Set(rot, ptMin, ptMax) (Scene::obb): row-major rotation, centre, half-extents
	struct OBB { float rot[9], pos[3], ext[3]; };
	// The block after the fusion (SceneDensify.cpp:1724-1737) on the cloud FuseDepthMaps left on the device: RemovePointsOutside(ROI) when bCrop2ROI (the caller
	// tests Scene::IsBounded; fBorderROI > 0 enlarges the extents by that factor, < 0 adds -fBorderROI), then EstimatePointColors / EstimatePointNormals as
	// Options::bPointColors / bPointNormals ask and `pc` has none.  `pc` is replaced by the finished cloud.
	void FinishPointCloud(PointCloud& pc, const OBB& roi, bool bCrop2ROI, float fBorderROI) { FinishOn(e_, opt_, pc, roi, bCrop2ROI, fBorderROI); }
	static void FinishOn(pmhip_engine* e, const Options& opt, PointCloud& pc, const OBB& roi, bool bCrop2ROI, float fBorderROI) {
		auto chk = [e](int rc) { if (rc != PMHIP_OK) throw std::runtime_error(std::string("pmhip: ") + pmhip_last_error(e)); };
		if (pc.size() == 0) return;                                                       // if (!pointcloud.IsEmpty())
		PMHipCloudParams p;
		memset(&p, 0, sizeof(p));
		p.bCrop = bCrop2ROI ? 1 : 0;
		memcpy(p.obbRot, roi.rot, sizeof(p.obbRot)); memcpy(p.obbPos, roi.pos, sizeof(p.obbPos)); memcpy(p.obbExt, roi.ext, sizeof(p.obbExt));
		p.fBorderROI = fBorderROI;
		p.bEstimateColor = opt.bPointColors && pc.colors.empty() ? 1 : 0;
		p.bEstimateNormal = opt.bPointNormals && pc.normals.empty() ? 1 : 0;
		p.nNeighbors = opt.nNeighbors;
		if (!p.bCrop && !p.bEstimateColor && !p.bEstimateNormal) return;
		const bool color = !pc.colors.empty() || p.bEstimateColor, normal = !pc.normals.empty() || p.bEstimateNormal;
		uint64_t nP = 0, nV = 0;
		chk(pmhip_scene_cloud_finish(e, &p, &nP, &nV));
		pc.points.assign((size_t)nP * 3, 0.f); pc.viewStart.assign((size_t)nP + 1, 0u); pc.views.assign((size_t)nV, 0u); pc.weights.assign((size_t)nV, 0.f);
		pc.projs.assign((size_t)nV * 2, (uint16_t)0);
		pc.colors.assign(color ? (size_t)nP * 3 : 0, (unsigned char)0); pc.normals.assign(normal ? (size_t)nP * 3 : 0, 0.f);
		chk(pmhip_scene_fuse_get(e, pc.points.data(), pc.viewStart.data(), pc.views.data(), pc.weights.data(), pc.projs.data(),
		                         color ? pc.colors.data() : nullptr, normal ? pc.normals.data() : nullptr));
	}

	// Scene::PointCloudFilter(thRemove) (--filter-point-cloud, SceneDensify.cpp:2225-2359) on the cloud FuseDepthMaps / FinishPointCloud left on the device, after
	// PointCloud::RemoveMinViews(nMinViews) when nMinViews > 0: the visibility vote over the loaded scene's cameras at each view's own width, then the reference's
	// backward swap-remove loop.  The application runs it for thRemove < 0; any value is taken here.  `pc` is replaced by the filtered cloud; `visibility`, when
	// given, receives the votes, indexed as the cloud was before the visibility removal.
	void FilterPointCloud(PointCloud& pc, int thRemove, unsigned nMinViews = 0, std::vector<int32_t>* visibility = nullptr) { FilterOn(e_, pc, thRemove, nMinViews, visibility); }
	static void FilterOn(pmhip_engine* e, PointCloud& pc, int thRemove, unsigned nMinViews, std::vector<int32_t>* visibility) {
		auto chk = [e](int rc) { if (rc != PMHIP_OK) throw std::runtime_error(std::string("pmhip: ") + pmhip_last_error(e)); };
		if (visibility) visibility->clear();
		if (pc.size() == 0) return;
		PMHipCloudFilterParams p;
		memset(&p, 0, sizeof(p));
		uint64_t nP = pc.size(), nV = 0;
		if (nMinViews > 0) { p.nMinViews = nMinViews; chk(pmhip_scene_cloud_filter(e, &p, &nP, &nV)); p.nMinViews = 0; }   // (on its own: nP is then the size of the vote)
		const uint64_t nVote = nP;
		p.bVisibility = 1; p.thRemove = thRemove;
		chk(pmhip_scene_cloud_filter(e, &p, &nP, &nV));
		if (visibility && nVote) { visibility->assign((size_t)nVote, 0); chk(pmhip_scene_cloud_visibility(e, visibility->data(), nVote)); }
		const bool color = !pc.colors.empty(), normal = !pc.normals.empty();
		pc.points.assign((size_t)nP * 3, 0.f); pc.viewStart.assign((size_t)nP + 1, 0u); pc.views.assign((size_t)nV, 0u); pc.weights.assign((size_t)nV, 0.f);
		pc.projs.assign((size_t)nV * 2, (uint16_t)0);
		pc.colors.assign(color ? (size_t)nP * 3 : 0, (unsigned char)0); pc.normals.assign(normal ? (size_t)nP * 3 : 0, 0.f);
		chk(pmhip_scene_fuse_get(e, pc.points.data(), pc.viewStart.data(), pc.views.data(), pc.weights.data(), pc.projs.data(),
		                         color ? pc.colors.data() : nullptr, normal ? pc.normals.data() : nullptr));
	}

	// A depth map that enters from outside instead of being estimated (a depthNNNN.dmap of an importer or a depth sensor, read with include/dmapio.h): depth and
	// confidence (may be null) become the view's resident maps, ViewWidth(idx) x ViewHeight(idx) entries.  normal == null: the map was stored without normals, and
	// EstimateMissingNormals() makes them from the depths, as DepthMapsData::InitViews does (EstimateNormalMap, SceneDensify.cpp:411-414).
	void SetDepthMap(int idx, const float* depth, const float* normal, const float* conf) {
		if (!depth) throw std::runtime_error("DenseDepthMapsHIP: SetDepthMap without a depth map");
		check(pmhip_scene_set_maps(e_, idx, depth, normal));
		if (conf) check(pmhip_scene_set_conf(e_, idx, conf));
		noNormals_.erase(std::remove(noNormals_.begin(), noNormals_.end(), (int32_t)idx), noNormals_.end());
		if (!normal) noNormals_.push_back((int32_t)idx);
	}
	// MVS::EstimateNormalMap on the device (pmhip_scene_estimate_normals) for the views SetDepthMap installed without normals since the last call; returns how many
	size_t EstimateMissingNormals() {
		const size_t n = noNormals_.size();
		check(pmhip_scene_estimate_normals(e_, noNormals_.data(), (int)n));
		noNormals_.clear();
		return n;
	}

	// A triangle mesh (Scene::mesh after --mesh-file) made resident for ProjectMesh: 3 floats per vertex, 3 vertex indices per face; vertexNormals null: computed as
	// Mesh::ComputeNormalVertices does.  Independent of the loaded scene.
	void SetMesh(const float* vertices, uint32_t nVertices, const uint32_t* faces, uint32_t nFaces, const float* vertexNormals = nullptr) {
		check(pmhip_mesh_set(e_, vertices, nVertices, faces, nFaces, vertexNormals));
	}
	// Mesh::Project(camera, depthMap, normalMap) into the listed views of the loaded scene, each at its own size and camera, in one call (what
	// Scene::ExportMeshToDepthMaps renders, Scene.cpp:680-736).  depth[k] receives ViewWidth x ViewHeight floats of view ids[k], normal[k] three times as many;
	// withNormals = false: depth only, `normal` is left alone.
	void ProjectMesh(const std::vector<int32_t>& ids, std::vector<std::vector<float>>& depth, std::vector<std::vector<float>>& normal, bool withNormals = true) {
		const size_t n = ids.size();
		std::vector<double> K(9 * n), R(9 * n), C(3 * n);
		std::vector<int32_t> wh(2 * n);
		std::vector<float*> dp(n), np(n);
		depth.resize(n);
		if (withNormals) normal.resize(n);
		for (size_t k = 0; k < n; ++k) {
			const View& v = views_.at((size_t)ids[k]);
			std::memcpy(&K[9 * k], v.K, 72); std::memcpy(&R[9 * k], v.R, 72); std::memcpy(&C[3 * k], v.C, 24);
			wh[2 * k] = ViewWidth(ids[k]); wh[2 * k + 1] = ViewHeight(ids[k]);
			const size_t P = (size_t)wh[2 * k] * wh[2 * k + 1];
			depth[k].assign(P, 0.f); dp[k] = depth[k].data();
			if (withNormals) { normal[k].assign(3 * P, 0.f); np[k] = normal[k].data(); }
		}
		check(pmhip_mesh_project(e_, (int)n, K.data(), R.data(), C.data(), wh.data(), dp.data(), withNormals ? np.data() : nullptr));
	}
	void ReleaseMesh() { check(pmhip_mesh_release(e_)); }

	// ---- the reference's image and PLY outputs, made on the device from the resident maps (include/pmhip_export.h).  The images come back as bytes for the host's own
	// codec (ViewWidth x ViewHeight pixels, red first); PLY files are plain bytes and are written here, binary little endian with the header of PLY::header_complete.
	// DepthMap2Image (ExportDepthMap): rgb gets 3 bytes per pixel; the range of the X84 rule unless minDepth / maxDepth are given; returns the range in use
	std::pair<float, float> DepthImage(int idx, std::vector<unsigned char>& rgb, float minDepth = FLT_MAX, float maxDepth = 0) {
		rgb.assign((size_t)ViewWidth(idx) * ViewHeight(idx) * 3, (unsigned char)0);
		float range[2] = {0, 0};
		check(pmhip_scene_depth_image(e_, idx, minDepth, maxDepth, rgb.data(), range));
		return std::make_pair(range[0], range[1]);
	}
	// ExportNormalMap's image
	void NormalImage(int idx, std::vector<unsigned char>& rgb) {
		rgb.assign((size_t)ViewWidth(idx) * ViewHeight(idx) * 3, (unsigned char)0);
		check(pmhip_scene_normal_image(e_, idx, rgb.data()));
	}
	// ExportConfidenceMap's image, one byte per pixel; false (and nothing to write) when no confidence is positive, as the reference returns
	bool ConfImage(int idx, std::vector<unsigned char>& gray) {
		gray.assign((size_t)ViewWidth(idx) * ViewHeight(idx), (unsigned char)0);
		int empty = 0;
		check(pmhip_scene_conf_image(e_, idx, gray.data(), nullptr, &empty));
		return !empty;
	}
	// MVS::ExportPointCloud (DepthMap.cpp:1753-1870) of view idx into `path`, with normals (x y z nx ny nz red green blue) or without (x y z red green blue); false and
	// no file when no depth is valid.  Returns through `count` the number of vertices.
	bool ViewCloud(int idx, const std::string& path, bool withNormals = true, uint64_t* count = nullptr) {
		uint64_t n = 0;
		if (pmhip_scene_view_cloud(e_, idx, withNormals ? 1 : 0, nullptr, 0, &n) != PMHIP_OK && n == 0) check(PMHIP_E_ARG);   // (too small a capacity is how the count is asked for)
		if (count) *count = n;
		if (!n) return false;
		std::vector<unsigned char> rec((size_t)n * (withNormals ? 27 : 15));
		check(pmhip_scene_view_cloud(e_, idx, withNormals ? 1 : 0, rec.data(), n, &n));
		std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) + "\nproperty float32 x\nproperty float32 y\nproperty float32 z\n";
		if (withNormals) head += "property float32 nx\nproperty float32 ny\nproperty float32 nz\n";
		head += "property uint8 red\nproperty uint8 green\nproperty uint8 blue\nend_header\n";
		writeFile(path, head, rec.data(), rec.size());
		return true;
	}
	// PointCloud::Save(path, bViews) of `pc` -- x y z [red green blue] [nx ny nz] [view_indices] [view_weights], properties in InitSaveProps' order (PointCloud.cpp:265-304);
	// minViews > 0: PointCloud::SaveNViews (the points with at least that many views, white without colours); scaleMult > 0: PointCloud::SaveWithScale, the per-point
	// scales computed on the device for the resident cloud (pmhip_scene_cloud_scale), which must be `pc` (as FuseDepthMaps / FinishPointCloud / FilterPointCloud left it).
	// False and no file for an empty cloud.
	bool SavePointCloud(const std::string& path, const PointCloud& pc, bool bViews = true, unsigned minViews = 0, float scaleMult = 0) {
		const size_t n = pc.size();
		if (!n) return false;
		const bool color = !pc.colors.empty() || (minViews > 0 && scaleMult <= 0), normal = !pc.normals.empty(), lists = bViews && minViews == 0 && scaleMult <= 0 && !pc.views.empty();
		const bool weights = lists && pc.weights.size() == pc.views.size();
		std::vector<float> scale, conf;
		if (scaleMult > 0) { scale.assign(n, 0.f); conf.assign(n, 0.f); check(pmhip_scene_cloud_scale(e_, scaleMult, scale.data(), conf.data())); }
		std::vector<unsigned char> body;
		auto put = [&body](const void* p, size_t bytes) { body.insert(body.end(), (const unsigned char*)p, (const unsigned char*)p + bytes); };
		size_t kept = 0;
		for (size_t i = 0; i < n; ++i) {
			const uint32_t a = pc.viewStart[i], b = pc.viewStart[i + 1];
			if (scaleMult <= 0 && minViews > 0 && b - a < minViews) continue;
			++kept;
			put(&pc.points[3 * i], 12);
			if (color) { const unsigned char white[3] = {255, 255, 255}; const unsigned char* c = pc.colors.empty() ? white : &pc.colors[3 * i]; const unsigned char rgb[3] = {c[2], c[1], c[0]}; put(rgb, 3); }
			if (normal) put(&pc.normals[3 * i], 12);
			if (lists) {
				if (b - a > 255) throw std::runtime_error("DenseDepthMapsHIP: a point with more than 255 views");
				const unsigned char cnt = (unsigned char)(b - a);
				put(&cnt, 1); put(&pc.views[a], 4 * (size_t)cnt);
				if (weights) { put(&cnt, 1); put(&pc.weights[a], 4 * (size_t)cnt); }
			}
			if (scaleMult > 0) { put(&conf[i], 4); put(&scale[i], 4); }
		}
		if (!kept) return false;
		std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(kept) + "\nproperty float32 x\nproperty float32 y\nproperty float32 z\n";
		if (color) head += "property uint8 red\nproperty uint8 green\nproperty uint8 blue\n";
		if (normal) head += "property float32 nx\nproperty float32 ny\nproperty float32 nz\n";
		if (lists) head += "property list uint8 uint32 view_indices\n";
		if (weights) head += "property list uint8 float32 view_weights\n";
		if (scaleMult > 0) head += "property float32 confidence\nproperty float32 value\n";
		head += "end_header\n";
		writeFile(path, head, body.data(), body.size());
		return true;
	}

	// One view's maps back to the host (any pointer may be null); ViewWidth(idx) x ViewHeight(idx) entries
	void GetMaps(int idx, float* depth, float* normal, float* conf) { check(pmhip_scene_get_maps(e_, idx, depth, normal, conf)); }
	int ViewWidth(int idx) const { return views_[(size_t)idx].w > 0 ? views_[(size_t)idx].w : w_; }
	int ViewHeight(int idx) const { return views_[(size_t)idx].h > 0 ? views_[(size_t)idx].h : h_; }

	// DepthData::Save for every view: "<dir>/depthNNNN.dmap" (ComposeDepthFilePath, DepthMap.h:72), written through dmap_write (include/dmapio.h);
	// declared as a template on the writer so that this header does not force libdmapio on callers that never save
	template <typename DMapHeaderT, typename WriteFn>
	void SaveDepthMaps(const std::string& dir, WriteFn dmapWrite) {
		std::vector<float> d, nrm, c;
		for (size_t i = 0; i < views_.size(); ++i) {
			const View& v = views_[i];
			const int vw = ViewWidth((int)i), vh = ViewHeight((int)i);
			d.resize((size_t)vw * vh); nrm.resize((size_t)vw * vh * 3); c.resize((size_t)vw * vh);
			GetMaps((int)i, d.data(), nrm.data(), c.data());
			DMapHeaderT hdr; std::memset(&hdr, 0, sizeof(hdr));
			hdr.imageWidth = hdr.depthWidth = (uint32_t)vw; hdr.imageHeight = hdr.depthHeight = (uint32_t)vh;
			hdr.dMin = v.dMin; hdr.dMax = v.dMax; hdr.type = 1u | 2u | 4u;
			hdr.nIDs = (uint32_t)std::min<size_t>(v.neighbors.size() + 1, 256);
			hdr.IDs[0] = v.ID;
			for (uint32_t k = 1; k < hdr.nIDs; ++k) hdr.IDs[k] = views_[(size_t)v.neighbors[k - 1]].ID;
			std::memcpy(hdr.K, v.K, 72); std::memcpy(hdr.R, v.R, 72); std::memcpy(hdr.C, v.C, 24);
			std::snprintf(hdr.imageFileName, sizeof(hdr.imageFileName), "%s", v.name.c_str());
			char name[32]; std::snprintf(name, sizeof(name), "depth%04u.dmap", v.ID);
			if (dmapWrite((dir + "/" + name).c_str(), &hdr, d.data(), nrm.data(), c.data(), nullptr) != 0) throw std::runtime_error("DenseDepthMapsHIP: cannot write " + dir + "/" + name);
		}
	}

	pmhip_engine* engine() { return e_; }

private:
	static void writeFile(const std::string& path, const std::string& head, const unsigned char* body, size_t bytes) {
		FILE* f = std::fopen(path.c_str(), "wb");
		const bool ok = f && std::fwrite(head.data(), 1, head.size(), f) == head.size() && std::fwrite(body, 1, bytes, f) == bytes;
		if (f && std::fclose(f) != 0) throw std::runtime_error("DenseDepthMapsHIP: cannot write " + path);
		if (!ok) throw std::runtime_error("DenseDepthMapsHIP: cannot write " + path);
	}
	void check(int rc) const {
		if (rc != PMHIP_OK) throw std::runtime_error(std::string("pmhip: ") + (e_ ? pmhip_last_error(e_) : "no device"));
	}
	pmhip_engine* e_;
	int w_, h_;
	Options opt_;
	std::vector<View> views_;
	std::vector<int32_t> ids_;
	std::vector<int32_t> noNormals_;   // views whose maps SetDepthMap installed without normals
};

} // namespace MVS
