// pm_host_export.hip -- host side of the image and PLY outputs (kernels: pm_export.hip; ABI: include/pmhip_export.h).  Part of the translation unit pm_engine.hip.

// grow-only working buffers and the statistics of the last call
static int exBegin(pmhip_engine* e, size_t pixels) {
	auto& x = e->ex;
	HIPCHK(e, hipSetDevice(e->device));
	if (!x.st) HIPCHK(e, x.st.alloc(PMEX_WORDS));
	for (hipEvent_t& ev : x.ev) if (!ev) HIPCHK(e, hipEventCreate(&ev));
	if (pixels) HIPCHK(e, x.image.reserve((pixels + 3) / 4 * 12));         // bytes: three whole words per four pixels (pmex_store_rgb4)
	x.launches = 0; x.us = 0;
	HIPCHK(e, hipEventRecord(x.ev[0], e->stream));
	return 0;
}
static int exEnd(pmhip_engine* e) {
	auto& x = e->ex;
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipEventRecord(x.ev[1], e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	float ms = 0; HIPCHK(e, hipEventElapsedTime(&ms, x.ev[0], x.ev[1]));
	x.us = (uint64_t)(ms * 1000.f);
	return 0;
}
static unsigned exBlocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + PMEX_Q - 1) / PMEX_Q, PMEX_MAX_BLOCKS)); }

// ComputeX84Threshold and GetMinMax of the n values at dv into the state words: two selections of four digits, no host round trip
static int exSelect(pmhip_engine* e, const float* dv, size_t n) {
	auto& x = e->ex;
	static const struct Init { uint32_t w[PMEX_WORDS]; Init() { memset(w, 0, sizeof(w)); w[PMEX_MIN] = 0xFFFFFFFFu; } } init;
	HIPCHK(e, hipMemcpyAsync(x.st, init.w, sizeof(init.w), hipMemcpyHostToDevice, e->stream));
	for (int mode = 0; mode < 2; ++mode)
		for (int pass = 0; pass < 4; ++pass) {
			hipLaunchKernelGGL(pmex_hist_kernel, dim3(exBlocks(n)), dim3(PMEX_TB), 0, e->stream, dv, n, mode, pass, x.st);
			hipLaunchKernelGGL(pmex_pick_kernel, dim3(1), dim3(256), 0, e->stream, mode, pass, x.st);
			x.launches += 2;
		}
	return 0;
}
static int exState(pmhip_engine* e, uint32_t st[PMEX_HIST]) {
	HIPCHK(e, hipMemcpyAsync(st, e->ex.st, sizeof(uint32_t) * PMEX_HIST, hipMemcpyDeviceToHost, e->stream));
	return 0;
}
static float exFloat(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// a view of the scene that holds a depth map
static int exView(pmhip_engine* e, const char* who, int idx) {
	if (idx < 0 || idx >= e->nImages) { e->err = std::string(who) + ": view " + std::to_string(idx) + " is not a view of the scene"; return PMHIP_E_ARG; }
	if (!e->views[idx].hasMaps) { e->err = std::string(who) + ": view " + std::to_string(idx) + " holds no depth map"; return PMHIP_E_STATE; }
	return 0;
}

// DepthMap2Image of n = w*h depths on the device
static int exDepthImage(pmhip_engine* e, const float* dv, size_t n, float minDepth, float maxDepth, uint8_t* rgb, float range[2]) {
	auto& x = e->ex;
	const int autoRange = minDepth == FLT_MAX && maxDepth == 0;
	if (autoRange) { int rc = exSelect(e, dv, n); if (rc) return rc; }
	hipLaunchKernelGGL(pmex_depth_image_kernel, dim3(exBlocks(n)), dim3(PMEX_TB), 0, e->stream, dv, n, autoRange, minDepth, maxDepth, x.st, (uint32_t*)(uint8_t*)x.image);
	++x.launches;
	uint32_t st[PMEX_HIST];
	int rc = exState(e, st); if (rc) return rc;
	HIPCHK(e, hipMemcpyAsync(rgb, x.image, n * 3, hipMemcpyDeviceToHost, e->stream));
	rc = exEnd(e); if (rc) return rc;
	if (range) { range[0] = exFloat(st[PMEX_RMIN]); range[1] = exFloat(st[PMEX_RMAX]); }
	return 0;
}

extern "C" {

int pmhip_x84_threshold(pmhip_engine* e, const float* values, uint64_t n, float mul, float out[4]) {
	if (!e) return PMHIP_E_ARG;
	if (!values || !out || n == 0 || n >= 0xFFFFFFFFull) { e->err = "pmhip_x84_threshold: values and out of 1 .. 2^32 - 2 values"; return PMHIP_E_ARG; }
	int rc = exBegin(e, 0); if (rc) return rc;
	auto& x = e->ex;
	HIPCHK(e, x.stage.reserve((size_t)n));
	HIPCHK(e, hipMemcpyAsync(x.stage, values, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, e->stream));
	rc = exSelect(e, x.stage, (size_t)n); if (rc) return rc;
	uint32_t st[PMEX_HIST];
	rc = exState(e, st); if (rc) return rc;
	rc = exEnd(e); if (rc) return rc;
	if (!st[PMEX_COUNT]) { e->err = "pmhip_x84_threshold: no value > 0"; return PMHIP_E_ARG; }
	out[0] = exFloat(st[PMEX_MEDIAN]); out[1] = mul * exFloat(st[PMEX_MAD]); out[2] = exFloat(st[PMEX_MIN]); out[3] = exFloat(st[PMEX_MAX]);
	return 0;
}

int pmhip_scene_depth_image(pmhip_engine* e, int idx, float minDepth, float maxDepth, uint8_t* rgb, float range[2]) {
	if (!e) return PMHIP_E_ARG;
	if (!rgb) { e->err = "pmhip_scene_depth_image: no image buffer"; return PMHIP_E_ARG; }
	int rc = exView(e, "pmhip_scene_depth_image", idx); if (rc) return rc;
	rc = exBegin(e, e->vpix(idx)); if (rc) return rc;
	return exDepthImage(e, e->depthOf(idx), e->vpix(idx), minDepth, maxDepth, rgb, range);
}

int pmhip_depth_image(pmhip_engine* e, const float* depth, int w, int h, float minDepth, float maxDepth, uint8_t* rgb, float range[2]) {
	if (!e) return PMHIP_E_ARG;
	if (!depth || !rgb || w <= 0 || h <= 0) { e->err = "pmhip_depth_image: depth and rgb of a map of at least 1 x 1"; return PMHIP_E_ARG; }
	const size_t n = (size_t)w * h;
	int rc = exBegin(e, n); if (rc) return rc;
	HIPCHK(e, e->ex.stage.reserve(n));
	HIPCHK(e, hipMemcpyAsync(e->ex.stage, depth, sizeof(float) * n, hipMemcpyHostToDevice, e->stream));
	return exDepthImage(e, e->ex.stage, n, minDepth, maxDepth, rgb, range);
}

int pmhip_scene_normal_image(pmhip_engine* e, int idx, uint8_t* rgb) {
	if (!e) return PMHIP_E_ARG;
	if (!rgb) { e->err = "pmhip_scene_normal_image: no image buffer"; return PMHIP_E_ARG; }
	int rc = exView(e, "pmhip_scene_normal_image", idx); if (rc) return rc;
	const size_t n = e->vpix(idx);
	rc = exBegin(e, n); if (rc) return rc;
	auto& x = e->ex;
	hipLaunchKernelGGL(pmex_normal_image_kernel, dim3(exBlocks(n)), dim3(PMEX_TB), 0, e->stream, e->normalOf(idx), n, (uint32_t*)(uint8_t*)x.image);
	++x.launches;
	HIPCHK(e, hipMemcpyAsync(rgb, x.image, n * 3, hipMemcpyDeviceToHost, e->stream));
	return exEnd(e);
}

int pmhip_scene_conf_image(pmhip_engine* e, int idx, uint8_t* gray, float range[2], int* empty) {
	if (!e) return PMHIP_E_ARG;
	if (!gray || !empty) { e->err = "pmhip_scene_conf_image: gray and empty"; return PMHIP_E_ARG; }
	int rc = exView(e, "pmhip_scene_conf_image", idx); if (rc) return rc;
	const size_t n = e->vpix(idx);
	rc = exBegin(e, n); if (rc) return rc;
	auto& x = e->ex;
	rc = exSelect(e, e->confOf(idx), n); if (rc) return rc;
	hipLaunchKernelGGL(pmex_conf_image_kernel, dim3(exBlocks(n)), dim3(PMEX_TB), 0, e->stream, e->confOf(idx), n, x.st, (uint32_t*)(uint8_t*)x.image);
	++x.launches;
	uint32_t st[PMEX_HIST];
	rc = exState(e, st); if (rc) return rc;
	HIPCHK(e, hipMemcpyAsync(gray, x.image, n, hipMemcpyDeviceToHost, e->stream));      // (all 0 when no confidence is positive: the kernel writes every pixel)
	rc = exEnd(e); if (rc) return rc;
	*empty = st[PMEX_COUNT] ? 0 : 1;
	if (range && st[PMEX_COUNT]) { range[0] = exFloat(st[PMEX_RMIN]); range[1] = exFloat(st[PMEX_RMAX]); }
	return 0;
}

int pmhip_scene_view_cloud(pmhip_engine* e, int idx, int withNormals, void* records, uint64_t capacity, uint64_t* count) {
	if (!e) return PMHIP_E_ARG;
	if (!count || (capacity && !records)) { e->err = "pmhip_scene_view_cloud: count, and records for a capacity"; return PMHIP_E_ARG; }
	int rc = exView(e, "pmhip_scene_view_cloud", idx); if (rc) return rc;
	if (!e->views[idx].set) { e->err = "pmhip_scene_view_cloud: view " + std::to_string(idx) + " has no camera (pmhip_scene_set_view)"; return PMHIP_E_STATE; }
	const size_t P = e->vpix(idx);
	if (P >= 0xFFFFFFFFull) { e->err = "pmhip_scene_view_cloud: more than 2^32 pixels"; return PMHIP_E_SIZE; }
	rc = exBegin(e, 0); if (rc) return rc;
	auto& x = e->ex;
	const unsigned nTiles = (unsigned)((P + PMFU_TILE - 1) / PMFU_TILE);
	HIPCHK(e, x.flags.reserve(P)); HIPCHK(e, x.tileSums.reserve(nTiles)); HIPCHK(e, x.tileOff.reserve(nTiles));
	if (!x.totals) HIPCHK(e, x.totals.alloc(2));
	HIPCHK(e, hipMemsetAsync(x.totals, 0, sizeof(uint32_t) * 2, e->stream));
	const float* depth = e->depthOf(idx);
	hipLaunchKernelGGL(pmex_valid_flags, dim3(resampleBlocks(P, 4096)), dim3(256), 0, e->stream, depth, (uint32_t)P, x.flags);
	hipLaunchKernelGGL(pmfu_tile_sums, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, x.flags, (uint32_t)P, x.tileSums);
	hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, x.tileSums, nTiles, x.totals, x.tileOff);
	x.launches += 3;
	uint32_t tot[2] = {0, 0};
	HIPCHK(e, hipMemcpyAsync(tot, x.totals, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	*count = tot[0];
	if (tot[0] > capacity) { e->err = "pmhip_scene_view_cloud: " + std::to_string(tot[0]) + " records, capacity " + std::to_string(capacity); exEnd(e); return PMHIP_E_ARG; }
	if (!tot[0]) return exEnd(e);
	const size_t bytes = (size_t)tot[0] * (withNormals ? 27 : 15);
	HIPCHK(e, x.records.reserve(bytes));
	PMFuseCam cam; memset(&cam, 0, sizeof(cam));
	memcpy(cam.K, e->views[idx].K, 72); memcpy(cam.R, e->views[idx].R, 72); memcpy(cam.C, e->views[idx].C, 24);
	const auto& f = e->fu;
	const uint8_t* bgr = f.hasBgr.empty() || !f.hasBgr[idx] ? nullptr : e->views[idx].sw ? (const uint8_t*)e->views[idx].oBgr : f.bgr ? f.bgr + 3 * (size_t)e->w * e->h * idx : nullptr;
	hipLaunchKernelGGL(pmex_cloud_scatter, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, depth, withNormals ? (const float*)e->normalOf(idx) : (const float*)nullptr, bgr, (uint32_t)P,
	                   (uint32_t)e->vw(idx), cam, x.tileOff, x.records);
	++x.launches;
	HIPCHK(e, hipMemcpyAsync(records, x.records, bytes, hipMemcpyDeviceToHost, e->stream));
	return exEnd(e);
}

int pmhip_scene_cloud_scale(pmhip_engine* e, float scaleMult, float* scale, float* confidence) {
	if (!e) return PMHIP_E_ARG;
	auto& f = e->fu; auto& c = e->cl;
	if (!f.out.points) { e->err = "pmhip_scene_cloud_scale: no cloud (pmhip_scene_fuse, pmhip_scene_cloud_set or pmhip_scene_cloud_load first)"; return PMHIP_E_STATE; }
	if (f.nPoints && (!scale || !confidence)) { e->err = "pmhip_scene_cloud_scale: scale and confidence"; return PMHIP_E_ARG; }
	const int N = e->nImages;
	if (N < 1) { e->err = "pmhip_scene_cloud_scale: no scene, so no cameras"; return PMHIP_E_STATE; }
	int rc = exBegin(e, 0); if (rc) return rc;
	if (!f.nPoints) return exEnd(e);
	auto& x = e->ex;
	HIPCHK(e, c.fused.reserve((size_t)N + 1));
	std::vector<uint32_t> used;
	rc = viewsInUse(e, N, c.fused, used); if (rc) return rc;
	if (used[(size_t)N]) { e->err = "pmhip_scene_cloud_scale: a point lists a view outside the scene"; return PMHIP_E_STATE; }
	std::vector<PMFuseCam> hc((size_t)N);
	for (int i = 0; i < N; ++i) {
		memset(&hc[i], 0, sizeof(PMFuseCam));
		if (!e->views[i].set) { if (used[(size_t)i]) { e->err = "pmhip_scene_cloud_scale: a point lists a view without a camera"; return PMHIP_E_STATE; } continue; }
		memcpy(hc[i].K, e->views[i].K, 72); memcpy(hc[i].R, e->views[i].R, 72); memcpy(hc[i].C, e->views[i].C, 24);
	}
	const uint32_t n = (uint32_t)f.nPoints;
	HIPCHK(e, x.cams.reserve((size_t)N)); HIPCHK(e, x.scale.reserve(2 * (size_t)n));
	HIPCHK(e, hipMemcpyAsync(x.cams, hc.data(), sizeof(PMFuseCam) * N, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(pmex_scale_kernel, dim3(resampleBlocks(n, 4096)), dim3(256), 0, e->stream, f.out.points, f.out.viewStart, f.out.views,
	                   f.haveWeight ? (const float*)f.out.weights : (const float*)nullptr, x.cams, n, scaleMult, x.scale, x.scale + n);
	x.launches += 2;                                                                        // (with the census of the views in use)
	HIPCHK(e, hipMemcpyAsync(scale, x.scale, sizeof(float) * n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipMemcpyAsync(confidence, x.scale + n, sizeof(float) * n, hipMemcpyDeviceToHost, e->stream));
	return exEnd(e);                                                                        // (hc lives until the synchronise in there)
}

int pmhip_export_get_stats(pmhip_engine* e, uint64_t out[8]) {
	if (!e || !out) return PMHIP_E_ARG;
	out[0] = PMEX_Q; out[1] = PMEX_MAX_BLOCKS; out[2] = PMFU_TILE; out[3] = e->ex.launches; out[4] = e->ex.us; out[5] = out[6] = out[7] = 0;
	return 0;
}

} // extern "C"
