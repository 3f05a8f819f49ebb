// pm_host_fuse.hip -- host side of FuseDepthMaps (kernels: pm_fuse.hip).  Part of the translation unit pm_engine.hip.
// ---- FuseDepthMaps (libs/MVS/SceneDensify.cpp:1372-1650) on the resident scene -------------------------------------------------
static int ensureFuse(pmhip_engine* e) {
	auto& f = e->fu;
	size_t P = (size_t)e->w * e->h; const size_t N = (size_t)e->nImages;
	for (int i = 0; i < e->nImages; ++i) P = std::max(P, e->vpix(i));           // a slab holds the largest image
	if (f.depth && f.slab >= P) return 0;
	if (f.depth) {                                                              // a view grew: start over (the colour images and the output stay)
		HIPCHK(e, hipStreamSynchronize(e->stream));
		static_cast<FuseWork&>(f) = FuseWork{};
	}
	HIPCHK(e, f.depth.alloc(P * N));
	HIPCHK(e, f.claimed.alloc(P * N));
	HIPCHK(e, f.resv.alloc(P * N));
	HIPCHK(e, f.cams.alloc(N));
	HIPCHK(e, f.dims.alloc(2 * N));
	HIPCHK(e, f.recN.alloc(P)); HIPCHK(e, f.recColor.alloc(3 * P));
	HIPCHK(e, f.recX.alloc(3 * P)); HIPCHK(e, f.recNormal.alloc(3 * P));
	HIPCHK(e, f.recWeight.alloc(PMFU_MAXV * P));
	HIPCHK(e, f.recView.alloc(PMFU_MAXV * P)); HIPCHK(e, f.recProj.alloc(PMFU_MAXV * P));
	HIPCHK(e, f.pend[0].alloc(P)); HIPCHK(e, f.pend[1].alloc(P));
	HIPCHK(e, f.counters.alloc(8)); HIPCHK(e, f.nDepthsDev.alloc(2));
	const size_t nTiles = (P + PMFU_TILE - 1) / PMFU_TILE;
	HIPCHK(e, f.tileSums.alloc(nTiles)); HIPCHK(e, f.tileOff.alloc(nTiles));
	HIPCHK(e, f.pin.alloc(16));
	f.slab = P;
	return 0;
}

extern "C" {

// pmhip_scene_set_color from a host image, or from a device image of the store (pmhip_scene_set_view_stored)
static int sceneSetColor(pmhip_engine* e, int idx, const unsigned char* bgr, hipMemcpyKind kind) {
	if (!e || !bgr || idx < 0 || idx >= e->nImages) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	auto& f = e->fu;
	const size_t P = (size_t)e->w * e->h;
	if (f.hasBgr.empty()) f.hasBgr.assign(e->nImages, 0);
	SceneView& v = e->views[idx];
	if (v.sw) {                                                                  // a view with its own size keeps its colour image itself
		if (!v.oBgr) HIPCHK(e, v.oBgr.alloc(3 * e->vpix(idx)));
		HIPCHK(e, hipMemcpyAsync(v.oBgr, bgr, 3 * e->vpix(idx), kind, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		f.hasBgr[idx] = 1;
		return 0;
	}
	if (!f.bgr) HIPCHK(e, f.bgr.alloc(3 * P * e->nImages));
	HIPCHK(e, hipMemcpyAsync(f.bgr + 3 * P * idx, bgr, 3 * P, kind, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	f.hasBgr[idx] = 1;
	return 0;
}
int pmhip_scene_set_color(pmhip_engine* e, int idx, const unsigned char* bgr) { return sceneSetColor(e, idx, bgr, hipMemcpyHostToDevice); }

int pmhip_scene_fuse(pmhip_engine* e, const int32_t* order, int nOrder, const PMHipFuseParams* prm, uint64_t* nPoints, uint64_t* nViews, uint64_t* nDepths) {
	if (!e || !order || nOrder <= 0 || !prm || e->nImages < 1) return PMHIP_E_ARG;
	bool mixed = false;
	for (int i = 0; i < e->nImages; ++i) { mixed = mixed || e->views[i].sw; if (e->vw(i) > 65535 || e->vh(i) > 65535) { e->err = "fusion stores projections as 16-bit pixel coordinates"; return PMHIP_E_SIZE; } }
	HIPCHK(e, hipSetDevice(e->device));
	int rc = ensureFuse(e); if (rc) return rc;
	auto& f = e->fu;
	const size_t P = f.slab, N = (size_t)e->nImages, P0 = (size_t)e->w * e->h;
	bool wantColor = prm->bEstimateColor != 0;
	if (wantColor) {
		// colours are read of the fused views and of their neighbours only (SceneDensify.cpp:1455-1560): a source-only slot -- a resampled copy of a neighbour that the estimation
		// read (ViewData::ScaleImage) -- has no depth map, is nobody's neighbour here and needs no colour
		std::vector<unsigned char> need((size_t)e->nImages, 0);
		for (int k = 0; k < nOrder; ++k) {
			const int v = order[k];
			if (v < 0 || v >= e->nImages) continue;
			need[(size_t)v] = 1;
			for (int j = 0; j < e->views[v].nNb; ++j) { const int b = e->views[v].nb[j]; if (b >= 0 && b < e->nImages) need[(size_t)b] = 1; }
		}
		for (int i = 0; i < e->nImages; ++i) if (need[(size_t)i] && e->views[i].set && (f.hasBgr.empty() || !f.hasBgr[i] || !(e->views[i].sw ? (const void*)e->views[i].oBgr : (const void*)f.bgr))) {
			e->err = "bEstimateColor needs pmhip_scene_set_color for every fused view and its neighbours"; return PMHIP_E_STATE; }
	}
	const bool wantNormal = prm->bEstimateNormal != 0;
	// cameras (P composed like Camera::ComposeP)
	std::vector<PMFuseCam> hc(N);
	for (size_t i = 0; i < N; ++i) { memset(&hc[i], 0, sizeof(PMFuseCam)); if (!e->views[i].set) continue; memcpy(hc[i].K, e->views[i].K, 72); memcpy(hc[i].R, e->views[i].R, 72); memcpy(hc[i].C, e->views[i].C, 24); pmfu_composeP(hc[i]); }
	HIPCHK(e, hipMemcpyAsync(f.cams, hc.data(), sizeof(PMFuseCam) * N, hipMemcpyHostToDevice, e->stream));
	// working copies of the depth maps, one slab per image; with views of different sizes also the read-only inputs are gathered into slabs (each image with its own row pitch)
	const bool slabs = mixed || P != P0;
	if (!slabs) HIPCHK(e, hipMemcpyAsync(f.depth, e->d_depth, sizeof(float) * P * N, hipMemcpyDeviceToDevice, e->stream));
	else {
		if (!f.normalS) { HIPCHK(e, f.normalS.alloc(3 * P * N)); HIPCHK(e, f.confS.alloc(P * N)); }
		if (wantColor && !f.bgrS) HIPCHK(e, f.bgrS.alloc(3 * P * N));
		HIPCHK(e, hipMemsetAsync(f.depth, 0, sizeof(float) * P * N, e->stream));
		std::vector<int> hw(N), hh(N);
		for (size_t i = 0; i < N; ++i) {
			const size_t Pi = e->vpix((int)i);
			hw[i] = e->vw((int)i); hh[i] = e->vh((int)i);
			HIPCHK(e, hipMemcpyAsync(f.depth + P * i, e->depthOf((int)i), sizeof(float) * Pi, hipMemcpyDeviceToDevice, e->stream));
			HIPCHK(e, hipMemcpyAsync(f.normalS + 3 * P * i, e->normalOf((int)i), sizeof(float) * 3 * Pi, hipMemcpyDeviceToDevice, e->stream));
			HIPCHK(e, hipMemcpyAsync(f.confS + P * i, e->confOf((int)i), sizeof(float) * Pi, hipMemcpyDeviceToDevice, e->stream));
			if (wantColor && e->views[i].set && !f.hasBgr.empty() && f.hasBgr[i]) HIPCHK(e, hipMemcpyAsync(f.bgrS + 3 * P * i, e->views[i].sw ? e->views[i].oBgr : f.bgr + 3 * P0 * i, 3 * Pi, hipMemcpyDeviceToDevice, e->stream));
		}
		HIPCHK(e, hipMemcpyAsync(f.dims, hw.data(), sizeof(int) * N, hipMemcpyHostToDevice, e->stream));          // iw = dims, ih = dims + N
		HIPCHK(e, hipMemcpyAsync(f.dims + N, hh.data(), sizeof(int) * N, hipMemcpyHostToDevice, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));                                 // hw / hh live on this frame
	}
	hipLaunchKernelGGL(pmfu_fill_u32, dim3(2048), dim3(256), 0, e->stream, f.claimed, P * N, PMFU_NO_ID);
	hipLaunchKernelGGL(pmfu_fill_u32, dim3(2048), dim3(256), 0, e->stream, f.resv, P * N, PMFU_FREE);
	HIPCHK(e, hipMemsetAsync(f.counters, 0, sizeof(uint32_t) * 8, e->stream));
	HIPCHK(e, hipMemsetAsync(f.nDepthsDev, 0, sizeof(unsigned long long) * 2, e->stream));
	// output capacity: a point needs a seed and every pixel joins at most one point, so both are bounded by the valid depths
	hipLaunchKernelGGL(pmfu_count_valid, dim3(2048), dim3(256), 0, e->stream, f.depth, P * N, f.nDepthsDev + 1);
	unsigned long long nValid = 0;
	HIPCHK(e, hipMemcpyAsync(&nValid, f.nDepthsDev + 1, sizeof(nValid), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (nValid >= 0xFFFFFFFFull) { e->err = "more than 2^32 depths"; return PMHIP_E_SIZE; }
	HIPCHK(e, f.out.reserve((size_t)nValid + 1, wantColor, wantNormal));
	const PMFuseOut out = f.out.view(wantColor, wantNormal);
	const unsigned nMin = std::min<unsigned>(prm->nMinViewsFuse, (unsigned)e->nImages);
	const float normalError = cosf(prm->fNormalDiffThreshold * (3.14159265358979323846f / 180.f));   // COS(FD2R(x)), SceneDensify.cpp:1455
	f.rounds = 0;
	for (int o = 0; o < nOrder; ++o) {
		const int A = order[o];
		if (A < 0 || A >= e->nImages || !e->views[A].set) { e->err = "fuse: view not set"; return PMHIP_E_ARG; }
		const size_t PA = e->vpix(A);                                               // image A's own pixels: seeds, records, compaction
		const unsigned nTiles = (unsigned)((PA + PMFU_TILE - 1) / PMFU_TILE);
		PMFuseCtx c; memset(&c, 0, sizeof(c));
		c.w = e->w; c.h = e->h; c.nImages = e->nImages; c.A = A;
		c.slab = P; if (slabs) { c.iw = f.dims; c.ih = f.dims + N; }
		for (int k = 0; k < e->views[A].nNb && c.nNb < PMFU_MAXNB; ++k) { const int b = e->views[A].nb[k]; if (b >= 0 && b < e->nImages && b != A && e->views[b].set) c.nb[c.nNb++] = b; }
		c.depth = f.depth; c.normal = slabs ? f.normalS : e->d_normal; c.conf = slabs ? f.confS : e->d_conf; c.bgr = slabs ? (wantColor ? f.bgrS : nullptr) : f.bgr; c.claimed = f.claimed; c.resv = f.resv; c.cams = f.cams;
		c.nMinViewsFuse = nMin; c.fDepthDiffThreshold = prm->fDepthDiffThreshold; c.normalError = normalError;
		c.bEstimateColor = wantColor ? 1 : 0; c.bEstimateNormal = wantNormal ? 1 : 0;
		c.recN = f.recN; c.recX = f.recX; c.recView = f.recView; c.recWeight = f.recWeight; c.recProj = f.recProj; c.recColor = f.recColor; c.recNormal = f.recNormal;
		if (prm->nMinViewsFuse < 2) {   // MergeDepthMaps (Scene::DenseReconstruction, SceneDensify.cpp:1695-1698)
			hipLaunchKernelGGL(pmfu_merge_kernel, dim3((unsigned)std::min<size_t>((PA + 255) / 256, 4096)), dim3(256), 0, e->stream, c, f.nDepthsDev);
			hipLaunchKernelGGL(pmfu_tile_sums, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, f.recN, (uint32_t)PA, f.tileSums);
			hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, f.tileSums, nTiles, f.counters + 2, f.tileOff);
			hipLaunchKernelGGL(pmfu_scatter_kernel, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, c, f.tileOff, out);
			HIPCHK(e, hipGetLastError());
			continue;
		}
		HIPCHK(e, hipMemsetAsync(f.counters, 0, sizeof(uint32_t) * 2, e->stream));
		hipLaunchKernelGGL(pmfu_seed_kernel, dim3((unsigned)std::min<size_t>((PA + 255) / 256, 4096)), dim3(256), 0, e->stream, c, f.pend[0], f.counters, f.nDepthsDev);
		HIPCHK(e, hipMemcpyAsync(f.pin, f.counters, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		uint32_t n = f.pin[0]; int cur = 0;
		while (n) {
			++f.rounds;
			HIPCHK(e, hipMemsetAsync(f.counters + 1, 0, sizeof(uint32_t), e->stream));
			const unsigned gb = (n + 255) / 256;
			hipLaunchKernelGGL(pmfu_reserve_kernel, dim3(gb), dim3(256), 0, e->stream, c, f.pend[cur], n);
			hipLaunchKernelGGL(pmfu_commit_kernel, dim3(gb), dim3(256), 0, e->stream, c, f.pend[cur], n, f.pend[cur ^ 1], f.counters + 1);
			HIPCHK(e, hipMemcpyAsync(f.pin, f.counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
			HIPCHK(e, hipStreamSynchronize(e->stream));
			if (f.pin[0] >= n) { e->err = "fuse: no progress in a reservation round"; return PMHIP_E_STATE; }
			n = f.pin[0]; cur ^= 1;
		}
		hipLaunchKernelGGL(pmfu_tile_sums, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, f.recN, (uint32_t)PA, f.tileSums);
		hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, f.tileSums, nTiles, f.counters + 2, f.tileOff);
		hipLaunchKernelGGL(pmfu_scatter_kernel, dim3(nTiles), dim3(PMFU_TB), 0, e->stream, c, f.tileOff, out);
		HIPCHK(e, hipGetLastError());
	}
	unsigned long long nd = 0;
	HIPCHK(e, hipMemcpyAsync(f.pin, f.counters + 2, sizeof(uint32_t) * 2, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipMemcpyAsync(&nd, f.nDepthsDev, sizeof(nd), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	f.nPoints = f.pin[0]; f.nViews = f.pin[1]; f.nDepths = nd; f.haveColor = wantColor; f.haveNormal = wantNormal; f.haveWeight = prm->nMinViewsFuse >= 2;   // (MergeDepthMaps leaves pointWeights empty)
	const uint32_t last = (uint32_t)f.nViews;
	HIPCHK(e, hipMemcpyAsync(f.out.viewStart + f.nPoints, &last, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (nPoints) *nPoints = f.nPoints; if (nViews) *nViews = f.nViews; if (nDepths) *nDepths = f.nDepths;
	return 0;
}

int pmhip_scene_fuse_get(pmhip_engine* e, float* points, uint32_t* viewStart, uint32_t* views, float* weights, uint16_t* projs, unsigned char* colors, float* normals) {
	if (!e || !e->fu.out.points) return PMHIP_E_STATE;
	HIPCHK(e, hipSetDevice(e->device));
	auto& f = e->fu;
	if ((colors && !f.haveColor) || (normals && !f.haveNormal)) { e->err = "fuse_get: colours / normals were not estimated"; return PMHIP_E_STATE; }
	const size_t n = (size_t)f.nPoints, v = (size_t)f.nViews;
	if (points && n) HIPCHK(e, hipMemcpyAsync(points, f.out.points, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, e->stream));
	if (viewStart) HIPCHK(e, hipMemcpyAsync(viewStart, f.out.viewStart, sizeof(uint32_t) * (n + 1), hipMemcpyDeviceToHost, e->stream));
	if (views && v) HIPCHK(e, hipMemcpyAsync(views, f.out.views, sizeof(uint32_t) * v, hipMemcpyDeviceToHost, e->stream));
	if (weights && v) HIPCHK(e, hipMemcpyAsync(weights, f.out.weights, sizeof(float) * v, hipMemcpyDeviceToHost, e->stream));
	if (projs && v) HIPCHK(e, hipMemcpyAsync(projs, f.out.projs, sizeof(uint16_t) * 2 * v, hipMemcpyDeviceToHost, e->stream));
	if (colors && n) HIPCHK(e, hipMemcpyAsync(colors, f.out.colors, 3 * n, hipMemcpyDeviceToHost, e->stream));
	if (normals && n) HIPCHK(e, hipMemcpyAsync(normals, f.out.normals, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

uint64_t pmhip_scene_fuse_rounds(pmhip_engine* e) { return e ? e->fu.rounds : 0; }

} // extern "C"
