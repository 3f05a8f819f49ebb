// pm_host_estimate.hip -- host side of the estimation: batch scratch, pyramids, launch helpers, and the pass structure of DepthMapsData::EstimateDepthMap.
// Part of the translation unit pm_engine.hip (included there, after the engine struct).
static int ensureBatch(pmhip_engine* e, int n, int bw, int bh) {
	if (n <= e->batchCap && bw <= e->batchW && bh <= e->batchH) return 0;
	n = std::max(n, e->batchCap); bw = std::max(bw, e->batchW); bh = std::max(bh, e->batchH);
	HIPCHK(e, hipStreamSynchronize(e->stream));
	for (int l = 0; l < 4; ++l) e->d_lvl[l].release();
	e->d_tasks.release(); e->h_tasks.release(); e->d_ups.release(); e->h_ups.release();
	const size_t cap = (size_t)std::max(n, 1);
	HIPCHK(e, e->d_lvl[0].alloc(cap * bw * bh));
	for (int l = 1; l <= e->nLevels; ++l)
		HIPCHK(e, e->d_lvl[l].alloc(cap * 6 * lvlSize(bw, l) * lvlSize(bh, l)));
	HIPCHK(e, e->d_tasks.alloc(4 * cap));
	HIPCHK(e, e->h_tasks.alloc(4 * cap));
	HIPCHK(e, e->d_ups.alloc(4 * cap));
	HIPCHK(e, e->h_ups.alloc(4 * cap));
	e->batchCap = (int)cap; e->batchW = bw; e->batchH = bh;
	return 0;
}

// tiled sweeps: snapshot storage for the batch (grow only)
static int ensureOld(pmhip_engine* e) {
	if (e->tileW <= 0 || e->tileH <= 0) return 0;
	if (e->oldCap >= e->batchCap && e->oldW >= e->batchW && e->oldH >= e->batchH) return 0;
	HIPCHK(e, hipStreamSynchronize(e->stream));
	for (int l = 0; l < 4; ++l) e->d_old[l].release();
	for (int l = 0; l <= e->nLevels; ++l)
		HIPCHK(e, e->d_old[l].alloc((size_t)e->batchCap * 5 * lvlSize(e->batchW, l) * lvlSize(e->batchH, l)));
	e->oldCap = e->batchCap; e->oldW = e->batchW; e->oldH = e->batchH;
	return 0;
}

// The launches of the resamplers (pm_kernels.hip, "resampling"), one helper each: the pyramid and the level hand-off below and the self-test hook pmhip_resample
// (pm_engine.hip) launch through these, so the hook runs production's grid, block cap included.  n outputs in blocks of 256, at most `cap` blocks; the kernels stride.
static inline unsigned resampleBlocks(size_t n, size_t cap) { return (unsigned)std::min<size_t>((n + 255) / 256, cap); }
static void launchArea(hipStream_t st, const float* src, float* dst, int sw, int sh, int dw, int dh, int f, int nImg) {
	hipLaunchKernelGGL(pm_area_kernel, dim3(resampleBlocks((size_t)dw * dh * nImg, 65535)), dim3(256), 0, st, src, dst, sw, sh, dw, dh, f, nImg);
}
static void launchSkew(hipStream_t st, const float* src, float* dst, int w, int h, int nImg) {
	hipLaunchKernelGGL(pm_skew_kernel, dim3(resampleBlocks((size_t)w * h * nImg, 65535)), dim3(256), 0, st, src, dst, w, h, nImg);
}
static void launchQuad(hipStream_t st, const float* src, float4* dst, int w, int h, int nImg) {
	hipLaunchKernelGGL(pm_quad_kernel, dim3(resampleBlocks((size_t)w * h * nImg, 65535)), dim3(256), 0, st, src, dst, w, h, nImg);
}
// the quad copy of one source depth map of the geometric rounds (PMSrcView::dqBase)
static void launchDepthQuads(hipStream_t st, const float* map, float4* dst, int dw, int dh) {
	hipLaunchKernelGGL(pm_depth_quads_kernel, dim3(resampleBlocks((size_t)dw * dh, 8192)), dim3(256), 0, st, (const uint32_t*)map, (PMQuadBits*)dst, dw, dh);
}
static void launchMaskLevel(hipStream_t st, const unsigned char* src, unsigned char* dst, int sw, int sh, int dw, int dh) {
	hipLaunchKernelGGL(pm_mask_level_kernel, dim3(resampleBlocks((size_t)dw * dh, 4096)), dim3(256), 0, st, src, dst, sw, sh, dw, dh);
}
// the level hand-off of nT views (ups[0 .. nT), device memory)
static void launchNearestDown(hipStream_t st, const PMUpTask* ups, int nT, int sw, int sh, int dw, int dh, int f) {
	hipLaunchKernelGGL(pm_nearest_down_kernel, dim3(resampleBlocks((size_t)dw * dh, 4096), nT), dim3(256), 0, st, ups, sw, sh, dw, dh, f);
}
static void launchUpsample(hipStream_t st, const PMUpTask* ups, int nT, int sw, int sh, int dw, int dh, int nearestDepth) {
	hipLaunchKernelGGL(pm_upsample_kernel, dim3(resampleBlocks((size_t)dw * dh, 4096), nT), dim3(256), 0, st, ups, sw, sh, dw, dh, nearestDepth);
}
// (no call site in the estimation: the self-test hooks only)
static void launchNearestUpF(hipStream_t st, const float* src, float* dst, int sw, int sh, int dw, int dh) {
	hipLaunchKernelGGL(pm_nearest_up_f_kernel, dim3(resampleBlocks((size_t)dw * dh, 4096)), dim3(256), 0, st, src, dst, sw, sh, dw, dh);
}

static int buildPyramid(pmhip_engine* e) {
	if (!e->pyramidDirty) return 0;
	// every level is resampled from the full-resolution image (ScaleDepthData(fullRes, 1/2^l), SceneDensify.cpp:654)
	for (int l = 1; l <= e->nLevels; ++l) launchArea(e->stream, e->d_img[0], e->d_img[l], e->w, e->h, e->lw(l), e->lh(l), 1 << l, e->nImages);
	for (int l = 0; l <= e->nLevels; ++l) {
		launchSkew(e->stream, e->d_img[l], e->d_imgS[l], e->lw(l), e->lh(l), e->nImages);
		launchQuad(e->stream, e->d_img[l], e->d_imgQ[l], e->lw(l), e->lh(l), e->nImages);
	}
	HIPCHK(e, hipGetLastError());
	e->pyramidDirty = false;
	return 0;
}
// pyramids of the views that carry their own image size (source views only)
static int buildSidePyramids(pmhip_engine* e) {
	for (SceneView& v : e->views) {
		if (!v.sw || !v.sideDirty) continue;
		for (int l = 1; l <= e->nLevels; ++l) {
			const int lw = lvlSize(v.sw, l), lh = lvlSize(v.sh, l);
			if (lw < 1 || lh < 1 || !v.sImg[l]) break;      // a view too small for this level has no pyramid entry there (estimateBatch reports PMHIP_E_SIZE if the level is used)
			launchArea(e->stream, v.sImg[0], v.sImg[l], v.sw, v.sh, lw, lh, 1 << l, 1);
		}
		for (int l = 0; l <= e->nLevels; ++l) {
			const int lw = lvlSize(v.sw, l), lh = lvlSize(v.sh, l);
			if (lw < 1 || lh < 1 || !v.sImg[l]) break;
			launchSkew(e->stream, v.sImg[l], v.sImgS[l], lw, lh, 1);
			launchQuad(e->stream, v.sImg[l], v.sImgQ[l], lw, lh, 1);
		}
		HIPCHK(e, hipGetLastError());
		v.sideDirty = false;
	}
	return 0;
}

static PMKParams makeKParams(const PMHipParams& p) {
	// DepthEstimator ctor, libs/MVS/DepthMap.cpp:397-406 (same float expressions)
	PMKParams k;
	k.smoothBonusDepth = 1.f - p.fRandomSmoothBonus;
	k.smoothBonusNormal = (1.f - p.fRandomSmoothBonus) * 0.96f;
	k.smoothSigmaDepth = -1.f / (2.f * (p.fRandomSmoothDepth * p.fRandomSmoothDepth));
	const float sn = PM_FD2R(p.fRandomSmoothNormal);
	k.smoothSigmaNormal = -1.f / (2.f * (sn * sn));
	k.thMagnitudeSq = p.fDescriptorMinMagnitudeThreshold > 0 ? p.fDescriptorMinMagnitudeThreshold * p.fDescriptorMinMagnitudeThreshold : -1.f;
	k.angle1Range = PM_FD2R(p.fRandomAngle1Range);
	k.angle2Range = PM_FD2R(p.fRandomAngle2Range);
	k.thConfSmall = p.fNCCThresholdKeep * 0.66f;
	k.thConfBig = p.fNCCThresholdKeep * 0.9f;
	k.thConfRand = p.fNCCThresholdKeep * 1.1f;
	k.thRobust = p.fNCCThresholdKeep * 4.f / 3.f;
	k.thKeep = p.fNCCThresholdKeep;
	k.geoWeight = p.fEstimationGeometricWeight;
	k.depthRatio = p.fRandomDepthRatio;
	k.nRandomIters = p.nRandomIters;
	return k;
}

// nv = next_pow2(source views of the batch); a pixel gets PM_INIT_LANES lanes (fewer if it has fewer views) and a lane scores nv / lanes views.  P: pixels of the level.
#ifndef PM_INIT_LANES
#define PM_INIT_LANES 2   // 100 views: 4 lanes 51.8, 2 lanes 52.1, 1 lane 51.8 Mpix/s (profiles/r06_call8); one view per lane (round 5): 51.1 (r06_call7)
#endif
template <bool GEO, int MODE, int G, int VPL>
static void launchInitAs(size_t P, int nT, hipStream_t s, const PMTask* t, const PMKParams& kp, uint32_t pass) {
	constexpr int PPB = PM_BLOCK / G;
	hipLaunchKernelGGL((pm_init_kernel<G, GEO, MODE, VPL>), dim3((unsigned)((P + PPB - 1) / PPB), nT), dim3(PM_BLOCK), 0, s, t, kp, pass);
}
template <bool GEO, int MODE>
static void launchInit(int nv, size_t P, int nT, hipStream_t s, const PMTask* t, const PMKParams& kp, uint32_t pass) {
	constexpr int L = PM_INIT_LANES;
	switch (nv) {
	case 1: launchInitAs<GEO, MODE, 1, 1>(P, nT, s, t, kp, pass); break;
	case 2: launchInitAs<GEO, MODE, 2, 1>(P, nT, s, t, kp, pass); break;
	case 4: launchInitAs<GEO, MODE, (L < 4 ? L : 4), 4 / (L < 4 ? L : 4)>(P, nT, s, t, kp, pass); break;
	case 8: launchInitAs<GEO, MODE, L, 8 / L>(P, nT, s, t, kp, pass); break;
	default: launchInitAs<GEO, MODE, 2 * L, 16 / (2 * L)>(P, nT, s, t, kp, pass); break;
	}
}
// Lanes per pixel for a batch whose views have at most maxSrc sources: G * VPL = next_pow2(maxSrc).  `lanes` (PMHipTuning::sweepLanes or the built-in
// default) caps G; VPL is what is left, limited to the instantiated mappings.
static void sweepMapping(int maxSrc, int lanes, int& G, int& VPL) {
	int NV = 1; while (NV < maxSrc) NV <<= 1;
	G = NV; VPL = 1;
	while (G > 4 && G > lanes && VPL < 4) { G >>= 1; VPL <<= 1; }   // a pixel gets at least a quad of lanes (one smoothness slot per lane)
	if (G < 4) G = 4;
	if (G == 8 && VPL > 2) { G <<= 1; VPL >>= 1; }   // (8,4) is not instantiated
}

// workgroups of a sweep launch whose workgroups hold ppw pixels each: the launch's pixels are numbered tile by tile, PMStep::len per tile
static unsigned stepBlocks(const PMStep& st, int ppw) { return (unsigned)(((long)st.len * st.ntx * st.nty + ppw - 1) / ppw); }
// (tiled sweeps are instantiated for the quad-buffer addressing only: a batch with source views of their own image size runs the reference's sweep)
template <bool GEO, bool BUF>
static bool launchSweep2(int G, int VPL, int nTasks, hipStream_t s, const PMTask* t, const PMKParams& kp, const PMStep& st, uint32_t pass) {
	const dim3 grid(stepBlocks(st, 64 / G), (unsigned)nTasks);
	const bool tiled = st.ntx * st.nty > 1;
#define PM_SWEEP2_CASE(g, vpl) case (g) * 16 + (vpl): \
		if constexpr (BUF) { if (tiled) { hipLaunchKernelGGL((pm_sweep2_kernel<g, vpl, GEO, BUF, true>), grid, dim3(64), 0, s, t, kp, st, pass); return true; } } \
		hipLaunchKernelGGL((pm_sweep2_kernel<g, vpl, GEO, BUF, false>), grid, dim3(64), 0, s, t, kp, st, pass); return true
	switch (G * 16 + VPL) {
	PM_SWEEP2_CASE(4, 1); PM_SWEEP2_CASE(8, 1); PM_SWEEP2_CASE(16, 1);
	PM_SWEEP2_CASE(4, 2); PM_SWEEP2_CASE(8, 2);
	PM_SWEEP2_CASE(4, 4);
	default: return false;
	}
#undef PM_SWEEP2_CASE
}

// the eight-wide speculative kernel (one wave per pixel; batches of one or two views, never with tiles): launch k of the reference's one-tile sweep as an anti-diagonal
template <bool GEO, bool BUF>
static void launchSweepWide(int nTasks, hipStream_t s, const PMTask* t, const PMKParams& kp, const PMStep& st, int lw, int lh, uint32_t pass) {
	const int dLo = 2 * PM_HW, dHi = (lw - 1 - PM_HW) + (lh - 1 - PM_HW);
	const int d = st.dir == 0 ? dLo + st.k : dHi - st.k;
	const int xlo = std::max(PM_HW, d - (lh - 1 - PM_HW)), xhi = std::min(lw - 1 - PM_HW, d - PM_HW);
	const int count = xhi - xlo + 1;
	if (count <= 0) return;
	hipLaunchKernelGGL((pm_sweep_wide_kernel<GEO, BUF>), dim3((unsigned)count, (unsigned)nTasks), dim3(64), 0, s, t, kp, st.dir, d, xlo, count, pass);
}
// the speculative kernel at 4 or 2 hypotheses per round (pm_wide_n.hip; PMHipTuning::wideHyps): 2 or 4 pixels per wave
template <bool GEO, bool BUF>
static void launchSweepWideN(int hyps, int nTasks, hipStream_t s, const PMTask* t, const PMKParams& kp, PMStep st, uint32_t pass) {
	const dim3 grid(stepBlocks(st, 8 / hyps), (unsigned)nTasks);
	if constexpr (BUF) if (st.ntx * st.nty > 1) {
		if (hyps == 4) hipLaunchKernelGGL((pm_sweep_widen_kernel<GEO, 4, BUF, true>), grid, dim3(64), 0, s, t, kp, st, pass);
		else hipLaunchKernelGGL((pm_sweep_widen_kernel<GEO, 2, BUF, true>), grid, dim3(64), 0, s, t, kp, st, pass);
		return;
	}
	if (hyps == 4) hipLaunchKernelGGL((pm_sweep_widen_kernel<GEO, 4, BUF, false>), grid, dim3(64), 0, s, t, kp, st, pass);
	else hipLaunchKernelGGL((pm_sweep_widen_kernel<GEO, 2, BUF, false>), grid, dim3(64), 0, s, t, kp, st, pass);
}
// one launch of a sweep for one view group with the kernel the batch calls for; false: the (lanes, views per lane) mapping is not instantiated
template <bool GEO, bool BUF>
static bool launchDiagonal(bool wide, int hyps, int G2, int V2, int nTasks, hipStream_t st, const PMTask* t, const PMKParams& kp, const PMStep& sp, int lw, int lh, uint32_t pass) {
	if (wide && hyps < 8) { launchSweepWideN<GEO, BUF>(hyps, nTasks, st, t, kp, sp, pass); return true; }
	if (wide) { launchSweepWide<GEO, BUF>(nTasks, st, t, kp, sp, lw, lh, pass); return true; }
	return launchSweep2<GEO, BUF>(G2, V2, nTasks, st, t, kp, sp, pass);
}

#ifdef PM_PROBES
// measurement builds (-DPM_PROBES, tools/): never part of the product library
static int g_probeRepeat = 1;
extern "C" int pmhip_probe_set(int key, int val) { if (key == 0) g_probeRepeat = val < 1 ? 1 : val; return 0; }
#endif
static size_t evBeginOn(pmhip_engine* e, int kind, hipStream_t st) {
	if (!e->statsOn) return 0;
	pmhip_engine::Ev ev; ev.kind = kind;
	hipEventCreate(&ev.a); hipEventCreate(&ev.b);
	hipEventRecord(ev.a, st);
	e->events.push_back(ev);
	return e->events.size() - 1;
}
static void evEndOn(pmhip_engine* e, size_t idx, hipStream_t st) {
	if (!e->statsOn) return;
	hipEventRecord(e->events[idx].b, st);
}
static void evBegin(pmhip_engine* e, int kind) { evBeginOn(e, kind, e->stream); }
static void evEnd(pmhip_engine* e) { if (e->statsOn) hipEventRecord(e->events.back().b, e->stream); }

// One DepthMapsData::EstimateDepthMap (SceneDensify.cpp:616-805) for each view of the batch, concurrently.
// ids: views of ONE size class (cw x ch: the scene's size, or the own size these views carry); estimateBatch below splits a batch into its classes.
static int estimateClass(pmhip_engine* e, const int32_t* ids, int nB, int cw, int ch, const PMHipParams& p, int nGeometricIter) {
	const unsigned iterBegin = nGeometricIter < 0 ? 0u : p.nEstimationIters + (unsigned)nGeometricIter;
	const unsigned iterEnd = nGeometricIter < 0 ? p.nEstimationIters : iterBegin + 1;
	const int S = nGeometricIter < 0 ? (int)p.nSubResolutionLevels : 0;
	if (lvlSize(cw, S) < 2 * PM_HW + 1 || lvlSize(ch, S) < 2 * PM_HW + 1) { e->err = "image too small for this many sub-resolution levels"; return PMHIP_E_SIZE; }
	const PMKParams kp = makeKParams(p);
	const bool geo = nGeometricIter >= 0;
	bool anyMask = false;
	for (unsigned char m : e->hasMask) anyMask = anyMask || m;
	const int nearestDepth = (e->maskMode < 0 ? anyMask : e->maskMode != 0) ? 1 : 0;
	if (anyMask && e->maskDirty) {
		for (int l = 1; l <= e->nLevels; ++l) {
			const size_t Pm = (size_t)e->lw(l) * e->lh(l);
			for (int i = 0; i < e->nImages; ++i) if (e->hasMask[i]) {
				const SceneView& mv = e->views[i];
				if (mv.sw) {   // a view with its own size: its own level masks
					const int mlw = lvlSize(mv.sw, l), mlh = lvlSize(mv.sh, l);
					if (mlw < 1 || mlh < 1 || !mv.oMask[l]) continue;
					launchMaskLevel(e->stream, mv.oMask[0], mv.oMask[l], mv.sw, mv.sh, mlw, mlh);
				} else
					launchMaskLevel(e->stream, e->d_mask[0] + (size_t)e->w * e->h * i, e->d_mask[l] + Pm * i, e->w, e->h, e->lw(l), e->lh(l));
			}
		}
		HIPCHK(e, hipGetLastError());
		e->maskDirty = false;
	}
	int maxSrc = 0;
	bool buf = e->quadBuffer != 0;
	for (int b = 0; b < nB; ++b) {
		const int id = ids[b];
		if (id < 0 || id >= e->nImages || !e->views[id].set) { e->err = "view not set"; return PMHIP_E_ARG; }
		const SceneView& v = e->views[id];
		if (v.nNb < 1) { e->err = "view has no source views"; return PMHIP_E_ARG; }
		for (int k = 0; k < v.nNb; ++k) if (v.nb[k] < 0 || v.nb[k] >= e->nImages || !e->views[v.nb[k]].set) { e->err = "neighbour view not set"; return PMHIP_E_ARG; }
		maxSrc = std::max(maxSrc, v.nNb);
		for (int k = 0; k < v.nNb; ++k) if (e->views[v.nb[k]].sw) buf = false;   // a source image of its own size is not in the level's quad buffer
	}
	// the buffer path addresses a sample by a 32-bit entry index into the level's quad buffer (PMTask::qCount, PMSrcView::qBase): a level-0 buffer of 2^32 entries or more
	// (about 330 views of 3840x2160) goes through the views' own pointers instead
	if (e->skewPitch(0) * (size_t)e->nImages > 0xFFFFFFFFull) buf = false;
	int G = 1; while (G < maxSrc) G <<= 1;          // init kernel: one view per lane
	int SG = G, VPL = 1;                             // sweep kernel: (lanes per pixel, views per lane)
	sweepMapping(maxSrc, e->sweepLanes > 0 ? e->sweepLanes : ((nB >= PMHIP_LANES4_FROM || (e->tileW > 0 && e->tileH > 0)) && maxSrc > 4 ? 4 : 16), SG, VPL);
	// latency mode (one wave per pixel, pm_sweep_wide_kernel) for batches too small to fill the GPU with one wave per 64 / G pixels
	const bool wideBatch = nB <= e->wideMaxViews && maxSrc <= 8;
	const size_t P0 = (size_t)cw * ch;                      // this class's pixels; the scene arrays are indexed with the scene's own
	const size_t P0s = (size_t)e->w * e->h;
	// the staging buffers are reused by the next call (and by the next size class): make sure the previous copies are done
	HIPCHK(e, hipStreamSynchronize(e->stream));
	// geometric round: the depth map a source view is read through -- the one the caller installed (pmhip_scene_set_source_depth), its own previous-round map (a view of
	// its own size) or its part of the scene's snapshot -- and the quad copies of exactly the maps this call reads, derived now, on the engine's stream, before the
	// view groups fork: the row-major maps are written by commits, copies, uploads and by callers through their device pointers, so no copy outlives a call
	struct GeoMap { const float* map; int dw, dh; size_t ofs; };
	std::vector<GeoMap> geoMaps;
	auto geoMapOf = [&](int nbId) -> GeoMap {
		const SceneView& sv = e->views[nbId];
		if (sv.sDepth) return {sv.sDepth, sv.dw, sv.dh, 0};
		if (sv.sw) return {sv.oSnap, sv.sw, sv.sh, 0};
		return {e->d_snap + P0s * nbId, e->w, e->h, 0};
	};
	auto geoQuadsOf = [&](const float* map) -> size_t {   // first entry of the map's copy in d_geoQ
		for (const GeoMap& m : geoMaps) if (m.map == map) return m.ofs;
		return 0;
	};
	// (a batch whose every launch goes to the speculative kernels -- wideBatch without tiles, pass B below -- never runs pm_sweep2_kernel, the only reader of the copies:
	// it derives none and holds no memory for them; pass B refuses a geometric launch of that kernel without them, should the two rules ever part)
	const bool quadsDerived = geo && !(wideBatch && !(e->tileW > 0 && e->tileH > 0));
	if (quadsDerived) {
		std::vector<char> seen((size_t)e->nImages, 0);
		size_t total = 0;
		for (int b = 0; b < nB; ++b) {
			const SceneView& v = e->views[ids[b]];
			for (int k = 0; k < v.nNb; ++k) if (!seen[v.nb[k]]) {
				seen[v.nb[k]] = 1;
				GeoMap m = geoMapOf(v.nb[k]);
				m.ofs = total; total += (size_t)m.dw * m.dh;
				geoMaps.push_back(m);
			}
		}
		if (total > 0xFFFFFFFFull) { e->err = "geometric round: the quad copies of the source depth maps of one call hold 2^32 entries or more (PMSrcView::dqBase)"; return PMHIP_E_SIZE; }
		HIPCHK(e, e->d_geoQ.reserve(total));
		for (const GeoMap& m : geoMaps) launchDepthQuads(e->stream, m.map, e->d_geoQ + m.ofs, m.dw, m.dh);
		HIPCHK(e, hipGetLastError());
	}
	for (int l = S; l >= 0; --l) {
		const int lw = lvlSize(cw, l), lh = lvlSize(ch, l);
		const size_t Pl = (size_t)lw * lh;
		const int slw = e->lw(l), slh = e->lh(l);            // the scene's size at this level: source views that live in the scene arrays
		const size_t Pls = (size_t)slw * slh;
		PMTask* ht = e->h_tasks + (size_t)l * e->batchCap;
		PMUpTask* hu = e->h_ups + (size_t)l * e->batchCap;
		for (int b = 0; b < nB; ++b) {
			const int id = ids[b];
			const SceneView& v = e->views[id];
			PMTask& t = ht[b];
			memset(&t, 0, sizeof(t));
			if (quadsDerived) { const uintptr_t q = (uintptr_t)(const float4*)e->d_geoQ; t.geoQLo = (uint32_t)q; t.geoQHi = (uint32_t)((unsigned long long)q >> 32); }
			if (l == 0) {
				t.depth = e->depthOf(id); t.normal = e->normalOf(id); t.conf = e->confOf(id);
				t.prior = (S > 0) ? e->d_lvl[0] + P0 * b : nullptr;
			} else {
				float* base = e->d_lvl[l] + Pl * 6 * b;
				t.depth = base; t.normal = base + Pl; t.conf = base + Pl * 4;
				t.prior = (l < S) ? base + Pl * 5 : nullptr;
			}
			if (e->tileW > 0 && e->tileH > 0) { float* ob = e->d_old[l] + Pl * 5 * b; t.depthOld = ob; t.normalOld = ob + Pl; t.confOld = ob + Pl * 4; }
			if (v.sw) { t.ref = v.sImg[l]; t.refS = v.sImgS[l]; }
			else { t.ref = e->d_img[l] + Pls * id; t.refS = e->d_imgS[l] + Pls * id; }
			t.qArr = e->d_imgQ[l]; t.qCount = (unsigned)(e->skewPitch(l) * (size_t)e->nImages);
			t.mask = (anyMask && e->hasMask[id]) ? (v.sw ? v.oMask[l] : e->d_mask[l] + Pls * id) : nullptr;
			t.w = lw; t.h = lh; t.nSrc = v.nNb;
			double K0[9];
			if (l == 0) memcpy(K0, v.K, sizeof(K0)); else scaleK(v.K, cw, ch, lw, lh, K0);
			inv33(K0, t.Hr);
			t.hrUpper = (t.Hr[1] == 0.0 && t.Hr[3] == 0.0 && t.Hr[6] == 0.0 && t.Hr[7] == 0.0) ? 1 : 0;
			t.fx = K0[0]; t.fy = K0[4]; t.cx = K0[2]; t.cy = K0[5];
			t.dMin = v.dMin; t.dMax = v.dMax; t.dMinSqr = sqrtf(v.dMin); t.dMaxSqr = sqrtf(v.dMax);
			t.k0 = p.seed; t.k1base = v.id * 0x9E3779B1u;
			double R0T[9]; transp33(v.R, R0T);
			double KR0[9]; mul33(K0, v.R, KR0);
			for (int k = 0; k < v.nNb; ++k) {
				const SceneView& sv = e->views[v.nb[k]];
				PMSrcView& s = t.src[k];
				double Kj[9];
				if (sv.sw) {
					// a source image of its own size: its own pyramid, its camera scaled from its own size (ScaleDepthData, SceneDensify.cpp:586-588)
					const int jw = lvlSize(sv.sw, l), jh = lvlSize(sv.sh, l);
					if (jw < 3 || jh < 3) { e->err = "source image too small for this many sub-resolution levels"; return PMHIP_E_SIZE; }
					s.img = sv.sImg[l]; s.imgQ = sv.sImgQ[l]; s.w = jw; s.h = jh;
					if (l == 0) memcpy(Kj, sv.K, sizeof(Kj)); else scaleK(sv.K, sv.sw, sv.sh, jw, jh, Kj);
				} else {
					s.img = e->d_img[l] + Pls * v.nb[k];
					s.imgQ = e->d_imgQ[l] + e->skewPitch(l) * v.nb[k];
					s.qBase = (unsigned)(e->skewPitch(l) * (size_t)v.nb[k]);
					s.w = slw; s.h = slh;
					if (l == 0) memcpy(Kj, sv.K, sizeof(Kj)); else scaleK(sv.K, e->w, e->h, slw, slh, Kj);
				}
				double KR[9], dC[3];
				mul33(Kj, sv.R, KR);
				mul33(KR, R0T, s.Hl);
				for (int i = 0; i < 3; ++i) dC[i] = v.C[i] - sv.C[i];
				mul31(KR, dC, s.Hm);
				s.depth = nullptr;
				if (geo) {
					// ViewData::Init geometric part, DepthMap.h:179-184.  cameraDepthMap is the neighbour's own camera when the map is the scene's
					// snapshot, or the camera stored with the map the caller installed (pmhip_scene_set_source_depth), whose size may differ too
					double tm[9], vv[3], RdT[9], iKd[9], t2[9], KdRd[9];
					const double* Kd = Kj; const double* Rd = sv.R; const double* Cd = sv.C;
					if (sv.sDepth) { Kd = sv.Kd; Rd = sv.Rd; Cd = sv.Cd; }   // (a view's own previous-round map has its own camera = Kj at level 0)
					const GeoMap gm = geoMapOf(v.nb[k]);
					s.depth = gm.map; s.dqBase = (unsigned)geoQuadsOf(gm.map); s.dw = gm.dw; s.dh = gm.dh;
					mul33(Kd, Rd, KdRd);
					mul33(KdRd, R0T, tm); for (int i = 0; i < 9; ++i) s.Tl[i] = (float)tm[i];
					for (int i = 0; i < 3; ++i) dC[i] = v.C[i] - Cd[i];
					mul31(KdRd, dC, vv); for (int i = 0; i < 3; ++i) s.Tm[i] = (float)vv[i];
					transp33(Rd, RdT); mul33(KR0, RdT, tm); invK(Kd, iKd); mul33(tm, iKd, t2);
					for (int i = 0; i < 9; ++i) s.Tr[i] = (float)t2[i];
					for (int i = 0; i < 3; ++i) dC[i] = Cd[i] - v.C[i];
					mul31(KR0, dC, vv); for (int i = 0; i < 3; ++i) s.Tn[i] = (float)vv[i];
				}
			}
			// level hand-off descriptors
			PMUpTask& u = hu[b];
			memset(&u, 0, sizeof(u));
			if (l == S && S > 0) { // coarsest: INTER_NEAREST of the caller's initial estimate
				u.sdepth = e->depthOf(id); u.snormal = e->normalOf(id); u.ddepth = t.depth; u.dnormal = t.normal; u.dprior = nullptr;
			} else if (l < S) {
				const size_t Pc = (size_t)lvlSize(cw, l + 1) * lvlSize(ch, l + 1);
				float* cb = e->d_lvl[l + 1] + Pc * 6 * b;
				u.sdepth = cb; u.snormal = cb + Pc; u.ddepth = t.depth; u.dnormal = t.normal; u.dprior = const_cast<float*>(t.prior);
			}
		}
		HIPCHK(e, hipMemcpyAsync(e->d_tasks + (size_t)l * e->batchCap, ht, sizeof(PMTask) * nB, hipMemcpyHostToDevice, e->stream));
		HIPCHK(e, hipMemcpyAsync(e->d_ups + (size_t)l * e->batchCap, hu, sizeof(PMUpTask) * nB, hipMemcpyHostToDevice, e->stream));
	}
	// ---- the pass as a sequence of steps that is the same for every view group: per level {hand-off, ScoreDepthMapTmp, sweeps of one launch per anti-diagonal}, EndDepthMapTmp.
	// A view group runs ALL of them on its own stream (views are independent; the steps of one view are not); the groups start together and meet again at the end of the
	// call.  Scheduling only: the maps cannot depend on it.
	// Measured and not kept (round 5, MI355X, full schedule at 1920x1080; all bit-identical):
	//  * group g + 1 starting behind group g, so that one group's short diagonals, coarse levels and init pass run under another group's long diagonals (commit c352a63,
	//    PMHipTuning::groupOffset): slower for every offset and batch size -- 100 views 47.8 -> 46.5 (5 % of the pass) -> 41.9 Mpix/s (40 %), 13 views 26.6 -> 25.4 -> 20.0
	//    (profiles/r05_call1_groups_*.log).  The late group also finishes late, and a group's launch chain runs slower beside the other's long diagonals than beside its ramps.
	//  * the groups waiting for each other before every sweep (round 4's fork / join per sweep): no difference (48.8 vs 48.8, profiles/r05_call4_ab_100.log).
	//  * the views of a group staggered along the pass, so that every launch mixes anti-diagonals, sweeps and levels and carries about the mean number of pixels
	//    (profiles/r05_view_stagger_experiment.diff): 100 views 46.2 -> 44.0 (5 steps per view) -> 37.7 (30) -> 35.0 Mpix/s (100), profiles/r05_call3_stagger_*.log.  A launch
	//    lasts one wave-visit at whatever fill, so evening out the fill buys nothing, while every step of the longer chain then costs the heavy kernel's visit.
	struct Step { int kind, l; unsigned iter; int k; };   // kind 0: level hand-off, 1: init pass, 2: launch k of sweep `iter`, 3: finalize, 4: snapshot of the maps before a tiled sweep
	std::vector<Step> steps;
	// a level's sweep geometry (PMStep): the reference's sweep is one tile = all pixels that take part; pmhip_set_sweep_tiles cuts them into tiles
	const bool tilesOn = e->tileW > 0 && e->tileH > 0;
	if (tilesOn && !buf) { e->err = "tiled sweeps (pmhip_set_sweep_tiles) address the level's quad buffer: not with source views of their own image size, PMHipTuning::quadBuffer = 2 or a level-0 buffer of 2^32 entries"; return PMHIP_E_ARG; }
	auto stepOf = [&](int l, int dir, int k) {
		const int vw = lvlSize(cw, l) - 2 * PM_HW, vh = lvlSize(ch, l) - 2 * PM_HW;
		PMStep sp; sp.dir = dir; sp.k = k;
		sp.tw = tilesOn ? std::min(e->tileW, vw) : vw; sp.th = tilesOn ? std::min(e->tileH, vh) : vh;
		sp.ntx = (vw + sp.tw - 1) / sp.tw; sp.nty = (vh + sp.th - 1) / sp.th;
		sp.len = std::max(0, std::min(std::min(k, sp.tw + sp.th - 2 - k), std::min(sp.tw, sp.th) - 1) + 1);
		return sp;
	};
	for (int l = S; l >= 0; --l) {
		if (S > 0) steps.push_back({0, l, 0u, 0});
		steps.push_back({1, l, 0u, 0});
		const PMStep g0s = stepOf(l, 0, 0);
		const int nDiag = g0s.tw + g0s.th - 1;
		for (unsigned iter = iterBegin; iter < iterEnd; ++iter) {
			if (g0s.ntx * g0s.nty > 1) steps.push_back({4, l, iter, 0});
			for (int k = 0; k < nDiag; ++k) steps.push_back({2, l, iter, k});
		}
	}
	steps.push_back({3, 0, 0u, 0});
	const long nSteps = (long)steps.size();
	const int NG = std::max(1, std::min(e->nGroups, nB));
	// group g's stream: the engine's own for a single group.  (Letting group 0 of several sweep on the engine's stream, or more than three groups, falls off a cliff:
	// 13 views 27 -> 15.6 Mpix/s, whatever GPU_MAX_HW_QUEUES says -- profiles/r04_call10_lanes_13.log.)
	auto gs = [&](int g) { return NG > 1 ? e->gstream[g] : e->stream; };
	auto g0 = [&](int g) { return (int)((long)nB * g / NG); };
	const size_t evWall = evBeginOn(e, 2, e->stream);
	if (NG > 1) {
		HIPCHK(e, hipEventRecord(e->forkEv, e->stream));
		for (int g = 0; g < NG; ++g) HIPCHK(e, hipStreamWaitEvent(gs(g), e->forkEv, 0));
	}
	float thFinal = p.fNCCThresholdKeep;   // EndDepthMapTmp: threshold x1.333 when geometric rounds will follow, SceneDensify.cpp:774-776
	if (nGeometricIter < 0 && p.nEstimationGeometricIters) thFinal *= 1.333f;
	size_t evSweep[16] = {}; bool evOpen[16] = {};
	size_t nLaunched = 0;
	const char* sweepErr = nullptr;
	const auto hostT0 = std::chrono::steady_clock::now();
	auto issue = [&](int g, const Step& sp) -> bool {
		const int l = sp.l, s0 = g0(g), nT = g0(g + 1) - s0;
		const int lw = lvlSize(cw, l), lh = lvlSize(ch, l);
		const size_t Pl = (size_t)lw * lh;
		const PMTask* dt = e->d_tasks + (size_t)l * e->batchCap + s0;
		const PMUpTask* du = e->d_ups + (size_t)l * e->batchCap + s0;
		hipStream_t st = gs(g);
		if (sp.kind != 2 && evOpen[g]) { evEndOn(e, evSweep[g], st); evOpen[g] = false; }
		switch (sp.kind) {
		case 0: {
			if (l == S) launchNearestDown(st, du, nT, cw, ch, lw, lh, 1 << S);
			else launchUpsample(st, du, nT, lvlSize(cw, l + 1), lvlSize(ch, l + 1), lw, lh, nearestDepth);
			return true;
		}
		case 1: {
			// pass A: ScoreDepthMapTmp, row-major pixels.  (Round 4, 24 views resident: the pass was latency-bound, and the same evaluation on anti-diagonals with the sweep's optimistic
			// quad rows was 9 % SLOWER -- the maps are row-major, and a wave that walks a diagonal reads and writes them one cache line per lane:
			// profiles/r04_call14_diagonal_init_kernel_stats.csv.  Round 6, 100 views resident: bound by VALU issue (0.89 busy); row-major pixels WITH the optimistic quad rows: +0.8 %.)
			const uint32_t passInit = (uint32_t)l * 64u + 32u + (geo ? 16u + (uint32_t)nGeometricIter : 0u);
			const size_t ev = evBeginOn(e, 1, st);
			// (optimistic rows from the level's quad buffer; the guarded rows from the row-major images for batches that read source views outside that buffer)
			if (buf && PM_INIT_MODE == 2) { if (geo) launchInit<true, 2>(G, Pl, nT, st, dt, kp, passInit); else launchInit<false, 2>(G, Pl, nT, st, dt, kp, passInit); }
			else { if (geo) launchInit<true, 0>(G, Pl, nT, st, dt, kp, passInit); else launchInit<false, 0>(G, Pl, nT, st, dt, kp, passInit); }
			evEndOn(e, ev, st);
			if (e->statsOn && g == 0) e->stats.initLaunches += 1;
			return true;
		}
		case 2: {
			// pass B: one launch per anti-diagonal.  The kernels compute the same bits, so the choice is per launch: the speculative kernels (more lanes per pixel, shorter
			// dependent chain) for batches and for diagonals too small to fill the GPU with 64 / G pixels per wave
			const int dir = (int)(sp.iter % 2u);
			const uint32_t pass = (uint32_t)l * 64u + sp.iter;
			const PMStep ps = stepOf(l, dir, sp.k);
			// pixels of this launch: a full tile's k-th anti-diagonal holds min(k, tw - 1, th - 1, tw + th - 2 - k) + 1 of them (the tiles at the right and bottom border fewer)
			const int perTile = ps.len;
			if (perTile <= 0) return true;
			const bool tiled = ps.ntx * ps.nty > 1;
			if (!evOpen[g]) { evSweep[g] = evBeginOn(e, 0, st); evOpen[g] = e->statsOn; }
			const long npx = (long)perTile * ps.ntx * ps.nty * nT;
			// larger batches: launches of at most widePixels pixels AND at most PMHIP_WIDE_DIAGONAL pixels per view go to the two-wide kernel (round 6: 100 views in two groups are
			// best at 17-20 000 pixels, 50 views at <= 10 000 -- the same ~400 pixels of diagonal per view: profiles/r06_call18, r06_call19)
			const long wpx = tiled ? (long)e->widePixels : std::min<long>(e->widePixels, (long)PMHIP_WIDE_DIAGONAL * nT);
			const bool wide = (wideBatch && !(tiled && npx > e->widePixels)) || (maxSrc <= 8 && npx <= wpx);
			int hyps = (wideBatch && e->wideHyps > 0) ? e->wideHyps : ((nB <= 2 || npx <= e->wide8Pixels) ? 8 : 2);
			if (tiled && hyps == 8) hyps = 2;   // (the eight-wide kernel walks whole anti-diagonals of the map)
			if (geo && !wide && !quadsDerived) { sweepErr = "geometric round: a pm_sweep2_kernel launch without the quad copies of the source depth maps"; return false; }
			++nLaunched;
#ifdef PM_PROBES
			for (int r = 1; r < g_probeRepeat; ++r)   // (measurement builds only) the same diagonal again, back to back: what does a launch find in the caches its predecessor filled?
				geo ? (buf ? launchDiagonal<true, true>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass) : launchDiagonal<true, false>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass))
				    : (buf ? launchDiagonal<false, true>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass) : launchDiagonal<false, false>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass));
#endif
			return geo ? (buf ? launchDiagonal<true, true>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass) : launchDiagonal<true, false>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass))
			           : (buf ? launchDiagonal<false, true>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass) : launchDiagonal<false, false>(wide, hyps, SG, VPL, nT, st, dt, kp, ps, lw, lh, pass));
		}
		case 4: {
			// tiled sweeps: the maps as this sweep finds them, for the reads across tile borders
			hipLaunchKernelGGL(pm_snapshot_kernel, dim3((unsigned)std::min<size_t>((Pl + 255) / 256, 2048), nT), dim3(256), 0, st, dt, Pl);
			return true;
		}
		default:
			hipLaunchKernelGGL(pm_finalize_kernel, dim3((unsigned)std::min<size_t>((P0 + 255) / 256, 4096), nT), dim3(256), 0, st, e->d_tasks + s0, thFinal);
			return true;
		}
	};
	// the host feeds the groups' streams in turn, step by step
	for (long i = 0; i < nSteps; ++i)
		for (int g = 0; g < NG; ++g)
			if (!issue(g, steps[i])) { e->err = sweepErr ? sweepErr : "sweep kernel: (lanes per pixel, views per lane) mapping not instantiated"; return PMHIP_E_ARG; }
	if (NG > 1) for (int g = 0; g < NG; ++g) { HIPCHK(e, hipEventRecord(e->joinEv[g], gs(g))); HIPCHK(e, hipStreamWaitEvent(e->stream, e->joinEv[g], 0)); }
	evEndOn(e, evWall, e->stream);
	HIPCHK(e, hipGetLastError());
	if (e->statsOn) {
		e->stats.sweepLaunches += nLaunched;
		e->stats.sweepHostMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - hostT0).count();
		// algorithmic bytes of the sweeps, SURVEY.md 8(d): P_l * [4(1+N) + 20 + 20 + 4[prior] + 4N[geo]] per view and sweep
		for (int l = S; l >= 0; --l) {
			const size_t Pl = (size_t)lvlSize(cw, l) * lvlSize(ch, l);
			double bytes = 0;
			for (int b = 0; b < nB; ++b) { const int N = e->views[ids[b]].nNb; bytes += (double)Pl * (4.0 * (1 + N) + 40.0 + (l < S ? 4.0 : 0.0) + (geo ? 4.0 * N : 0.0)); }
			e->stats.sweepBytes += bytes * (iterEnd - iterBegin);
			e->stats.sweepPixels += (uint64_t)Pl * nB * (iterEnd - iterBegin);
		}
	}
	for (int b = 0; b < nB; ++b) e->views[ids[b]].hasMaps = true;
	return 0;
}


// One DepthMapsData::EstimateDepthMap for each view of the batch.  The reference sizes every depth map on its own image (DepthMapsData::InitViews, SceneDensify.cpp:306-459):
// the views of a batch are grouped by size -- the scene's, or the one a view carries (pmhip_scene_set_view_sized) -- and each size class sweeps on its own.
static int estimateBatch(pmhip_engine* e, const int32_t* ids, int nB, const PMHipParams& p, int nGeometricIter) {
	if (nB <= 0) return 0;
	if (nGeometricIter >= 0 && !e->geom) { e->err = "geometric round requested but engine initialised with bGeomConsistency == 0"; return PMHIP_E_STATE; }
	const int S = nGeometricIter < 0 ? (int)p.nSubResolutionLevels : 0;
	if (S > e->nLevels || S > 3) { e->err = "nSubResolutionLevels exceeds the pyramid allocated by pmhip_scene_create"; return PMHIP_E_ARG; }
	int rc = buildPyramid(e); if (rc) return rc;
	rc = buildSidePyramids(e); if (rc) return rc;
	std::vector<std::pair<int, int>> sizes; std::vector<std::vector<int32_t>> members;   // size classes in order of first appearance
	int maxN = 0, maxW = 0, maxH = 0;
	for (int b = 0; b < nB; ++b) {
		const int id = ids[b];
		if (id < 0 || id >= e->nImages || !e->views[id].set) { e->err = "view not set"; return PMHIP_E_ARG; }
		const std::pair<int, int> sz(e->vw(id), e->vh(id));
		size_t c = 0; while (c < sizes.size() && sizes[c] != sz) ++c;
		if (c == sizes.size()) { sizes.push_back(sz); members.emplace_back(); }
		members[c].push_back(id);
		maxN = std::max(maxN, (int)members[c].size()); maxW = std::max(maxW, sz.first); maxH = std::max(maxH, sz.second);
	}
	rc = ensureBatch(e, maxN, maxW, maxH); if (rc) return rc;
	rc = ensureOld(e); if (rc) return rc;
	for (size_t c = 0; c < sizes.size(); ++c) {
		rc = estimateClass(e, members[c].data(), (int)members[c].size(), sizes[c].first, sizes[c].second, p, nGeometricIter);
		if (rc) return rc;
	}
	return 0;
}
