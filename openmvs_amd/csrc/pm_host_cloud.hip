// pm_host_cloud.hip -- host side of the finishing steps and the visibility filter on the fused cloud (kernels: pm_cloud.hip, pm_cloud_filter.hip).
// Part of the translation unit pm_engine.hip.
// ---- the finishing steps on the fused cloud (pm_cloud.hip; SceneDensify.cpp:1724-1737) --------------------------------------------
static int ensureCloudPoints(pmhip_engine* e, size_t n) {
	auto& c = e->cl;
	if (!c.misc) { HIPCHK(e, c.misc.alloc(16)); HIPCHK(e, c.sample.alloc(3 * 1024)); }
	HIPCHK(e, c.hole.reserve(n + 1)); HIPCHK(e, c.nxt.reserve(n + 1)); HIPCHK(e, c.cellOf.reserve(n + 1)); HIPCHK(e, c.spts.reserve(n + 1));
	const size_t nT = (std::max(n, c.counts.n) + PMCL_TILE - 1) / PMCL_TILE + 1;
	HIPCHK(e, c.tileSums.reserve(nT)); HIPCHK(e, c.tileOff.reserve(nT));
	return 0;
}

// cameras (P composed like Camera::ComposeP) and the colour image of every view
static int uploadCloudViews(pmhip_engine* e) {
	auto& c = e->cl; auto& f = e->fu;
	const int N = e->nImages;
	HIPCHK(e, c.cams.reserve(N)); HIPCHK(e, c.imgs.reserve(N)); HIPCHK(e, c.used.reserve((size_t)N + 1));
	std::vector<PMFuseCam> hc((size_t)N); std::vector<PMClImg> hi((size_t)N);
	const size_t P0 = (size_t)e->w * e->h;
	for (int i = 0; i < N; ++i) {
		memset(&hc[i], 0, sizeof(PMFuseCam)); hi[i] = PMClImg{nullptr, e->vw(i), e->vh(i)};
		if (!e->views[i].set) continue;
		memcpy(hc[i].K, e->views[i].K, 72); memcpy(hc[i].R, e->views[i].R, 72); memcpy(hc[i].C, e->views[i].C, 24); pmfu_composeP(hc[i]);
		const bool has = !f.hasBgr.empty() && f.hasBgr[i];
		if (has) hi[i].bgr = e->views[i].sw ? e->views[i].oBgr : (f.bgr ? f.bgr + 3 * P0 * i : nullptr);
	}
	HIPCHK(e, hipMemcpyAsync(c.cams, hc.data(), sizeof(PMFuseCam) * N, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipMemcpyAsync(c.imgs, hi.data(), sizeof(PMClImg) * N, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));                       // hc / hi live on this frame
	return 0;
}

// the views the resident cloud's points list: used[i] != 0, counted on the device into buf (N + 1 entries); used[N] != 0: a point lists a view outside 0 .. N-1
static int viewsInUse(pmhip_engine* e, int N, uint32_t* buf, std::vector<uint32_t>& used) {
	auto& f = e->fu;
	HIPCHK(e, hipMemsetAsync(buf, 0, sizeof(uint32_t) * (N + 1), e->stream));
	hipLaunchKernelGGL(pmcl_mark_views, dim3((unsigned)std::min<uint64_t>((f.nViews + 255) / 256, 2048)), dim3(256), 0, e->stream, f.out.views, (uint32_t)f.nViews, (uint32_t)N, buf);
	used.resize((size_t)N + 1);
	HIPCHK(e, hipMemcpyAsync(used.data(), buf, sizeof(uint32_t) * (N + 1), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

// Counting sort of the resident cloud's n points by a key below nKeys.  `count(blocks)` launches the kernel that writes every point's key (c.cellOf) and the points per key
// (c.counts); afterwards c.cellStart[0 .. nKeys) is the scan of the counts and c.spts holds the points in key order.  endMark: cellStart[nKeys] = n as well.
template <class Count>
static int sortCloud(pmhip_engine* e, uint32_t n, uint32_t nKeys, bool endMark, Count count) {
	auto& c = e->cl; auto& f = e->fu;
	const size_t nSlots = (size_t)nKeys + (endMark ? 1 : 0);
	HIPCHK(e, c.counts.reserve(nSlots)); HIPCHK(e, c.cellStart.reserve(nSlots));
	int rc = ensureCloudPoints(e, n); if (rc) return rc;                // (the sorted copy, and tiles for the scan)
	HIPCHK(e, hipMemsetAsync(c.counts, 0, sizeof(uint32_t) * nKeys, e->stream));
	HIPCHK(e, hipMemsetAsync(c.misc, 0, sizeof(uint32_t) * 4, e->stream));
	const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
	count(nb);
	const unsigned nT = (nKeys + PMCL_TILE - 1) / PMCL_TILE;
	hipLaunchKernelGGL(pmcl_tile_sums_u32, dim3(nT), dim3(PMCL_TB), 0, e->stream, c.counts, nKeys, c.tileSums);
	hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, c.tileSums, nT, c.misc, c.tileOff);
	hipLaunchKernelGGL(pmcl_scan_apply, dim3(nT), dim3(PMCL_TB), 0, e->stream, c.counts, nKeys, c.tileOff, c.cellStart);
	if (endMark) HIPCHK(e, hipMemcpyAsync(c.cellStart + nKeys, &n, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(pmcl_scatter_kernel, dim3(nb), dim3(256), 0, e->stream, f.out.points, n, c.cellOf, c.counts, c.spts);
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipStreamSynchronize(e->stream));                       // (n lives on this frame)
	return 0;
}

static float orderedToFloat(uint32_t u) { const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u; float f; memcpy(&f, &b, 4); return f; }

// the grid over the resident cloud, its points counting-sorted by cell.  Cell edge: the k-th neighbour distance of a sample of the cloud (median),
// scaled to the whole cloud's density as for a surface; no finer than 1/4096 of the largest extent, and no more cells than twice the points (2^26 at most)
static int buildGrid(pmhip_engine* e, int k, PMClGrid& g) {
	auto& c = e->cl; auto& f = e->fu;
	const uint32_t n = (uint32_t)f.nPoints;
	int rc = ensureCloudPoints(e, n); if (rc) return rc;
	const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
	HIPCHK(e, hipMemsetAsync(c.misc + 8, 0xFF, sizeof(uint32_t) * 3, e->stream));
	HIPCHK(e, hipMemsetAsync(c.misc + 11, 0, sizeof(uint32_t) * 3, e->stream));
	hipLaunchKernelGGL(pmcl_bbox_kernel, dim3(nb), dim3(256), 0, e->stream, f.out.points, n, c.misc + 8);
	const uint32_t S = std::min<uint32_t>(n, 1024);
	hipLaunchKernelGGL(pmcl_sample_kernel, dim3((S + 255) / 256), dim3(256), 0, e->stream, f.out.points, n, S, c.sample);
	uint32_t bb[6]; std::vector<float> hs((size_t)S * 3);
	HIPCHK(e, hipMemcpyAsync(bb, c.misc + 8, sizeof(bb), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipMemcpyAsync(hs.data(), c.sample, sizeof(float) * 3 * S, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	double lo[3], ext[3], L = 0;
	for (int a = 0; a < 3; ++a) { lo[a] = (double)orderedToFloat(bb[a]); ext[a] = (double)orderedToFloat(bb[3 + a]) - lo[a]; L = std::max(L, ext[a]); }
	if (!(L < 1e300)) { e->err = "cloud: points are not finite"; return PMHIP_E_ARG; }
	double h = L > 0 ? L / 4096. : 1.;
	const uint32_t j = std::min<uint32_t>((uint32_t)k, S > 1 ? S - 1 : 1);
	if (S > 1) {
		std::vector<double> rk(S), d2(S);
		for (uint32_t a = 0; a < S; ++a) {
			for (uint32_t b = 0; b < S; ++b) {
				const double dx = (double)hs[a*3] - hs[b*3], dy = (double)hs[a*3+1] - hs[b*3+1], dz = (double)hs[a*3+2] - hs[b*3+2];
				d2[b] = dx * dx + dy * dy + dz * dz;
			}
			std::nth_element(d2.begin(), d2.begin() + j, d2.end());      // d2[0] is the point itself
			rk[a] = d2[j];
		}
		std::nth_element(rk.begin(), rk.begin() + S / 2, rk.end());
		const double r = sqrt(rk[S / 2]) * sqrt((double)k * S / ((double)j * n));
		h = std::max(h, r);
	}
	const double maxCells = (double)std::min<size_t>(std::max<size_t>((size_t)2 * n, 4096), (size_t)1 << 26);
	int dims[3];
	for (;;) {
		double cells = 1;
		for (int a = 0; a < 3; ++a) { dims[a] = (int)std::min(floor(ext[a] / h) + 1., 1e9); cells *= dims[a]; }
		if (cells <= maxCells) break;
		h *= 1.25;
	}
	const uint32_t nCells = (uint32_t)dims[0] * dims[1] * dims[2];
	g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2]; g.h = h; g.invh = 1. / h; g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
	return sortCloud(e, n, nCells, true, [&](unsigned blocks) {
		g.cellStart = c.cellStart; g.spts = c.spts;
		hipLaunchKernelGGL(pmcl_count_kernel, dim3(blocks), dim3(256), 0, e->stream, f.out.points, n, g, c.cellOf, c.counts);
	});
}

static int launchKnn(pmhip_engine* e, bool pca, const PMClGrid& g, int k, uint32_t nq, const PMClKnnOut& o) {
	const dim3 gr((nq + 255) / 256), bl(256);
	const float* pts = e->fu.out.points;
	if (k <= 16) { if (pca) hipLaunchKernelGGL((pmcl_knn_kernel<16, true>), gr, bl, 0, e->stream, g, pts, k, nq, o); else hipLaunchKernelGGL((pmcl_knn_kernel<16, false>), gr, bl, 0, e->stream, g, pts, k, nq, o); }
	else { if (pca) hipLaunchKernelGGL((pmcl_knn_kernel<32, true>), gr, bl, 0, e->stream, g, pts, k, nq, o); else hipLaunchKernelGGL((pmcl_knn_kernel<32, false>), gr, bl, 0, e->stream, g, pts, k, nq, o); }
	HIPCHK(e, hipGetLastError());
	return 0;
}

// The RFOREACH + RemovePoint loop of the reference (PointCloud.cpp:66-93) on the resident cloud, see pm_cloud.hip for the order.  The caller has called
// ensureCloudPoints, cleared misc[0..3] and launched the kernel that writes the hole flags (c.hole) and the holes per tile (c.tileSums) of the n points:
// pmcl_crop_flags for the ROI, pmclf_flags for the visibility filter and RemoveMinViews.
static int removeFlagged(pmhip_engine* e) {
	auto& c = e->cl; auto& f = e->fu;
	const uint32_t n = (uint32_t)f.nPoints;
	const unsigned nT = (n + PMCL_TILE - 1) / PMCL_TILE;
	hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, c.tileSums, nT, c.misc, c.tileOff);
	hipLaunchKernelGGL(pmcl_crop_next, dim3(nT), dim3(PMCL_TB), 0, e->stream, c.hole, n, c.tileOff, c.misc, c.nxt);
	uint32_t H = 0;
	HIPCHK(e, hipMemcpyAsync(&H, c.misc, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	if (H == 0) return 0;
	const uint32_t m = n - H;
	const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
	for (int round = 0; round < 64; ++round) {                          // chains only climb: at most log2(n) + 1 rounds
		uint32_t changed = 0;
		HIPCHK(e, hipMemsetAsync(c.misc + 4, 0, sizeof(uint32_t), e->stream));
		hipLaunchKernelGGL(pmcl_jump, dim3(nb), dim3(256), 0, e->stream, c.nxt, n, c.misc + 4);
		HIPCHK(e, hipMemcpyAsync(&changed, c.misc + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		if (!changed) break;
	}
	// the target buffers: as large as the current ones, colours / normals as the cloud has them
	HIPCHK(e, c.alt.reserve(f.out.cap, f.haveColor, f.haveNormal));
	const PMFuseOut in = f.out.view(f.haveColor, f.haveNormal), out = c.alt.view(f.haveColor, f.haveNormal);
	const unsigned mT = (m + PMCL_TILE - 1) / PMCL_TILE;
	HIPCHK(e, hipMemsetAsync(c.misc, 0, sizeof(uint32_t) * 4, e->stream));
	if (m) {
		hipLaunchKernelGGL(pmcl_crop_tile_sums, dim3(mT), dim3(PMCL_TB), 0, e->stream, c.nxt, f.out.viewStart, m, c.tileSums);
		hipLaunchKernelGGL(pmfu_scan_tiles, dim3(1), dim3(1024), 0, e->stream, c.tileSums, mT, c.misc, c.tileOff);
		hipLaunchKernelGGL(pmcl_crop_scatter, dim3(mT), dim3(PMCL_TB), 0, e->stream, in, c.nxt, m, c.tileOff, out);
	}
	uint32_t nv = 0;
	HIPCHK(e, hipMemcpyAsync(&nv, c.misc, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpyAsync(out.viewStart + m, &nv, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipStreamSynchronize(e->stream));
	std::swap(f.out, c.alt);
	f.nPoints = m; f.nViews = nv;
	return 0;
}

// PointCloud::RemovePointsOutside
static int cropCloud(pmhip_engine* e, const PMClObb& box) {
	auto& c = e->cl; auto& f = e->fu;
	const uint32_t n = (uint32_t)f.nPoints;
	int rc = ensureCloudPoints(e, n); if (rc) return rc;
	HIPCHK(e, hipMemsetAsync(c.misc, 0, sizeof(uint32_t) * 4, e->stream));
	hipLaunchKernelGGL(pmcl_crop_flags, dim3((n + PMCL_TILE - 1) / PMCL_TILE), dim3(PMCL_TB), 0, e->stream, f.out.points, n, box, c.hole, c.tileSums);
	return removeFlagged(e);
}

// hole flags from the votes (vis) or the view counts, then the removal
static int removeByFlags(pmhip_engine* e, const int* vis, int th, uint32_t nMin) {
	auto& c = e->cl; auto& f = e->fu;
	const uint32_t n = (uint32_t)f.nPoints;
	int rc = ensureCloudPoints(e, n); if (rc) return rc;
	HIPCHK(e, hipMemsetAsync(c.misc, 0, sizeof(uint32_t) * 4, e->stream));
	hipLaunchKernelGGL(pmclf_flags, dim3((n + PMCL_TILE - 1) / PMCL_TILE), dim3(PMCL_TB), 0, e->stream, vis, th, f.out.viewStart, nMin, n, c.hole, c.tileSums);
	return removeFlagged(e);
}

// the body of pmhip_scene_cloud_set / _load: a cloud from the host becomes the resident one (N: the views its points may list, `what`: the views' name in the messages)
static int loadCloud(pmhip_engine* e, const std::string& who, const char* what, int N, const float* points, const uint32_t* viewStart, const uint32_t* views, const float* weights,
                     const unsigned char* colors, const float* normals, uint64_t nPoints) {
	if (nPoints >= 0xFFFFFFFFull || viewStart[0] != 0) { e->err = who + ": bad sizes"; return PMHIP_E_ARG; }
	const uint64_t nV = viewStart[nPoints];
	for (uint64_t i = 0; i < nPoints; ++i) if (viewStart[i + 1] <= viewStart[i]) { e->err = who + ": every point needs a view"; return PMHIP_E_ARG; }
	for (uint64_t v = 0; v < nV; ++v) if (views[v] >= (uint32_t)N) { e->err = who + ": view index outside " + what; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	auto& f = e->fu;
	HIPCHK(e, f.out.reserve((size_t)std::max<uint64_t>(nPoints, nV) + 1, colors != nullptr, normals != nullptr));
	if (nPoints) {
		HIPCHK(e, hipMemcpyAsync(f.out.points, points, sizeof(float) * 3 * nPoints, hipMemcpyHostToDevice, e->stream));
		if (colors) HIPCHK(e, hipMemcpyAsync(f.out.colors, colors, 3 * nPoints, hipMemcpyHostToDevice, e->stream));
		if (normals) HIPCHK(e, hipMemcpyAsync(f.out.normals, normals, sizeof(float) * 3 * nPoints, hipMemcpyHostToDevice, e->stream));
	}
	HIPCHK(e, hipMemcpyAsync(f.out.viewStart, viewStart, sizeof(uint32_t) * (nPoints + 1), hipMemcpyHostToDevice, e->stream));
	if (nV) {
		HIPCHK(e, hipMemcpyAsync(f.out.views, views, sizeof(uint32_t) * nV, hipMemcpyHostToDevice, e->stream));
		if (weights) HIPCHK(e, hipMemcpyAsync(f.out.weights, weights, sizeof(float) * nV, hipMemcpyHostToDevice, e->stream));
		else HIPCHK(e, hipMemsetAsync(f.out.weights, 0, sizeof(float) * nV, e->stream));
		HIPCHK(e, hipMemsetAsync(f.out.projs, 0, sizeof(uint16_t) * 2 * nV, e->stream));
	}
	HIPCHK(e, hipStreamSynchronize(e->stream));
	f.nPoints = nPoints; f.nViews = nV; f.nDepths = 0; f.rounds = 0; f.haveColor = colors != nullptr; f.haveNormal = normals != nullptr; f.haveWeight = weights != nullptr;
	return 0;
}

extern "C" {

int pmhip_scene_cloud_set(pmhip_engine* e, const float* points, const uint32_t* viewStart, const uint32_t* views, const float* weights, uint64_t nPoints) {
	if (!e || !viewStart || (nPoints && (!points || !views))) return PMHIP_E_ARG;
	if (e->nImages < 1) { e->err = "cloud_set: no scene"; return PMHIP_E_STATE; }
	return loadCloud(e, "cloud_set", "the scene", e->nImages, points, viewStart, views, weights, nullptr, nullptr, nPoints);
}

int pmhip_scene_cloud_knn(pmhip_engine* e, int nNeighbors, const uint32_t* queries, uint32_t nQueries, uint32_t* out) {
	if (!e || nNeighbors < 1 || nNeighbors > 32 || (nQueries && (!queries || !out))) return PMHIP_E_ARG;
	auto& f = e->fu; auto& c = e->cl;
	if (!f.out.points || !f.nPoints) { e->err = "cloud_knn: no cloud"; return PMHIP_E_STATE; }
	for (uint32_t i = 0; i < nQueries; ++i) if (queries[i] >= f.nPoints) { e->err = "cloud_knn: query outside the cloud"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	const int k = (int)std::min<uint64_t>((uint64_t)nNeighbors, f.nPoints);
	PMClGrid g; int rc = buildGrid(e, k, g); if (rc) return rc;
	if (!nQueries) return 0;
	HIPCHK(e, c.qbuf.reserve(nQueries)); HIPCHK(e, c.obuf.reserve((size_t)nQueries * k));
	HIPCHK(e, hipMemcpyAsync(c.qbuf, queries, sizeof(uint32_t) * nQueries, hipMemcpyHostToDevice, e->stream));
	PMClKnnOut o; memset(&o, 0, sizeof(o)); o.queries = c.qbuf; o.idx = c.obuf;
	rc = launchKnn(e, false, g, k, nQueries, o); if (rc) return rc;
	std::vector<uint32_t> tmp((size_t)nQueries * k);
	HIPCHK(e, hipMemcpyAsync(tmp.data(), c.obuf, sizeof(uint32_t) * tmp.size(), hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	for (uint32_t q = 0; q < nQueries; ++q)
		for (int j = 0; j < nNeighbors; ++j) out[(size_t)q * nNeighbors + j] = j < k ? tmp[(size_t)q * k + j] : PMCL_NONE;
	return 0;
}

int pmhip_scene_cloud_finish(pmhip_engine* e, const PMHipCloudParams* p, uint64_t* nPoints, uint64_t* nViews) {
	if (!e || !p) return PMHIP_E_ARG;
	auto& f = e->fu; auto& c = e->cl;
	if (!f.out.points) { e->err = "cloud_finish: no cloud (pmhip_scene_fuse or pmhip_scene_cloud_set first)"; return PMHIP_E_STATE; }
	if (p->bEstimateNormal && (p->nNeighbors < 1 || p->nNeighbors > 32)) { e->err = "cloud_finish: nNeighbors must be 1..32"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	for (double& t : c.ms) t = 0;
	using clk = std::chrono::steady_clock;
	auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
	int rc = 0;
	if (p->bCrop && f.nPoints) {                                       // (the reference skips the whole block for an empty cloud)
		const auto t0 = clk::now();
		PMClObb box; memcpy(box.rot, p->obbRot, sizeof(box.rot)); memcpy(box.pos, p->obbPos, sizeof(box.pos));
		for (int a = 0; a < 3; ++a) box.ext[a] = p->fBorderROI == 0 ? p->obbExt[a] : p->fBorderROI > 0 ? p->obbExt[a] * p->fBorderROI : p->obbExt[a] + (-p->fBorderROI);
		rc = cropCloud(e, box); if (rc) return rc;
		c.ms[0] = ms(t0);
	}
	const bool wantColor = p->bEstimateColor && !f.haveColor && f.nPoints, wantNormal = p->bEstimateNormal && !f.haveNormal && f.nPoints;
	if (wantColor || wantNormal) { rc = uploadCloudViews(e); if (rc) return rc; }
	const uint32_t n = (uint32_t)f.nPoints;
	if (wantColor) {
		const auto t0 = clk::now();
		// every view a point lists must have its colour image (the reference loads them all; a view without one here is a caller error)
		const int N = e->nImages;
		std::vector<uint32_t> used;
		rc = viewsInUse(e, N, c.used, used); if (rc) return rc;
		if (used[(size_t)N]) { e->err = "cloud_finish: a point lists a view outside the scene"; return PMHIP_E_STATE; }
		for (int i = 0; i < N; ++i)
			if (used[(size_t)i] && (f.hasBgr.empty() || !f.hasBgr[(size_t)i] || !(e->views[i].sw ? (const void*)e->views[i].oBgr : (const void*)f.bgr))) {
				e->err = "cloud_finish: bEstimateColor needs pmhip_scene_set_color for every view the points list"; return PMHIP_E_STATE; }
		HIPCHK(e, f.out.reserve(f.out.cap, true, false));
		hipLaunchKernelGGL(pmcl_color_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, f.out.view(), n, c.cams, c.imgs);
		HIPCHK(e, hipGetLastError());
		HIPCHK(e, hipStreamSynchronize(e->stream));
		f.haveColor = true;
		c.ms[3] = ms(t0);
	}
	if (wantNormal) {
		auto t0 = clk::now();
		const int k = (int)std::min<uint64_t>((uint64_t)p->nNeighbors, f.nPoints);
		PMClGrid g; rc = buildGrid(e, k, g); if (rc) return rc;
		c.ms[1] = ms(t0);
		t0 = clk::now();
		HIPCHK(e, f.out.reserve(f.out.cap, false, true));
		PMClKnnOut o; memset(&o, 0, sizeof(o));
		o.normals = f.out.normals; o.viewStart = f.out.viewStart; o.views = f.out.views; o.cams = c.cams;
		rc = launchKnn(e, true, g, k, n, o); if (rc) return rc;
		HIPCHK(e, hipStreamSynchronize(e->stream));
		f.haveNormal = true;
		c.ms[2] = ms(t0);
	}
	if (nPoints) *nPoints = f.nPoints;
	if (nViews) *nViews = f.nViews;
	return 0;
}

int pmhip_scene_cloud_times(pmhip_engine* e, double ms[4]) {
	if (!e || !ms) return PMHIP_E_ARG;
	for (int i = 0; i < 4; ++i) ms[i] = e->cl.ms[i];
	return 0;
}


// ---- Scene::PointCloudFilter / PointCloud::RemoveMinViews on the resident cloud (pm_cloud_filter.hip) ------------------------------------
int pmhip_scene_cloud_load(pmhip_engine* e, const float* points, const uint32_t* viewStart, const uint32_t* views, const float* weights, const unsigned char* colors, const float* normals,
                           uint64_t nPoints, int32_t nCams) {
	if (!e || !viewStart || nCams < 0 || (nPoints && (!points || !views))) return PMHIP_E_ARG;
	const int N = nCams > 0 ? nCams : e->nImages;
	if (N < 1) { e->err = "cloud_load: no scene and no camera count"; return PMHIP_E_STATE; }
	return loadCloud(e, "cloud_load", "the cameras", N, points, viewStart, views, weights, colors, normals, nPoints);
}

int pmhip_scene_cloud_filter(pmhip_engine* e, const PMHipCloudFilterParams* p, uint64_t* nPoints, uint64_t* nViews) {
	if (!e || !p) return PMHIP_E_ARG;
	auto& f = e->fu; auto& c = e->cl;
	if (!f.out.points) { e->err = "cloud_filter: no cloud (pmhip_scene_fuse, pmhip_scene_cloud_set or pmhip_scene_cloud_load first)"; return PMHIP_E_STATE; }
	if ((p->camC != nullptr) != (p->camAngle != nullptr) || (p->camC && p->nCams < 1)) { e->err = "cloud_filter: camC and camAngle go together, with nCams > 0"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	for (double& t : c.fms) t = 0;
	c.visN = 0; c.cones.clear(); c.fcount[0] = c.fcount[1] = 0;
	using clk = std::chrono::steady_clock;
	auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
	int rc = 0;
	if (p->nMinViews > 0 && f.nPoints) {                               // PointCloud::RemoveMinViews
		const auto t0 = clk::now();
		rc = removeByFlags(e, nullptr, 0, p->nMinViews); if (rc) return rc;
		c.fms[2] += ms(t0);
	}
	if (p->bVisibility && f.nPoints) {
		const int N = p->camC ? p->nCams : e->nImages;
		if (N < 1) { e->err = "cloud_filter: no scene and no cameras"; return PMHIP_E_STATE; }
		const uint32_t n = (uint32_t)f.nPoints;
		// the views in use; a point that lists a view outside the cameras is a caller error
		HIPCHK(e, c.fused.reserve((size_t)N + 1));
		std::vector<uint32_t> used;
		rc = viewsInUse(e, N, c.fused, used); if (rc) return rc;
		if (used[(size_t)N]) { e->err = "cloud_filter: a point lists a view outside the cameras"; return PMHIP_E_STATE; }
		// the cones: origin Cast<float>(C), angle = float(ComputeFOV(0) / width), cosAngleSq = SQUARE(cosf(angle)) -- on the host, once per view
		std::vector<PMClfView> V((size_t)N);
		c.cones.assign((size_t)N * 2, 0.f);
		for (int i = 0; i < N; ++i) {
			memset(&V[i], 0, sizeof(PMClfView));
			const double* C; float angle;
			if (p->camC) { C = p->camC + 3 * i; angle = p->camAngle[i]; }
			else {
				if (!e->views[i].set) { if (used[(size_t)i]) { e->err = "cloud_filter: a point lists a view that is not set"; return PMHIP_E_STATE; } continue; }
				C = e->views[i].C;
				const double w = (double)e->vw(i);
				angle = (float)(2. * atan(w / (2. * e->views[i].K[0])) / w);
			}
			const float cs = cosf(angle);
			V[i].ox = (float)C[0]; V[i].oy = (float)C[1]; V[i].oz = (float)C[2]; V[i].cosSq = cs * cs; V[i].view = (uint32_t)i;
			pmclf_plan(V[i].cosSq, V[i]);
			c.cones[(size_t)i * 2] = angle; c.cones[(size_t)i * 2 + 1] = V[i].cosSq;
		}
		HIPCHK(e, c.vis.reserve(n));
		HIPCHK(e, hipMemsetAsync(c.vis, 0, sizeof(int) * (size_t)n, e->stream));
		if (!c.fstats) HIPCHK(e, c.fstats.alloc(2));
		HIPCHK(e, hipMemsetAsync(c.fstats, 0, sizeof(unsigned long long) * 2, e->stream));
		for (int i = 0; i < N; ++i) {
			if (!used[(size_t)i]) continue;                                  // views that no point lists are skipped
			auto t0 = clk::now();
			const uint32_t nBins = 6u * (uint32_t)V[i].R * (uint32_t)V[i].R;   // (sorted with one more bin, empty: binStart[nBins] = n)
			rc = sortCloud(e, n, nBins + 1, false, [&](unsigned blocks) {
				hipLaunchKernelGGL(pmclf_count_kernel, dim3(blocks), dim3(256), 0, e->stream, f.out.points, n, V[i], c.cellOf, c.counts);
			}); if (rc) return rc;
			c.fms[0] += ms(t0);
			t0 = clk::now();
			hipLaunchKernelGGL(pmclf_cone_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, V[i], c.spts, c.cellStart, n, f.out.viewStart, f.out.views, c.vis, c.fstats);
			HIPCHK(e, hipGetLastError());
			HIPCHK(e, hipStreamSynchronize(e->stream));
			c.fms[1] += ms(t0);
		}
		c.visN = n;
		unsigned long long st[2] = {0, 0};
		HIPCHK(e, hipMemcpyAsync(st, c.fstats, sizeof(st), hipMemcpyDeviceToHost, e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		c.fcount[0] = st[0]; c.fcount[1] = st[1];
		const auto t0 = clk::now();
		rc = removeByFlags(e, c.vis, p->thRemove, 0u); if (rc) return rc;
		c.fms[2] += ms(t0);
	}
	if (nPoints) *nPoints = f.nPoints;
	if (nViews) *nViews = f.nViews;
	return 0;
}

int pmhip_scene_cloud_visibility(pmhip_engine* e, int32_t* out, uint64_t n) {
	if (!e || (n && !out)) return PMHIP_E_ARG;
	if (n != e->cl.visN) { e->err = "cloud_visibility: n is not the size of the cloud the last filter voted on"; return PMHIP_E_ARG; }
	if (!n) return 0;
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipMemcpyAsync(out, e->cl.vis, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int pmhip_scene_cloud_filter_cones(pmhip_engine* e, float* out) {
	if (!e || !out) return PMHIP_E_ARG;
	if (e->cl.cones.empty()) { e->err = "cloud_filter_cones: no visibility filter has run"; return PMHIP_E_STATE; }
	memcpy(out, e->cl.cones.data(), sizeof(float) * e->cl.cones.size());
	return 0;
}

int pmhip_scene_cloud_filter_counts(pmhip_engine* e, uint64_t out[2]) {
	if (!e || !out) return PMHIP_E_ARG;
	out[0] = e->cl.fcount[0]; out[1] = e->cl.fcount[1];
	return 0;
}

int pmhip_scene_cloud_filter_times(pmhip_engine* e, double ms[3]) {
	if (!e || !ms) return PMHIP_E_ARG;
	for (int i = 0; i < 3; ++i) ms[i] = e->cl.fms[i];
	return 0;
}

} // extern "C"
