// pm_host_filter.hip -- host side of the depth-map filters (kernels: pm_filter.hip).  Part of the translation unit pm_engine.hip.
extern "C" {

// DepthMapsData::FilterDepthMap for each view of viewIds against its first <= 8 neighbours (Scene::DenseReconstructionFilter,
// SceneDensify.cpp:2136-2170).  Results are staged; pmhip_scene_filter_commit installs them once every view has been
// filtered against the *unfiltered* maps of its neighbours (EVT_ADJUSTDEPTHMAP is processed after all filter events, :2183-2210).
int pmhip_scene_filter(pmhip_engine* e, const int32_t* viewIds, int nViews, int bAdjust, uint32_t nMinViewsFilter,
		uint32_t nMinViewsFilterAdjust, float fDepthDiffThreshold, int sync) {
	if (!e || !viewIds || nViews <= 0 || e->nImages < 2) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = (size_t)e->w * e->h;
	if (!e->d_fdepth) {
		HIPCHK(e, e->d_fdepth.alloc(P0 * e->nImages));
		HIPCHK(e, e->d_fconf.alloc(P0 * e->nImages));
		HIPCHK(e, e->d_fvalid.alloc(e->nImages));
		HIPCHK(e, hipMemsetAsync(e->d_fvalid, 0, e->nImages, e->stream));
	}
	// every view is filtered at its own size (the reference sizes each depth map on its own image): the splat buffer holds the largest reference view of the call,
	// a view with its own size stages its result in its own buffers
	size_t Pref = 0, Pany = 0;
	for (int b = 0; b < nViews; ++b) {
		const int id = viewIds[b];
		if (id < 0 || id >= e->nImages || !e->views[id].set) { e->err = "view not set"; return PMHIP_E_ARG; }
		Pref = std::max(Pref, e->vpix(id)); Pany = std::max(Pany, e->vpix(id));
		SceneView& v = e->views[id];
		for (int k = 0; k < v.nNb; ++k) if (v.nb[k] >= 0 && v.nb[k] < e->nImages) Pany = std::max(Pany, e->vpix(v.nb[k]));
		if (v.sw && !v.oFDepth) { HIPCHK(e, v.oFDepth.alloc(e->vpix(id))); HIPCHK(e, v.oFConf.alloc(e->vpix(id))); }
	}
	const int CH = std::min(nViews, 4); // reference views per launch: bounds the splat buffer (8 x 8 B per pixel per view)
	if (e->splatCap < CH || e->splatPix < Pref) {
		HIPCHK(e, hipStreamSynchronize(e->stream));
		e->d_splat.release(); e->d_ftasks.release(); e->h_ftasks.release();
		const int cap = std::max(CH, e->splatCap); const size_t pix = std::max(Pref, e->splatPix);
		HIPCHK(e, e->d_splat.alloc(pix * PMF_MAXN * cap));
		HIPCHK(e, e->d_ftasks.alloc(cap));
		HIPCHK(e, e->h_ftasks.alloc(cap));
		e->splatCap = cap; e->splatPix = pix;
	}
	const unsigned nCal = (unsigned)e->nImages;
	const unsigned nMinViews = std::min(nMinViewsFilter, nCal - 1), nMinViewsAdjust = std::min(nMinViewsFilterAdjust, nCal - 1);
	std::vector<unsigned char> hv(e->nImages, 2); // 2 = untouched
	for (int b0 = 0; b0 < nViews; b0 += CH) {
		const int nb = std::min(CH, nViews - b0);
		HIPCHK(e, hipStreamSynchronize(e->stream)); // staging reuse
		for (int b = 0; b < nb; ++b) {
			const int id = viewIds[b0 + b];
			const SceneView& v = e->views[id];
			PMFTask& t = e->h_ftasks[b];
			memset(&t, 0, sizeof(t));
			memcpy(t.ref.K, v.K, 72); memcpy(t.ref.R, v.R, 72); memcpy(t.ref.C, v.C, 24);
			t.refDepth = e->depthOf(id); t.refConf = e->confOf(id);
			t.N = 0;
			for (int k = 0; k < v.nNb && t.N < PMF_MAXN; ++k) {
				const int j = v.nb[k];
				// neighbours without a depth map are skipped before the eight slots are filled (SceneDensify.cpp:2150-2163: !depthData.IsValid())
				if (j < 0 || j >= e->nImages || !e->views[j].set || !e->views[j].hasMaps) continue;
				const SceneView& sv = e->views[j];
				memcpy(t.nb[t.N].K, sv.K, 72); memcpy(t.nb[t.N].R, sv.R, 72); memcpy(t.nb[t.N].C, sv.C, 24);
				t.nbDepth[t.N] = e->depthOf(j); t.nbConf[t.N] = e->confOf(j); t.nbw[t.N] = e->vw(j); t.nbh[t.N] = e->vh(j);
				++t.N;
			}
			t.splat = e->d_splat + e->splatPix * PMF_MAXN * b;
			t.outDepth = v.sw ? v.oFDepth : e->d_fdepth + P0 * id; t.outConf = v.sw ? v.oFConf : e->d_fconf + P0 * id;
			t.w = e->vw(id); t.h = e->vh(id); t.dMin = v.dMin; t.dMax = v.dMax;
			t.filterable = !((unsigned)t.N < nMinViews || (unsigned)t.N < nMinViewsAdjust); // :1060-1063
			hv[id] = t.filterable ? 1 : 0;
		}
		HIPCHK(e, hipMemcpyAsync(e->d_ftasks, e->h_ftasks, sizeof(PMFTask) * nb, hipMemcpyHostToDevice, e->stream));
		const size_t nS = e->splatPix * PMF_MAXN * nb;
		hipLaunchKernelGGL(pmf_clear_kernel, dim3((unsigned)std::min<size_t>((nS + 255) / 256, 65535)), dim3(256), 0, e->stream, e->d_splat, nS);
		const unsigned gx = (unsigned)std::min<size_t>((Pany + 255) / 256, 2048);
		hipLaunchKernelGGL(pmf_splat_kernel, dim3(gx, nb, PMF_MAXN), dim3(256), 0, e->stream, e->d_ftasks);
		hipLaunchKernelGGL(pmf_vote_kernel, dim3(gx, nb), dim3(256), 0, e->stream, e->d_ftasks, bAdjust, nMinViews, nMinViewsAdjust, fDepthDiffThreshold);
		HIPCHK(e, hipGetLastError());
	}
	HIPCHK(e, hipStreamSynchronize(e->stream));
	for (int i = 0; i < e->nImages; ++i) if (hv[i] != 2) HIPCHK(e, hipMemcpyAsync(e->d_fvalid + i, &hv[i], 1, hipMemcpyHostToDevice, e->stream));
	// hv lives on this stack frame: the small copies above must have left it whatever the caller asked for; `sync` only says whether the caller
	// wants the filter kernels themselves finished on return (they are, as a consequence) -- kept in the ABI for symmetry with pmhip_scene_estimate
	HIPCHK(e, hipStreamSynchronize(e->stream));
	(void)sync;
	return 0;
}

// DepthMapsData::GapInterpolation (SceneDensify.cpp:904-1045) on the maps of these views, in place (row pass, then column pass).
int pmhip_scene_gap_interpolation(pmhip_engine* e, const int32_t* viewIds, int nViews, uint32_t nIpolGapSize, float fDepthDiffThreshold) {
	if (!e || !viewIds || nViews <= 0) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	size_t Pmax = 0;
	for (int b = 0; b < nViews; ++b) { if (viewIds[b] < 0 || viewIds[b] >= e->nImages) return PMHIP_E_ARG; Pmax = std::max(Pmax, e->vpix(viewIds[b])); }
	DevBuf<float> tmp; DevBuf<PMGTask> dt;
	HIPCHK(e, tmp.alloc(Pmax * 5));
	HIPCHK(e, dt.alloc(2));
	const float th = fDepthDiffThreshold * 2.5f;
	int rc = 0;
	for (int b = 0; b < nViews && rc == 0; ++b) {
		const int id = viewIds[b];
		const size_t P0 = e->vpix(id); const int vw = e->vw(id), vh = e->vh(id);
		const unsigned gx = (unsigned)std::min<size_t>((P0 + 255) / 256, 4096);
		float* D = e->depthOf(id); float* N = e->normalOf(id); float* Cf = e->confOf(id);
		PMGTask ht[2] = {{D, N, Cf, tmp, tmp + P0, tmp + P0 * 4, vw, vh}, {tmp, tmp + P0, tmp + P0 * 4, D, N, Cf, vw, vh}};
		if (hipMemcpyAsync(dt, ht, sizeof(ht), hipMemcpyHostToDevice, e->stream) != hipSuccess) { rc = PMHIP_E_HIP; break; }
		hipLaunchKernelGGL(pmf_gap_kernel, dim3(gx, 1), dim3(256), 0, e->stream, dt, 1, nIpolGapSize, th);       // 1. row-wise
		hipLaunchKernelGGL(pmf_gap_kernel, dim3(gx, 1), dim3(256), 0, e->stream, dt + 1, 0, nIpolGapSize, th);   // 2. column-wise
		if (hipStreamSynchronize(e->stream) != hipSuccess) { rc = PMHIP_E_HIP; break; }
	}
	if (rc == PMHIP_E_HIP) e->err = "gap interpolation: HIP error";
	return rc;
}

// DepthMapsData::RemoveSmallSegments (SceneDensify.cpp:809-900) on the maps of these views, in place; see pm_filter.hip.
int pmhip_scene_remove_small_segments(pmhip_engine* e, const int32_t* viewIds, int nViews, uint32_t nSpeckleSize, float fDepthDiffThreshold) {
	if (!e || !viewIds || nViews <= 0) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	int nmax = 0, cap = 0;
	for (int b = 0; b < nViews; ++b) {
		if (viewIds[b] < 0 || viewIds[b] >= e->nImages) return PMHIP_E_ARG;
		const int vw = e->vw(viewIds[b]), vh = e->vh(viewIds[b]);
		nmax = std::max(nmax, (int)e->vpix(viewIds[b])); cap = std::max(cap, (int)std::min<long long>(2LL * vw * vh - vw - vh, INT_MAX / 2));   // (2 * ne is an int below)
	}
	// A 4-connected w x h map has 2wh - w - h neighbouring pairs and each is one-directional in at most one direction, so the edge list of the largest view
	// cannot outgrow `cap` pairs (a geometric ramp with a ratio at the threshold fills it: every pair is asymmetric and every pixel its own component).
	// `ovr` first receives the sizes of the 2 * ne edge ends, then one (root, value) pair for each of the <= min(2 * ne, n) components the edges touch.
	const size_t nOvr = 2 * (size_t)std::max(std::max(cap, nmax), 1);
	DevBuf<int> parent, size, edges, nEdges, ovr;
	HIPCHK(e, parent.alloc(nmax)); HIPCHK(e, size.alloc(nmax));
	HIPCHK(e, edges.alloc(2 * (size_t)std::max(cap, 1))); HIPCHK(e, nEdges.alloc(1)); HIPCHK(e, ovr.alloc(nOvr));
	const float th = fDepthDiffThreshold * 0.7f;
	int rc = 0;
	std::vector<int> hedges, hsize;
	for (int b = 0; b < nViews && rc == 0; ++b) {
		const int id = viewIds[b];
		const int n = (int)e->vpix(id), vw = e->vw(id), vh = e->vh(id);
		const unsigned gx = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 4096);
		float* D = e->depthOf(id); float* N = e->normalOf(id); float* Cf = e->confOf(id);
		hipMemsetAsync(nEdges, 0, sizeof(int), e->stream);
		hipLaunchKernelGGL(pmf_cc_init_kernel, dim3(gx), dim3(256), 0, e->stream, parent, size, n);
		hipLaunchKernelGGL(pmf_cc_hook_kernel, dim3(gx), dim3(256), 0, e->stream, D, parent, vw, vh, th);
		hipLaunchKernelGGL(pmf_cc_flatten_kernel, dim3(gx), dim3(256), 0, e->stream, parent, size, n);
		hipLaunchKernelGGL(pmf_cc_asym_kernel, dim3(gx), dim3(256), 0, e->stream, D, parent, vw, vh, th, edges, nEdges, cap);
		int ne = 0;
		if (hipMemcpyAsync(&ne, nEdges, sizeof(int), hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) { rc = PMHIP_E_HIP; break; }
		if (ne > cap) { e->err = "remove_small_segments: asymmetric edge list overflow"; rc = PMHIP_E_HIP; break; }   // a guard: unreachable by the bound above
		if (ne > 0) {
			// replay the reference's seed order on the quotient graph of components linked by one-directional edges
			hedges.resize(2 * (size_t)ne); hsize.resize(2 * (size_t)ne);
			hipLaunchKernelGGL(pmf_cc_gather_kernel, dim3((2 * ne + 255) / 256), dim3(256), 0, e->stream, size, edges, ovr, 2 * ne);   // (a 4K view: 2*ne ints instead of 33 MB)
			if (hipMemcpyAsync(hedges.data(), edges, sizeof(int) * 2 * ne, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
				hipMemcpyAsync(hsize.data(), ovr, sizeof(int) * 2 * ne, hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) { rc = PMHIP_E_HIP; break; }
			std::map<int, int> csize;                   // component root -> size
			for (int k = 0; k < 2 * ne; ++k) csize[hedges[k]] = hsize[k];
			std::map<int, std::set<int>> adj;
			for (int k = 0; k < ne; ++k) { adj[hedges[2 * k]].insert(hedges[2 * k + 1]); adj[hedges[2 * k + 1]]; }
			std::set<int> done;
			std::vector<int> pairs;
			for (auto& kv : adj) {                      // std::map iterates roots in increasing (= seed) order
				const int r = kv.first;
				if (done.count(r)) continue;
				std::vector<int> seg{r}; done.insert(r);
				for (size_t q = 0; q < seg.size(); ++q) for (int nb : adj[seg[q]]) if (!done.count(nb)) { done.insert(nb); seg.push_back(nb); }
				long total = 0; for (int x : seg) total += csize[x];
				const int val = total < (long)nSpeckleSize ? 0 : (int)nSpeckleSize;   // forces remove / keep for every member
				for (int x : seg) { pairs.push_back(x); pairs.push_back(val); }
			}
			const int np = (int)(pairs.size() / 2);
			if (hipMemcpy(ovr, pairs.data(), sizeof(int) * pairs.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = PMHIP_E_HIP; break; }
			hipLaunchKernelGGL(pmf_cc_override_kernel, dim3((np + 255) / 256), dim3(256), 0, e->stream, size, ovr, np);
		}
		hipLaunchKernelGGL(pmf_cc_apply_kernel, dim3(gx), dim3(256), 0, e->stream, D, N, Cf, parent, size, vw, vh, (int)nSpeckleSize);
		if (hipStreamSynchronize(e->stream) != hipSuccess) { rc = PMHIP_E_HIP; break; }
	}
	if (rc == PMHIP_E_HIP && e->err.empty()) e->err = "remove_small_segments: HIP error";
	return rc;
}

// install the staged filtered depth / confidence maps of the views filtered since the last commit (normal maps are
// left untouched, exactly like the reference: LoadDepthMap + LoadConfidenceMap only, SceneDensify.cpp:2190-2192)
int pmhip_scene_filter_commit(pmhip_engine* e) {
	if (!e || !e->d_fdepth) return PMHIP_E_STATE;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P0 = (size_t)e->w * e->h;
	std::vector<unsigned char> hv(e->nImages);
	HIPCHK(e, hipMemcpy(hv.data(), e->d_fvalid, e->nImages, hipMemcpyDeviceToHost));
	for (int i = 0; i < e->nImages; ++i) if (hv[i] == 1) {
		const SceneView& v = e->views[i];
		HIPCHK(e, hipMemcpyAsync(e->depthOf(i), v.sw ? v.oFDepth : e->d_fdepth + P0 * i, sizeof(float) * e->vpix(i), hipMemcpyDeviceToDevice, e->stream));
		HIPCHK(e, hipMemcpyAsync(e->confOf(i), v.sw ? v.oFConf : e->d_fconf + P0 * i, sizeof(float) * e->vpix(i), hipMemcpyDeviceToDevice, e->stream));
	}
	HIPCHK(e, hipMemsetAsync(e->d_fvalid, 0, e->nImages, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

} // extern "C"
