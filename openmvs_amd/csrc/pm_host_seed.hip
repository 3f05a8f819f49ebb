// pm_host_seed.hip -- the seed rasteriser behind libpmhip.so (kernels and the launch sequence: seed_raster.hip; C ABI: include/pmhip_seed.h).  Part of the translation
// unit pm_engine.hip.

// check, upload, rasterise into (dDepth, dNormal), synchronise, collect the statistics
static int seedInto(pmhip_engine* e, int mode, int w, int h, const float* proj, const float* z, const float* normals, uint32_t nVerts, const uint32_t* faces,
		uint32_t nFaces, float* dDepth, float* dNormal) {
	HIPCHK(e, seedRun(e->seed, e->stream, mode, w, h, proj, z, normals, nVerts, faces, nFaces, dDepth, dNormal));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, seedCollect(e->seed, mode, nVerts == 0 || (mode == SEED_MODE_FACES && nFaces == 0)));
	return 0;
}

extern "C" {

int pmhip_seed_raster(pmhip_engine* e, int mode, int w, int h, const float* proj, const float* z, const float* normals, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces,
		float* depthOut, float* normalOut) {
	if (!e) return PMHIP_E_ARG;
	const std::string why = seedCheck("pmhip_seed_raster", mode, w, h, proj, z, nVerts, faces, nFaces);
	if (!why.empty()) { e->err = why; return PMHIP_E_ARG; }
	if (!depthOut) { e->err = "pmhip_seed_raster: no depth map to write"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P = (size_t)w * h;
	const bool wantNormal = normals && normalOut;
	HIPCHK(e, e->seedDepth.reserve(P));
	if (wantNormal) HIPCHK(e, e->seedNormal.reserve(3 * P));
	const int rc = seedInto(e, mode, w, h, proj, z, wantNormal ? normals : nullptr, nVerts, faces, nFaces, e->seedDepth, wantNormal ? e->seedNormal.p : nullptr);
	if (rc) return rc;
	HIPCHK(e, hipMemcpy(depthOut, e->seedDepth, sizeof(float) * P, hipMemcpyDeviceToHost));
	if (wantNormal) HIPCHK(e, hipMemcpy(normalOut, e->seedNormal, sizeof(float) * 3 * P, hipMemcpyDeviceToHost));
	return 0;
}

int pmhip_scene_seed_view(pmhip_engine* e, int view, int mode, const float* proj, const float* z, const float* normals, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces) {
	if (!e) return PMHIP_E_ARG;
	if (view < 0 || view >= e->nImages) { e->err = "pmhip_scene_seed_view: view " + std::to_string(view) + " of " + std::to_string(e->nImages); return PMHIP_E_ARG; }
	const int w = e->vw(view), h = e->vh(view);
	const std::string why = seedCheck("pmhip_scene_seed_view", mode, w, h, proj, z, nVerts, faces, nFaces);
	if (!why.empty()) { e->err = why; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	const int rc = seedInto(e, mode, w, h, proj, z, normals, nVerts, faces, nFaces, e->depthOf(view), normals ? e->normalOf(view) : nullptr);
	if (rc) return rc;
	e->views[view].hasMaps = true;                                          // as pmhip_scene_set_maps with a depth map
	return 0;
}

int pmhip_seed_set_tuning(pmhip_engine* e, int boxPixels) {
	if (!e) return PMHIP_E_ARG;
	if (boxPixels) e->seed.boxMax = boxPixels < 0 ? SEED_BOX_PIXELS : boxPixels;
	return 0;
}

int pmhip_seed_get_stats(pmhip_engine* e, uint64_t out[4]) {
	if (!e || !out) return PMHIP_E_ARG;
	out[0] = e->seed.statLarge; out[1] = (uint64_t)e->seed.boxMax; out[2] = e->seed.statUs; out[3] = e->seed.statBytes;
	return 0;
}

} // extern "C"
