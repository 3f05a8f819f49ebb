// pm_host_normal.hip -- host side of the normal maps from depth (kernel: pm_normal.hip).  Part of the translation unit pm_engine.hip.

// n pixels in blocks of 256, at most PM_NORMAL_MAX_BLOCKS of them; the kernel strides (the resamplers' launch, pm_host_estimate.hip).  K's four entries are cast to
// float here as EstimateNormalMap reads them from a KMatrix cast to float.
#ifndef PM_NORMAL_MAX_BLOCKS
#define PM_NORMAL_MAX_BLOCKS 4096
#endif
static void launchNormalMap(hipStream_t st, const float* depth, float* normal, int w, int h, const double K[9]) {
	hipLaunchKernelGGL(pm_normal_map_kernel, dim3(resampleBlocks((size_t)w * h, PM_NORMAL_MAX_BLOCKS)), dim3(256), 0, st, depth, normal, w, h,
	                   (float)K[0], (float)K[4], (float)K[2], (float)K[5]);
}

extern "C" {

// EstimateNormalMap(K of the view, its resident depth map) into its resident normal map, for each listed view at its own size.  Every view is checked before the
// first launch: a refused call leaves the maps as they were.
int pmhip_scene_estimate_normals(pmhip_engine* e, const int32_t* viewIds, int nViews) {
	if (!e) return PMHIP_E_ARG;
	if (nViews < 0 || (nViews > 0 && !viewIds)) { e->err = "pmhip_scene_estimate_normals: no view list"; return PMHIP_E_ARG; }
	for (int b = 0; b < nViews; ++b) {
		const int id = viewIds[b];
		if (id < 0 || id >= e->nImages) { e->err = "pmhip_scene_estimate_normals: view " + std::to_string(id) + " is not a view of the scene"; return PMHIP_E_ARG; }
		if (!e->views[id].set) { e->err = "pmhip_scene_estimate_normals: view " + std::to_string(id) + " has no camera (pmhip_scene_set_view)"; return PMHIP_E_STATE; }
		if (!e->views[id].hasMaps) { e->err = "pmhip_scene_estimate_normals: view " + std::to_string(id) + " holds no depth map"; return PMHIP_E_STATE; }
	}
	if (nViews == 0) return 0;
	HIPCHK(e, hipSetDevice(e->device));
	for (int b = 0; b < nViews; ++b) {
		const int id = viewIds[b];
		launchNormalMap(e->stream, e->depthOf(id), e->normalOf(id), e->vw(id), e->vh(id), e->views[id].K);
	}
	HIPCHK(e, hipGetLastError());
	return 0;
}

// EstimateNormalMap on host buffers: depth w*h floats in, normal w*h*3 floats out.  Blocking; needs no scene and leaves a loaded one alone.
int pmhip_estimate_normal_map(pmhip_engine* e, const double K[9], const float* depth, int w, int h, float* normal) {
	if (!e) return PMHIP_E_ARG;
	if (!K || !depth || !normal || w <= 0 || h <= 0) { e->err = "pmhip_estimate_normal_map: K, depth and normal of a map of at least 1 x 1"; return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	const size_t n = (size_t)w * h;
	DevBuf<float> dd, dn;
	HIPCHK(e, dd.alloc(n)); HIPCHK(e, dn.alloc(n * 3));
	HIPCHK(e, hipMemcpy(dd, depth, n * sizeof(float), hipMemcpyHostToDevice));
	launchNormalMap(e->stream, dd, dn, w, h, K);
	HIPCHK(e, hipGetLastError());
	HIPCHK(e, hipStreamSynchronize(e->stream));
	HIPCHK(e, hipMemcpy(normal, dn, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
	return 0;
}

} // extern "C"
