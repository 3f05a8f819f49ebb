// pm_host_mesh.hip -- host side of the mesh renderer (kernels: pm_mesh.hip; C ABI: include/pmhip_mesh.h).  Part of the translation unit pm_engine.hip.

// Mesh::ComputeNormalVertices (libs/MVS/Mesh.cpp:356-371) on the host, once per mesh: the float sums run in face order, which no floating atomic keeps, and one pass
// over the faces costs less than their upload.  cv::Point3_::cross and cv::normalize (the norm and the product in double) term by term; no contraction (build flags).
static void meshVertexNormals(const float* V, uint32_t nV, const uint32_t* F, uint32_t nF, float* N) {
	memset(N, 0, sizeof(float) * 3 * (size_t)nV);
	for (size_t f = 0; f < nF; ++f) {
		const float* v0 = V + 3 * (size_t)F[3 * f]; const float* v1 = V + 3 * (size_t)F[3 * f + 1]; const float* v2 = V + 3 * (size_t)F[3 * f + 2];
		const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2], bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
		const float t[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
		for (int k = 0; k < 3; ++k) { float* n = N + 3 * (size_t)F[3 * f + k]; n[0] += t[0]; n[1] += t[1]; n[2] += t[2]; }
	}
	for (size_t i = 0; i < nV; ++i) {
		float* n = N + 3 * i;
		const double nv = sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
		const double s = nv ? 1. / nv : 0.;
		n[0] = (float)(n[0] * s); n[1] = (float)(n[1] * s); n[2] = (float)(n[2] * s);
	}
}

// what a call checks before anything is launched
static int meshCheckViews(pmhip_engine* e, const char* who, int nViews, const double* K9, const double* R9, const double* C3, const int32_t* wh) {
	if (nViews < 0 || (nViews > 0 && (!K9 || !R9 || !C3 || !wh))) { e->err = std::string(who) + ": K, R, C and sizes of every view"; return PMHIP_E_ARG; }
	for (int i = 0; i < nViews; ++i)
		if (wh[2 * i] <= 0 || wh[2 * i + 1] <= 0 || (uint64_t)wh[2 * i] * (uint64_t)wh[2 * i + 1] > (uint64_t)INT_MAX) {
			e->err = std::string(who) + ": view " + std::to_string(i) + " is " + std::to_string(wh[2 * i]) + " x " + std::to_string(wh[2 * i + 1]); return PMHIP_E_ARG; }
	if (!e->mesh.set) { e->err = std::string(who) + ": no mesh (pmhip_mesh_set)"; return PMHIP_E_STATE; }
	return 0;
}

// The views [first, first + n) of a call rendered into m.keys / m.depth / m.normal (n fits the budget: meshBatchEnd).  Leaves the stream running.
static int meshRenderBatch(pmhip_engine* e, int first, int n, const double* K9, const double* R9, const double* C3, const int32_t* wh, const unsigned char* wantNormal) {
	MeshMem& m = e->mesh;
	std::vector<PMMeshView> hv((size_t)n);
	size_t pix = 0, maxPix = 0; bool anyNormal = false;
	for (int b = 0; b < n; ++b) {
		const int i = first + b;
		PMMeshView& v = hv[b];
		memset(&v, 0, sizeof(v));
		memcpy(v.R, R9 + 9 * (size_t)i, 72); memcpy(v.C, C3 + 3 * (size_t)i, 24);
		const double* K = K9 + 9 * (size_t)i;
		v.k00 = K[0]; v.k11 = K[4]; v.k02 = K[2]; v.k12 = K[5];
		for (int k = 0; k < 9; ++k) v.Rf[k] = (float)v.R[k];
		v.w = wh[2 * i]; v.h = wh[2 * i + 1]; v.wantNormal = wantNormal && wantNormal[i]; v.pix = pix;
		anyNormal = anyNormal || v.wantNormal;
		const size_t p = (size_t)v.w * v.h;
		pix += p; maxPix = std::max(maxPix, p);
	}
	HIPCHK(e, m.views.reserve((size_t)n)); HIPCHK(e, m.rec.reserve((size_t)n * m.nV)); HIPCHK(e, m.keys.reserve(pix)); HIPCHK(e, m.depth.reserve(pix));
	if (anyNormal) HIPCHK(e, m.normal.reserve(3 * pix));
	HIPCHK(e, m.largeCount.reserve((size_t)n)); HIPCHK(e, m.largeList.reserve((size_t)n * m.nF));
	HIPCHK(e, hipMemcpyAsync(m.views, hv.data(), sizeof(PMMeshView) * n, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));                          // (hv is pageable and leaves scope)
	for (hipEvent_t& ev : m.ev) if (!ev) HIPCHK(e, hipEventCreate(&ev));
	HIPCHK(e, hipEventRecord(m.ev[0], e->stream));
	HIPCHK(e, hipMemsetAsync(m.keys, 0xFF, sizeof(unsigned long long) * pix, e->stream));
	HIPCHK(e, hipMemsetAsync(m.largeCount, 0, sizeof(uint32_t) * n, e->stream));
	hipLaunchKernelGGL(pm_mesh_vertex_kernel, dim3(resampleBlocks(m.nV, PM_MESH_MAX_BLOCKS), n), dim3(256), 0, e->stream, m.views, m.verts, m.nV, m.rec);
	hipLaunchKernelGGL(pm_mesh_face_kernel, dim3(resampleBlocks(m.nF, PM_MESH_MAX_BLOCKS), n), dim3(256), 0, e->stream, m.views, m.rec, m.nV, m.faces, m.nF, m.boxMax,
	                   m.keys, m.largeCount, m.largeList);
	hipLaunchKernelGGL(pm_mesh_large_kernel, dim3(std::min<uint32_t>(m.nF, PM_MESH_LARGE_BLOCKS), n), dim3(256), 0, e->stream, m.views, m.rec, m.nV, m.faces, m.nF,
	                   m.keys, m.largeCount, m.largeList);
	hipLaunchKernelGGL(pm_mesh_resolve_kernel, dim3(resampleBlocks(maxPix, PM_MESH_MAX_BLOCKS), n), dim3(256), 0, e->stream, m.views, m.rec, m.nV, m.faces, m.normals,
	                   m.keys, m.depth, m.normal);
	HIPCHK(e, hipGetLastError());
	return 0;
}

// one past the last view of the batch that starts at `first`: views are added while their records, lists, keys and maps fit the budget; always at least one
static int meshBatchEnd(const MeshMem& m, int first, int nViews, const int32_t* wh, const unsigned char* wantNormal) {
	uint64_t bytes = 0;
	int i = first;
	for (; i < nViews; ++i) {
		const uint64_t p = (uint64_t)wh[2 * i] * wh[2 * i + 1];
		const uint64_t b = sizeof(PMMeshVert) * (uint64_t)m.nV + 4 * (uint64_t)m.nF + p * (8 + 4 + (wantNormal && wantNormal[i] ? 12 : 0)) + sizeof(PMMeshView) + 4;
		if (i > first && bytes + b > m.batchBytes) break;
		bytes += b;
	}
	return i;
}

// the listed faces and the device time of the batch just rendered, for the statistics (the stream is synchronised)
static int meshCountLarge(pmhip_engine* e, int n) {
	float ms = 0;
	if (hipEventElapsedTime(&ms, e->mesh.ev[0], e->mesh.ev[1]) == hipSuccess) e->mesh.statMs += ms;
	std::vector<uint32_t> c((size_t)n);
	HIPCHK(e, hipMemcpy(c.data(), e->mesh.largeCount, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
	for (uint32_t v : c) e->mesh.statLarge += v;
	return 0;
}

extern "C" {

int pmhip_mesh_set(pmhip_engine* e, const float* vertices, uint32_t nVertices, const uint32_t* faces, uint32_t nFaces, const float* vertexNormals) {
	if (!e) return PMHIP_E_ARG;
	if (!vertices || !faces || nVertices == 0 || nFaces == 0) { e->err = "pmhip_mesh_set: vertices and faces of a mesh of at least one face"; return PMHIP_E_ARG; }
	for (size_t k = 0; k < 3 * (size_t)nFaces; ++k)
		if (faces[k] >= nVertices) { e->err = "pmhip_mesh_set: face " + std::to_string(k / 3) + " names vertex " + std::to_string(faces[k]) + " of " + std::to_string(nVertices); return PMHIP_E_ARG; }
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	std::vector<float> computed;
	if (!vertexNormals) { computed.resize(3 * (size_t)nVertices); meshVertexNormals(vertices, nVertices, faces, nFaces, computed.data()); vertexNormals = computed.data(); }
	freeMesh(e);
	MeshMem& m = e->mesh;
	HIPCHK(e, m.verts.alloc(3 * (size_t)nVertices)); HIPCHK(e, m.normals.alloc(3 * (size_t)nVertices)); HIPCHK(e, m.faces.alloc(3 * (size_t)nFaces));
	HIPCHK(e, hipMemcpy(m.verts, vertices, sizeof(float) * 3 * nVertices, hipMemcpyHostToDevice));
	HIPCHK(e, hipMemcpy(m.normals, vertexNormals, sizeof(float) * 3 * nVertices, hipMemcpyHostToDevice));
	HIPCHK(e, hipMemcpy(m.faces, faces, sizeof(uint32_t) * 3 * nFaces, hipMemcpyHostToDevice));
	m.nV = nVertices; m.nF = nFaces; m.set = true;
	return 0;
}

int pmhip_mesh_get_vertex_normals(pmhip_engine* e, float* out) {
	if (!e) return PMHIP_E_ARG;
	if (!out) { e->err = "pmhip_mesh_get_vertex_normals: no buffer"; return PMHIP_E_ARG; }
	if (!e->mesh.set) { e->err = "pmhip_mesh_get_vertex_normals: no mesh (pmhip_mesh_set)"; return PMHIP_E_STATE; }
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipMemcpy(out, e->mesh.normals, sizeof(float) * 3 * e->mesh.nV, hipMemcpyDeviceToHost));
	return 0;
}

int pmhip_mesh_project(pmhip_engine* e, int nViews, const double* K9, const double* R9, const double* C3, const int32_t* wh, float* const* depthOut, float* const* normalOut) {
	if (!e) return PMHIP_E_ARG;
	int rc = meshCheckViews(e, "pmhip_mesh_project", nViews, K9, R9, C3, wh);
	if (rc) return rc;
	if (nViews > 0 && !depthOut) { e->err = "pmhip_mesh_project: no depth maps to write"; return PMHIP_E_ARG; }
	for (int i = 0; i < nViews; ++i) if (!depthOut[i]) { e->err = "pmhip_mesh_project: view " + std::to_string(i) + " has no depth map to write"; return PMHIP_E_ARG; }
	if (nViews == 0) return 0;
	HIPCHK(e, hipSetDevice(e->device));
	MeshMem& m = e->mesh;
	std::vector<unsigned char> want((size_t)nViews, 0);
	for (int i = 0; i < nViews; ++i) want[i] = normalOut && normalOut[i];
	m.statBatches = m.statLarge = 0; m.statMs = 0;
	for (int first = 0; first < nViews;) {
		const int end = meshBatchEnd(m, first, nViews, wh, want.data());
		if ((rc = meshRenderBatch(e, first, end - first, K9, R9, C3, wh, want.data())) != 0) return rc;
		HIPCHK(e, hipEventRecord(m.ev[1], e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));
		size_t pix = 0;
		for (int i = first; i < end; ++i) {
			const size_t p = (size_t)wh[2 * i] * wh[2 * i + 1];
			HIPCHK(e, hipMemcpy(depthOut[i], m.depth + pix, sizeof(float) * p, hipMemcpyDeviceToHost));
			if (want[i]) HIPCHK(e, hipMemcpy(normalOut[i], m.normal + 3 * pix, sizeof(float) * 3 * p, hipMemcpyDeviceToHost));
			pix += p;
		}
		if ((rc = meshCountLarge(e, end - first)) != 0) return rc;
		++m.statBatches;
		first = end;
	}
	return 0;
}

int pmhip_mesh_visibility(pmhip_engine* e, int nViews, const double* K9, const double* R9, const double* C3, const int32_t* wh, uint32_t* bitsOut, float thFrontDepth) {
	if (!e) return PMHIP_E_ARG;
	int rc = meshCheckViews(e, "pmhip_mesh_visibility", nViews, K9, R9, C3, wh);
	if (rc) return rc;
	if (nViews > 0 && !bitsOut) { e->err = "pmhip_mesh_visibility: no bitset to write"; return PMHIP_E_ARG; }
	if (nViews == 0) return 0;
	HIPCHK(e, hipSetDevice(e->device));
	MeshMem& m = e->mesh;
	const int nWords = (nViews + 31) / 32;
	HIPCHK(e, m.bits.reserve((size_t)m.nV * nWords));
	m.statBatches = m.statLarge = 0; m.statMs = 0;
	for (int first = 0; first < nViews;) {
		const int end = meshBatchEnd(m, first, nViews, wh, nullptr);
		if ((rc = meshRenderBatch(e, first, end - first, K9, R9, C3, wh, nullptr)) != 0) return rc;
		// every word the batch touches gets one writer per vertex: a word an earlier batch began is read first (pm_mesh_visible_kernel)
		hipLaunchKernelGGL(pm_mesh_visible_kernel, dim3(resampleBlocks(m.nV, PM_MESH_MAX_BLOCKS), (end - 1) / 32 - first / 32 + 1), dim3(256), 0, e->stream, m.views, m.rec,
		                   m.nV, m.depth, first, end - first, nWords, thFrontDepth, m.bits);
		HIPCHK(e, hipGetLastError());
		HIPCHK(e, hipEventRecord(m.ev[1], e->stream));
		HIPCHK(e, hipStreamSynchronize(e->stream));                      // (the next batch overwrites the records and maps)
		if ((rc = meshCountLarge(e, end - first)) != 0) return rc;
		++m.statBatches;
		first = end;
	}
	HIPCHK(e, hipMemcpy(bitsOut, m.bits, sizeof(uint32_t) * (size_t)m.nV * nWords, hipMemcpyDeviceToHost));
	return 0;
}

int pmhip_mesh_release(pmhip_engine* e) {
	if (!e) return PMHIP_E_ARG;
	hipSetDevice(e->device);
	hipStreamSynchronize(e->stream);
	freeMesh(e);
	return 0;
}

int pmhip_mesh_set_tuning(pmhip_engine* e, int boxPixels, uint64_t batchBytes) {
	if (!e) return PMHIP_E_ARG;
	if (boxPixels) e->mesh.boxMax = boxPixels < 0 ? PM_MESH_BOX_PIXELS : boxPixels;
	if (batchBytes) e->mesh.batchBytes = batchBytes;
	return 0;
}

int pmhip_mesh_get_stats(pmhip_engine* e, uint64_t* out) {
	if (!e || !out) return PMHIP_E_ARG;
	out[0] = e->mesh.statBatches; out[1] = e->mesh.statLarge; out[2] = (uint64_t)e->mesh.boxMax; out[3] = e->mesh.batchBytes;
	out[4] = (uint64_t)(e->mesh.statMs * 1e3 + .5);
	return 0;
}

} // extern "C"
