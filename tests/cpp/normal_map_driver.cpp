// Drives include/DenseDepthMapsHIP.hpp the way a host that resumes depth maps from files would: every view's depth and confidence are installed (SetDepthMap), some of
// them without normals, and EstimateMissingNormals makes those on the device; then the host-buffer form (pmhip_estimate_normal_map) on the first view's depths.
// Usage: normal_map_driver <scene.bin> <out.bin>
//   scene.bin: i32 n, w, h | per view: i32 vw, vh, hasNormal, f64 K[9] R[9] C[3], f32 depth[vw*vh], conf[vw*vh], normal[vw*vh*3] if hasNormal
//   out.bin:   per view f32 depth[vw*vh] normal[vw*vh*3] conf[vw*vh] | f32 normal[vw0*vh0*3] of pmhip_estimate_normal_map(view 0)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "DenseDepthMapsHIP.hpp"

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
	int32_t hd[3]; if (fread(hd, 4, 3, f) != 3) return 4;
	const int n = hd[0], w = hd[1], h = hd[2];
	std::vector<MVS::DenseDepthMapsHIP::View> views((size_t)n);
	std::vector<std::vector<float>> gray((size_t)n), depth((size_t)n), conf((size_t)n), normal((size_t)n);
	for (int i = 0; i < n; ++i) {
		auto& v = views[(size_t)i];
		int32_t vh[3]; double cam[21];
		if (fread(vh, 4, 3, f) != 3 || fread(cam, 8, 21, f) != 21) return 4;
		const size_t P = (size_t)vh[0] * vh[1];
		depth[(size_t)i].resize(P); conf[(size_t)i].resize(P); gray[(size_t)i].assign(P, 0.5f);
		if (fread(depth[(size_t)i].data(), 4, P, f) != P || fread(conf[(size_t)i].data(), 4, P, f) != P) return 4;
		if (vh[2]) { normal[(size_t)i].resize(P * 3); if (fread(normal[(size_t)i].data(), 4, P * 3, f) != P * 3) return 4; }
		v.w = vh[0]; v.h = vh[1]; v.gray = gray[(size_t)i].data();
		memcpy(v.K, cam, 72); memcpy(v.R, cam + 9, 72); memcpy(v.C, cam + 18, 24);
		v.dMin = 0.1f; v.dMax = 100.f; v.ID = (uint32_t)i;
		for (int j = 0; j < n; ++j) if (j != i) v.neighbors.push_back(j);
	}
	fclose(f);
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVS::DenseDepthMapsHIP::Options opt;
	opt.nSubResolutionLevels = 0;
	try {
		dense.LoadScene(views, w, h, opt);
		if (dense.EstimateMissingNormals() != 0) return 8;                           // nothing installed yet: a no-op
		size_t without = 0;
		for (int i = 0; i < n; ++i) {
			dense.SetDepthMap(i, depth[(size_t)i].data(), normal[(size_t)i].empty() ? nullptr : normal[(size_t)i].data(), conf[(size_t)i].data());
			without += normal[(size_t)i].empty();
		}
		if (dense.EstimateMissingNormals() != without || dense.EstimateMissingNormals() != 0) return 9;
		f = fopen(argv[2], "wb"); if (!f) return 6;
		for (int i = 0; i < n; ++i) {
			const size_t P = (size_t)dense.ViewWidth(i) * dense.ViewHeight(i);
			std::vector<float> d(P), nrm(P * 3), c(P);
			dense.GetMaps(i, d.data(), nrm.data(), c.data());
			fwrite(d.data(), 4, P, f); fwrite(nrm.data(), 4, P * 3, f); fwrite(c.data(), 4, P, f);
		}
		std::vector<float> one(depth[0].size() * 3);
		if (pmhip_estimate_normal_map(dense.engine(), views[0].K, depth[0].data(), views[0].w, views[0].h, one.data()) != PMHIP_OK) return 10;
		if (pmhip_estimate_normal_map(dense.engine(), views[0].K, depth[0].data(), 0, views[0].h, one.data()) != PMHIP_E_ARG) return 11;
		fwrite(one.data(), 4, one.size(), f);
		fclose(f);
		printf("views %d, normals estimated for %zu\n", n, without);
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
