// A C++ host that seeds a resident view from its point mesh: mvsf_point_mesh (libmvsfront.so) -> MVS::PatchMatchHIP::SeedView -> pmhip_scene_estimate, the route
// INTEGRATION.md describes next to mvsf_init_depth_map.  Nothing but the mesh crosses to the device for the seed.
// Usage: seed_view_driver <scene.mvs> <job.bin> <out.bin>
//   job.bin: i32 n, w, h, nLevels, nIters, seed, mode, nPoints | per view: f64 K[9] R[9] C[3], f32 dMin dMax, i32 nNb, i32 nb[nNb], f32 gray[w*h] | u32 points[nPoints]
//            (view 0 is estimated; its dMin / dMax in the file are ignored: the host takes them from the mesh, as InitViews does)
//   out.bin: f32 dMin dMax | seed depth[w*h] normal[w*h*3] | estimated depth[w*h] normal[w*h*3] conf[w*h]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "PatchMatchHIP.hpp"
#include "mvsfront.h"

int main(int argc, char** argv) {
	if (argc < 4) return 2;
	mvsf_scene* sc = nullptr;
	if (mvsf_load(argv[1], &sc) != 0) return 3;
	FILE* f = fopen(argv[2], "rb"); if (!f) return 3;
	int32_t hd[8]; if (fread(hd, 4, 8, f) != 8) return 4;
	const int n = hd[0], w = hd[1], h = hd[2], nLevels = hd[3], mode = hd[6], nPoints = hd[7];
	const size_t P = (size_t)w * h;
	struct View { double cam[21]; float range[2]; std::vector<int32_t> nb; std::vector<float> gray; };
	std::vector<View> views((size_t)n);
	for (View& v : views) {
		int32_t nNb;
		if (fread(v.cam, 8, 21, f) != 21 || fread(v.range, 4, 2, f) != 2 || fread(&nNb, 4, 1, f) != 1) return 4;
		v.nb.resize((size_t)nNb); v.gray.resize(P);
		if (fread(v.nb.data(), 4, (size_t)nNb, f) != (size_t)nNb || fread(v.gray.data(), 4, P, f) != P) return 4;
	}
	std::vector<uint32_t> points((size_t)nPoints);
	if (fread(points.data(), 4, (size_t)nPoints, f) != (size_t)nPoints) return 4;
	fclose(f);
	// the mesh of view 0's sparse points: the counts first, then the arrays
	int nVerts = 0, nFaces = 0; float dMin = 0, dMax = 0;
	if (mvsf_point_mesh(sc, 0, w, h, points.data(), nPoints, 0, 0.f, nullptr, nullptr, nullptr, 0, &nVerts, nullptr, 0, &nFaces, nullptr, nullptr) != 0) return 5;
	std::vector<float> proj((size_t)nVerts * 2), z((size_t)nVerts), nrm((size_t)nVerts * 3); std::vector<uint32_t> faces((size_t)nFaces * 3);
	if (mvsf_point_mesh(sc, 0, w, h, points.data(), nPoints, 0, 0.f, proj.data(), z.data(), nrm.data(), nVerts, &nVerts, faces.data(), nFaces, &nFaces, &dMin, &dMax) != 0) return 5;
	if (nVerts > 1 && mvsf_point_mesh(sc, 0, w, h, points.data(), nPoints, 0, 0.f, proj.data(), z.data(), nrm.data(), nVerts - 1, &nVerts, faces.data(), nFaces, &nFaces, &dMin, &dMax) != -2) return 5;
	dMin *= 0.9f; dMax *= 1.1f;                                                        // DepthMapsData::InitViews
	mvsf_free(sc);
	MVS::PatchMatchHIP pm(0);
	if (!pm.IsValid()) { fprintf(stderr, "no device\n"); return 6; }
	try {
		pm.Init(false);
		pmhip_engine* e = pm.engine();
		if (pmhip_scene_create(e, n, w, h, nLevels) != PMHIP_OK) return 7;
		for (int i = 0; i < n; ++i) {
			View& v = views[(size_t)i];
			if (pmhip_scene_set_view(e, i, v.gray.data(), 0, v.cam, v.cam + 9, v.cam + 18, i ? v.range[0] : dMin, i ? v.range[1] : dMax, v.nb.data(), (int)v.nb.size()) != PMHIP_OK) return 7;
		}
		pm.SeedView(0, mode, proj.data(), z.data(), nrm.data(), (uint32_t)nVerts, faces.data(), (uint32_t)nFaces);
		std::vector<float> d(P), nm(P * 3), c(P);
		f = fopen(argv[3], "wb"); if (!f) return 8;
		fwrite(&dMin, 4, 1, f); fwrite(&dMax, 4, 1, f);
		if (pmhip_scene_get_maps(e, 0, d.data(), nm.data(), nullptr) != PMHIP_OK) return 9;
		fwrite(d.data(), 4, P, f); fwrite(nm.data(), 4, P * 3, f);
		MVS::PatchMatchHIP::Options opt;
		opt.nSubResolutionLevels = (uint32_t)nLevels; opt.nEstimationIters = (uint32_t)hd[4]; opt.seed = (uint32_t)hd[5];
		const int32_t id0 = 0;
		if (pmhip_scene_estimate(e, &id0, 1, &opt, -1, 1) != PMHIP_OK) { fprintf(stderr, "%s\n", pmhip_last_error(e)); return 10; }
		if (pmhip_scene_get_maps(e, 0, d.data(), nm.data(), c.data()) != PMHIP_OK) return 9;
		fwrite(d.data(), 4, P, f); fwrite(nm.data(), 4, P * 3, f); fwrite(c.data(), 4, P, f);
		fclose(f);
		bool refused = false;                                                          // a refusal surfaces as the adapter's exception, with the library's reason
		try { pm.SeedView(n, mode, proj.data(), z.data(), nullptr, (uint32_t)nVerts, faces.data(), (uint32_t)nFaces); } catch (const std::exception&) { refused = true; }
		if (!refused) return 11;
		printf("vertices %d, faces %d, range %g .. %g\n", nVerts, nFaces, dMin, dMax);
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 12; }
	return 0;
}
