// Drives include/DenseDepthMapsHIP.hpp the way a host that exports a scan's depth maps would (Scene::ExportMeshToDepthMaps): the scene's views are loaded, the mesh is
// made resident (SetMesh, vertex normals computed by the engine), ProjectMesh renders it into the listed views at their own sizes -- once with normals, once depth
// only -- and ReleaseMesh frees it; a render without a mesh must throw.
// Usage: mesh_project_driver <scene.bin> <out.bin>
//   scene.bin: i32 n, w, h, nVertices, nFaces | per view: i32 vw, vh, f64 K[9] R[9] C[3] | f32 vertices[3 nVertices] | u32 faces[3 nFaces]
//   out.bin:   per view f32 depth[vw*vh] normal[vw*vh*3] | per view f32 depth[vw*vh] of the depth-only call
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "DenseDepthMapsHIP.hpp"

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
	int32_t hd[5]; if (fread(hd, 4, 5, f) != 5) return 4;
	const int n = hd[0], w = hd[1], h = hd[2];
	std::vector<MVS::DenseDepthMapsHIP::View> views((size_t)n);
	std::vector<std::vector<float>> gray((size_t)n);
	for (int i = 0; i < n; ++i) {
		auto& v = views[(size_t)i];
		int32_t vh[2]; double cam[21];
		if (fread(vh, 4, 2, f) != 2 || fread(cam, 8, 21, f) != 21) return 4;
		gray[(size_t)i].assign((size_t)vh[0] * vh[1], 0.5f);
		v.w = vh[0]; v.h = vh[1]; v.gray = gray[(size_t)i].data();
		memcpy(v.K, cam, 72); memcpy(v.R, cam + 9, 72); memcpy(v.C, cam + 18, 24);
		v.dMin = 0.1f; v.dMax = 100.f; v.ID = (uint32_t)i;
		for (int j = 0; j < n; ++j) if (j != i) v.neighbors.push_back(j);
	}
	std::vector<float> V((size_t)hd[3] * 3); std::vector<uint32_t> F((size_t)hd[4] * 3);
	if (fread(V.data(), 4, V.size(), f) != V.size() || fread(F.data(), 4, F.size(), f) != F.size()) return 4;
	fclose(f);
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVS::DenseDepthMapsHIP::Options opt;
	opt.nSubResolutionLevels = 0;
	try {
		dense.LoadScene(views, w, h, opt);
		std::vector<int32_t> ids;
		for (int i = n - 1; i >= 0; --i) ids.push_back(i);                           // any order: the maps come back in the order asked
		std::vector<std::vector<float>> depth, normal, depthOnly, none;
		bool threw = false;
		try { dense.ProjectMesh(ids, depth, normal); } catch (const std::exception&) { threw = true; }
		if (!threw) return 8;                                                        // no mesh yet
		dense.SetMesh(V.data(), (uint32_t)hd[3], F.data(), (uint32_t)hd[4]);
		dense.ProjectMesh(ids, depth, normal);
		dense.ProjectMesh(ids, depthOnly, none, false);
		if (!none.empty()) return 9;
		dense.ReleaseMesh();
		f = fopen(argv[2], "wb"); if (!f) return 6;
		for (int i = 0; i < n; ++i) { const size_t k = (size_t)(n - 1 - i); fwrite(depth[k].data(), 4, depth[k].size(), f); fwrite(normal[k].data(), 4, normal[k].size(), f); }
		for (int i = 0; i < n; ++i) { const size_t k = (size_t)(n - 1 - i); fwrite(depthOnly[k].data(), 4, depthOnly[k].size(), f); }
		fclose(f);
		printf("views %d, vertices %d, faces %d\n", n, hd[3], hd[4]);
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
