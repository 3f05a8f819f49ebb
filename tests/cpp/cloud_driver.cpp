// Drives include/OptDenseHIP.hpp + DenseDepthMapsHIP.hpp through Scene::DenseReconstruction's last block the way a patched SceneDensify.cpp:1724-1737 would
// (INTEGRATION.md): estimate, fuse, then FinishPointCloud with --estimate-colors 1 --estimate-normals 1 and a crop to an OBB.
// Usage: cloud_driver <scene.bin> <out.bin> <obb.bin> [seed]
//   scene.bin: as tests/cpp/dense_driver.cpp;  obb.bin: f32 rot[9] pos[3] ext[3] border
//   out.bin:   twice (fused, then finished): u64 nPoints, nViews | f32 points[3*nPoints] | u32 viewStart[nPoints+1] | u32 views[nViews] | u8 colors[3*nPoints] | f32 normals[3*nPoints]
//              (colours / normals only in the finished cloud)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "OptDenseHIP.hpp"

static void put(FILE* f, const MVS::DenseDepthMapsHIP::PointCloud& pc) {
	const uint64_t cnt[2] = {(uint64_t)pc.size(), (uint64_t)pc.views.size()};
	fwrite(cnt, 8, 2, f); fwrite(pc.points.data(), 4, pc.points.size(), f); fwrite(pc.viewStart.data(), 4, pc.viewStart.size(), f); fwrite(pc.views.data(), 4, pc.views.size(), f);
	fwrite(pc.colors.data(), 1, pc.colors.size(), f); fwrite(pc.normals.data(), 4, pc.normals.size(), f);
}

int main(int argc, char** argv) {
	if (argc < 4) return 2;
	FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
	int32_t hd[4]; if (fread(hd, 4, 4, f) != 4) return 4;
	const int n = hd[0], w = hd[1], h = hd[2], ns = hd[3];
	const size_t P = (size_t)w * h;
	std::vector<std::vector<float>> gray((size_t)n, std::vector<float>(P));
	std::vector<std::vector<unsigned char>> bgr((size_t)n, std::vector<unsigned char>(P * 3));
	std::vector<MVS::DenseDepthMapsHIP::View> views((size_t)n);
	for (int i = 0; i < n; ++i) {
		auto& v = views[(size_t)i];
		double cam[21]; float rng[2]; std::vector<int32_t> nb((size_t)ns);
		if (fread(gray[(size_t)i].data(), 4, P, f) != P || fread(bgr[(size_t)i].data(), 1, P * 3, f) != P * 3 || fread(cam, 8, 21, f) != 21 || fread(rng, 4, 2, f) != 2 ||
		    fread(nb.data(), 4, (size_t)ns, f) != (size_t)ns) return 4;
		v.gray = gray[(size_t)i].data(); v.bgr = bgr[(size_t)i].data();
		memcpy(v.K, cam, 72); memcpy(v.R, cam + 9, 72); memcpy(v.C, cam + 18, 24);
		v.dMin = rng[0]; v.dMax = rng[1]; v.neighbors = nb; v.ID = (uint32_t)i;
	}
	fclose(f);
	float ob[16];
	f = fopen(argv[3], "rb"); if (!f || fread(ob, 4, 16, f) != 16) return 4;
	fclose(f);
	MVS::DenseDepthMapsHIP::OBB roi;
	memcpy(roi.rot, ob, 36); memcpy(roi.pos, ob + 9, 12); memcpy(roi.ext, ob + 12, 12);
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVSFOptDense od;
	mvsf_optdense_init(&od);                                                     // the table's defaults
	od.nEstimateColors = 1; od.nEstimateNormals = 1;                             // --estimate-colors 1 --estimate-normals 1
	MVS::DenseDepthMapsHIP::Options opt = MVS::DenseOptionsFrom(od, argc > 4 ? (uint32_t)atoi(argv[4]) : 31u);
	if (opt.bEstimateColor || opt.bEstimateNormal || !opt.bPointColors || !opt.bPointNormals) return 8;
	try {
		dense.LoadScene(views, w, h, opt);
		dense.ComputeDepthMaps();
		MVS::DenseDepthMapsHIP::PointCloud pc;
		dense.FuseDepthMaps(pc);                                                 // SceneDensify.cpp:1695-1712
		f = fopen(argv[2], "wb"); if (!f) return 6;
		put(f, pc);
		dense.FinishPointCloud(pc, roi, true, ob[15]);                           // :1724-1737
		put(f, pc);
		fclose(f);
		printf("fused then finished: %zu points, colours %zu, normals %zu\n", pc.size(), pc.colors.size() / 3, pc.normals.size() / 3);
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
