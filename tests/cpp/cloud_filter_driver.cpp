// Drives include/DenseDepthMapsHIP.hpp::FilterPointCloud the way a patched Scene::PointCloudFilter would: estimate, fuse, finish with
// --estimate-colors 1 --estimate-normals 1, then --filter-point-cloud <th> after RemoveMinViews(<minViews>).
// Usage: cloud_filter_driver <scene.bin> <out.bin> <th> <minViews> [seed]
//   scene.bin: as tests/cpp/dense_driver.cpp
//   out.bin:   twice (finished, then filtered): u64 nPoints, nViews | f32 points[3*nPoints] | u32 viewStart[nPoints+1] | u32 views[nViews] | f32 weights[nViews] |
//              u8 colors[3*nPoints] | f32 normals[3*nPoints]; then u64 n | i32 visibility[n]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "OptDenseHIP.hpp"

static void put(FILE* f, const MVS::DenseDepthMapsHIP::PointCloud& pc) {
	const uint64_t cnt[2] = {(uint64_t)pc.size(), (uint64_t)pc.views.size()};
	fwrite(cnt, 8, 2, f); fwrite(pc.points.data(), 4, pc.points.size(), f); fwrite(pc.viewStart.data(), 4, pc.viewStart.size(), f); fwrite(pc.views.data(), 4, pc.views.size(), f); fwrite(pc.weights.data(), 4, pc.weights.size(), f);
	fwrite(pc.colors.data(), 1, pc.colors.size(), f); fwrite(pc.normals.data(), 4, pc.normals.size(), f);
}

int main(int argc, char** argv) {
	if (argc < 5) return 2;
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
	MVS::DenseDepthMapsHIP::OBB roi;
	memset(&roi, 0, sizeof(roi));
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVSFOptDense od;
	mvsf_optdense_init(&od);                                                     // the table's defaults
	od.nEstimateColors = 1; od.nEstimateNormals = 1;                             // --estimate-colors 1 --estimate-normals 1
	MVS::DenseDepthMapsHIP::Options opt = MVS::DenseOptionsFrom(od, argc > 5 ? (uint32_t)atoi(argv[5]) : 31u);
	if (opt.bEstimateColor || opt.bEstimateNormal || !opt.bPointColors || !opt.bPointNormals) return 8;
	try {
		dense.LoadScene(views, w, h, opt);
		dense.ComputeDepthMaps();
		MVS::DenseDepthMapsHIP::PointCloud pc;
		dense.FuseDepthMaps(pc);                                                 // SceneDensify.cpp:1695-1712
		dense.FinishPointCloud(pc, roi, false, 0.f);                             // :1724-1737
		f = fopen(argv[2], "wb"); if (!f) return 6;
		put(f, pc);
		const size_t before = pc.size();
		std::vector<int32_t> vis;
		dense.FilterPointCloud(pc, atoi(argv[3]), (unsigned)atoi(argv[4]), &vis);  // Scene::PointCloudFilter, :2225-2359
		put(f, pc);
		const uint64_t nVis = vis.size();
		fwrite(&nVis, 8, 1, f); fwrite(vis.data(), 4, vis.size(), f);
		fclose(f);
		printf("finished then filtered: %zu -> %zu points, %zu votes\n", before, pc.size(), vis.size());
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
