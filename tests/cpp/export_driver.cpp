// Drives the output methods of include/DenseDepthMapsHIP.hpp: a scene of three views (one of its own size) gets its maps through SetDepthMap; DepthImage, ConfImage and
// ViewCloud run for every view; then a cloud given by the caller becomes the resident one and SavePointCloud writes it with scales, with its view lists, and thinned by
// view count.
// Usage: export_driver <scene.bin> <out dir>
//   scene.bin: i32 n, w, h | per view: i32 vw, vh, hasColour, f64 K[9] R[9] C[3], f32 depth[vw*vh], conf[vw*vh], normal[vw*vh*3], u8 bgr[vw*vh*3] if hasColour
//              | i32 nPoints, nViews, f32 scaleMult, f32 points[3 nPoints], u32 viewStart[nPoints + 1], u32 views[nViews], f32 weights[nViews]
//   out dir:   depth<i>.rgb, conf<i>.gray (raw bytes), view<i>.ply, cloud_scale.ply, cloud_views.ply, cloud_2views.ply
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "DenseDepthMapsHIP.hpp"

static void dump(const std::string& path, const std::vector<unsigned char>& bytes) {
	FILE* f = fopen(path.c_str(), "wb"); if (!f) exit(6);
	fwrite(bytes.data(), 1, bytes.size(), f); fclose(f);
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	const std::string out = argv[2];
	FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
	int32_t hd[3]; if (fread(hd, 4, 3, f) != 3) return 4;
	const int n = hd[0], w = hd[1], h = hd[2];
	std::vector<MVS::DenseDepthMapsHIP::View> views((size_t)n);
	std::vector<std::vector<float>> gray((size_t)n), depth((size_t)n), conf((size_t)n), normal((size_t)n);
	std::vector<std::vector<unsigned char>> bgr((size_t)n);
	for (int i = 0; i < n; ++i) {
		auto& v = views[(size_t)i];
		int32_t vh[3]; double cam[21];
		if (fread(vh, 4, 3, f) != 3 || fread(cam, 8, 21, f) != 21) return 4;
		const size_t P = (size_t)vh[0] * vh[1];
		depth[(size_t)i].resize(P); conf[(size_t)i].resize(P); normal[(size_t)i].resize(P * 3); gray[(size_t)i].assign(P, 0.5f);
		if (fread(depth[(size_t)i].data(), 4, P, f) != P || fread(conf[(size_t)i].data(), 4, P, f) != P || fread(normal[(size_t)i].data(), 4, P * 3, f) != P * 3) return 4;
		if (vh[2]) { bgr[(size_t)i].resize(P * 3); if (fread(bgr[(size_t)i].data(), 1, P * 3, f) != P * 3) return 4; v.bgr = bgr[(size_t)i].data(); }
		v.w = vh[0]; v.h = vh[1]; v.gray = gray[(size_t)i].data();
		memcpy(v.K, cam, 72); memcpy(v.R, cam + 9, 72); memcpy(v.C, cam + 18, 24);
		v.dMin = 0.1f; v.dMax = 100.f; v.ID = (uint32_t)i;
		for (int j = 0; j < n; ++j) if (j != i) v.neighbors.push_back(j);
	}
	int32_t ch[2]; float scaleMult;
	if (fread(ch, 4, 2, f) != 2 || fread(&scaleMult, 4, 1, f) != 1) return 4;
	MVS::DenseDepthMapsHIP::PointCloud pc;
	pc.points.resize((size_t)ch[0] * 3); pc.viewStart.resize((size_t)ch[0] + 1); pc.views.resize((size_t)ch[1]); pc.weights.resize((size_t)ch[1]);
	if (fread(pc.points.data(), 4, pc.points.size(), f) != pc.points.size() || fread(pc.viewStart.data(), 4, pc.viewStart.size(), f) != pc.viewStart.size() ||
	    fread(pc.views.data(), 4, pc.views.size(), f) != pc.views.size() || fread(pc.weights.data(), 4, pc.weights.size(), f) != pc.weights.size()) return 4;
	fclose(f);
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVS::DenseDepthMapsHIP::Options opt;
	opt.nSubResolutionLevels = 0;
	try {
		dense.LoadScene(views, w, h, opt);
		std::vector<unsigned char> img;
		for (int i = 0; i < n; ++i) {
			dense.SetDepthMap(i, depth[(size_t)i].data(), normal[(size_t)i].data(), conf[(size_t)i].data());
			const std::string si = std::to_string(i);
			const std::pair<float, float> range = dense.DepthImage(i, img);
			if (!(range.first <= range.second)) return 8;
			dump(out + "/depth" + si + ".rgb", img);
			if (!dense.ConfImage(i, img)) return 9;
			dump(out + "/conf" + si + ".gray", img);
			dense.NormalImage(i, img);
			if (img.size() != depth[(size_t)i].size() * 3) return 10;
			uint64_t count = 0;
			if (!dense.ViewCloud(i, out + "/view" + si + ".ply", i != 1, &count) || !count) return 11;      // (the middle view without normals: the 15-byte layout)
		}
		if (pmhip_scene_cloud_set(dense.engine(), pc.points.data(), pc.viewStart.data(), pc.views.data(), pc.weights.data(), pc.size()) != PMHIP_OK) return 12;
		if (!dense.SavePointCloud(out + "/cloud_scale.ply", pc, true, 0, scaleMult)) return 13;
		if (!dense.SavePointCloud(out + "/cloud_views.ply", pc) || !dense.SavePointCloud(out + "/cloud_2views.ply", pc, true, 2)) return 14;
		if (dense.SavePointCloud(out + "/cloud_none.ply", MVS::DenseDepthMapsHIP::PointCloud())) return 15;
		printf("views %d, points %zu\n", n, pc.size());
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
