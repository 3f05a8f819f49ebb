// Drives include/DenseDepthMapsHIP.hpp from decoded 8-bit images, the way a host without OpenMVS would: no gray image, no BGR image at the
// working resolution -- the engine's image store makes them (View::image8).
// Usage: stored_view_driver <scene.bin> <out.bin> [seed]
//   scene.bin: i32 n, W0, H0, nsrc, level, minRes, maxRes | per view: u8 rgb[W0*H0*3], f64 K[9] R[9] C[3] (at the working size), f32 dMin dMax, i32 neighbors[nsrc]
//   out.bin:   i32 w, h | per view f32 depth[w*h] normal[w*h*3] conf[w*h] | u64 nPoints | f32 points[3*nPoints] | u8 colors[3*nPoints]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "DenseDepthMapsHIP.hpp"

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
	int32_t hd[7]; if (fread(hd, 4, 7, f) != 7) return 4;
	const int n = hd[0], W0 = hd[1], H0 = hd[2], ns = hd[3];
	int w = 0, h = 0;
	MVS::DenseDepthMapsHIP::WorkingSize(W0, H0, (unsigned)hd[4], (unsigned)hd[5], (unsigned)hd[6], w, h);
	const size_t P0 = (size_t)W0 * H0, P = (size_t)w * h;
	std::vector<std::vector<unsigned char>> rgb((size_t)n, std::vector<unsigned char>(P0 * 3));
	std::vector<MVS::DenseDepthMapsHIP::View> views((size_t)n);
	for (int i = 0; i < n; ++i) {
		auto& v = views[(size_t)i];
		double cam[21]; float rng[2]; std::vector<int32_t> nb((size_t)ns);
		if (fread(rgb[(size_t)i].data(), 1, P0 * 3, f) != P0 * 3 || fread(cam, 8, 21, f) != 21 || fread(rng, 4, 2, f) != 2 || fread(nb.data(), 4, (size_t)ns, f) != (size_t)ns) return 4;
		v.image8 = rgb[(size_t)i].data(); v.W0 = W0; v.H0 = H0; v.channelOrder = 1; v.w = w; v.h = h;
		memcpy(v.K, cam, 72); memcpy(v.R, cam + 9, 72); memcpy(v.C, cam + 18, 24);
		v.dMin = rng[0]; v.dMax = rng[1]; v.neighbors = nb; v.ID = (uint32_t)i;
	}
	fclose(f);
	MVS::DenseDepthMapsHIP dense(0);
	if (!dense.IsValid()) { fprintf(stderr, "no device\n"); return 5; }
	MVS::DenseDepthMapsHIP::Options opt;
	opt.seed = argc > 3 ? (uint32_t)atoi(argv[3]) : 31u;
	opt.nSubResolutionLevels = 1; opt.nEstimationIters = 2; opt.nEstimationGeometricIters = 1; opt.nOptimize = 0;
	try {
		dense.LoadScene(views, w, h, opt);
		if (pmhip_image_bytes(dense.engine()) != 0) return 8;                    // every entry was dropped after its view adopted it
		dense.ComputeDepthMaps();
		MVS::DenseDepthMapsHIP::PointCloud pc;
		dense.FuseDepthMaps(pc);
		if (pc.colors.size() != pc.points.size()) return 9;                      // the colour images came from the store
		f = fopen(argv[2], "wb"); if (!f) return 6;
		const int32_t wh[2] = {w, h}; fwrite(wh, 4, 2, f);
		std::vector<float> d(P), nrm(P * 3), c(P);
		for (int i = 0; i < n; ++i) { dense.GetMaps(i, d.data(), nrm.data(), c.data()); fwrite(d.data(), 4, P, f); fwrite(nrm.data(), 4, P * 3, f); fwrite(c.data(), 4, P, f); }
		const uint64_t cnt = (uint64_t)pc.size();
		fwrite(&cnt, 8, 1, f); fwrite(pc.points.data(), 4, pc.points.size(), f); fwrite(pc.colors.data(), 1, pc.colors.size(), f);
		fclose(f);
		printf("depth maps %d at %d x %d, fused points %zu\n", n, w, h, pc.size());
	} catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return 7; }
	return 0;
}
