// sgm_post_oracle.cpp -- sequential CPU restatement of the tSGM steps around SemiGlobalMatcher::Match (libs/MVS/SemiGlobalMatcher.cpp in
// /root/reference): ConsistencyCrossCheck :1449-1489, FilterByCost :1491-1514, ExtractMask :1516-1573, FlipDirection :1628-1655,
// UpscaleMask :1657-1690, RefineDisparityMap :1693-1811.  *** TEST INFRASTRUCTURE ONLY ***  PARITY UNPINNED (no reference goldens; the
// reference does not build here).  Written as the reference writes them: raster loops with in-place overwrites; cos/sin through
// csrc/pm_math.h like the product (documented deviation from libm).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../openmvs_amd/csrc/pm_math.h"
#include "../openmvs_amd/csrc/sgm_post.h"   // sgmp_f2i / sgmp_addw only: the float -> int conversions the language leaves undefined, defined as x86 performs them

namespace {
const int16_t NO_DISP = 32767;
const uint8_t INVALID = 0, VALID = 255;
const int HW = 3;
typedef float real;
real o_cos(real x) { float s, c; pm_sincosf(x, &s, &c); return c; }
real o_sin(real x) { float s, c; pm_sincosf(x, &s, &c); return s; }
struct Fit {
	static real linear(real x) { return x / real(2); }
	static real poly4(real x) { return (x * x * x * x + x) / real(4); }
	static real parabola(real x) { return x / (x + real(1)); }
	static real sine(real x) { return real(0.5) * (o_sin((x - real(1)) * real(1.5707963267948966192313216916398)) + real(1)); }
	static real cosine(real x) { return (real(1) - o_cos(x * (real)(3.1415926535897932384626433832795 / 3.0))); }
	static real lcBlend(real x) { const real factor(real(1.195) - o_cos(x * (real)(3.1415926535897932384626433832795 / 2.3))); return cosine(x) * factor + linear(x) * (real(1) - factor); }
	static real semisubpixel(uint16_t primary, uint16_t other) { return real(0.5) * (static_cast<real>(primary) / static_cast<real>(other)); }
	static real subpixelMode(uint16_t prev, uint16_t center, uint16_t next, int mode) {
		if (prev == center) return center == next ? real(0) : semisubpixel(center, next);
		if (center == next) return prev == center ? real(0) : -semisubpixel(center, prev);
		const uint16_t ld(prev - center), rd(next - center);
		real x, mult;
		if (ld < rd) { x = static_cast<real>(ld) / static_cast<real>(rd); mult = real(1); }
		else { x = static_cast<real>(rd) / static_cast<real>(ld); mult = real(-1); }
		real value(0);
		switch (mode) { case 1: value = linear(x); break; case 2: value = poly4(x); break; case 3: value = parabola(x); break;
			case 4: value = sine(x); break; case 5: value = cosine(x); break; case 6: value = lcBlend(x); break; }
		return (value - real(0.5)) * mult;
	}
};
}

extern "C" {
struct OrcSgmPixel { unsigned long long idx; short minDisp, maxDisp; int pad; };

void orc_sgm_cross_check(int16_t* l2r, const int16_t* r2l, int wl, int h, int wr, int thCross) {
	for (int r = 0; r < h; ++r) for (int c = 0; c < wl; ++c) {
		int16_t& ld = l2r[(size_t)r * wl + c];
		if (ld == NO_DISP) continue;
		const int vx = c + ld;
		if (vx < 0 || vx >= wr) { ld = NO_DISP; continue; }
		const int16_t rd = r2l[(size_t)r * wr + vx];
		if (rd == NO_DISP) { ld = NO_DISP; continue; }
		if (abs(ld + rd) > thCross) ld = NO_DISP;
	}
}
void orc_sgm_filter_by_cost(int16_t* disp, const uint16_t* cost, int w, int h, uint16_t th) {
	for (size_t i = 0; i < (size_t)w * h; ++i) { if (disp[i] == NO_DISP) continue; if (cost[i] > th) disp[i] = NO_DISP; }
}
void orc_sgm_extract_mask(const int16_t* disp, uint8_t* mask, int w, int h, int thValid, int initValid) {
	if (initValid) memset(mask, VALID, (size_t)w * h);
	for (int r = 0; r < h; ++r) { int numValid = 0;
		for (int c = 0; c < w; ++c) { uint8_t& m = mask[(size_t)r * w + c]; if (m == INVALID) continue; m = INVALID; if (disp[(size_t)r * w + c] == NO_DISP) continue; if (++numValid >= thValid) break; } }
	for (int r = 0; r < h; ++r) { int numValid = 0;
		for (int c = w; --c >= 0; ) { uint8_t& m = mask[(size_t)r * w + c]; if (m == INVALID) continue; m = INVALID; if (disp[(size_t)r * w + c] == NO_DISP) continue; if (++numValid >= thValid) break; } }
}
void orc_sgm_upscale_mask(const uint8_t* mask, int w, int h, uint8_t* mask2x, int w2, int h2) {
	memset(mask2x, INVALID, (size_t)w2 * h2);
	for (int r = 0; r < h; ++r) for (int c = 0; c < w; ++c) {
		const int r2 = r * 2 + HW, c2 = c * 2 + HW; const uint8_t m = mask[(size_t)r * w + c];
		for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) { const int ux = c2 + j, uy = r2 + i; if (ux >= 0 && uy >= 0 && ux < w2 && uy < h2) mask2x[(size_t)uy * w2 + ux] = m; }
	}
}
void orc_sgm_flip_direction(const int16_t* l2r, int w, int h, int16_t* r2l) {
	for (size_t i = 0; i < (size_t)w * h; ++i) r2l[i] = NO_DISP;
	for (int r = 0; r < h; ++r) for (int c = 0; c < w; ++c) {
		const int16_t d = l2r[(size_t)r * w + c];
		if (d == NO_DISP) continue;
		for (int x = (c + d - 1 > 0 ? c + d - 1 : 0), xe = (c + d + 2 < w ? c + d + 2 : w); x < xe; ++x) r2l[(size_t)r * w + x] = (int16_t)-d;
	}
}
void orc_sgm_refine(int16_t* disp, const OrcSgmPixel* pixels, const uint16_t* accums, long nPix, int mode, int steps) {
	if (steps <= 1) return;
	if (mode == 0) { for (long i = 0; i < nPix; ++i) if (disp[i] != NO_DISP) disp[i] = (int16_t)(disp[i] * steps); return; }
	for (long idx = 0; idx < nPix; ++idx) {
		const OrcSgmPixel& pixel = pixels[idx];
		if (pixel.maxDisp - pixel.minDisp < 2) continue;
		int16_t& d = disp[idx];
		if (d == NO_DISP) continue;
		const uint16_t* acc = accums + pixel.idx;
		const int idxDisp = d - pixel.minDisp;
		real disparity((real)d);
		if (d == pixel.minDisp) disparity += Fit::semisubpixel(acc[idxDisp], acc[idxDisp + 1]);
		else if (d + 1 == pixel.maxDisp) disparity -= Fit::semisubpixel(acc[idxDisp], acc[idxDisp - 1]);
		else disparity += Fit::subpixelMode(acc[idxDisp - 1], acc[idxDisp], acc[idxDisp + 1], mode);
		d = (int16_t)sgmp_f2i(floorf(disparity * steps + .5f));
	}
}
} // extern "C"

// ---- Disparity2RangeMap (:1350-1444), Depth2DisparityMap (:1836-1860), Disparity2DepthMap (:1862-1923) -------------------------------
#include <algorithm>
namespace {
int getMedian(std::vector<int16_t>& v) {   // cList::GetMedian<Disparity>, libs/Common/List.h:668-678
	const size_t n = v.size();
	if (n % 2) { std::nth_element(v.begin(), v.begin() + (n >> 1), v.end()); return v[n >> 1]; }
	std::nth_element(v.begin(), v.begin() + (n >> 1), v.end());
	const int16_t nth = v[n >> 1];
	std::nth_element(v.begin(), v.begin() + (n >> 1) - 1, v.begin() + (n >> 1));
	const int16_t nth1 = v[(n >> 1) - 1];
	return (int16_t)(((int16_t)nth1 + (int16_t)nth) / (int16_t)2);
}
template <typename T> T getPixel(const T* img, int w, int h, int y, int x) { x = x < 0 ? 0 : (x >= w ? w - 1 : x); y = y < 0 ? 0 : (y >= h ? h - 1 : y); return img[(size_t)y * w + x]; }
template <typename T, typename F> bool sampleSafe(const T* img, int w, int h, float px, float py, F functor, float& v) {   // Types.inl:2315-2332
	const int lx = sgmp_f2i(px), ly = sgmp_f2i(py);
	const float x = px - lx, x1 = 1.f - x, y = py - ly, y1 = 1.f - y;
	const T x0y0 = getPixel(img, w, h, ly, lx), x1y0 = getPixel(img, w, h, ly, lx + 1), x0y1 = getPixel(img, w, h, ly + 1, lx), x1y1 = getPixel(img, w, h, ly + 1, lx + 1);
	const bool b00 = functor(x0y0), b10 = functor(x1y0), b01 = functor(x0y1), b11 = functor(x1y1);
	if (!b00 && !b10 && !b01 && !b11) return false;
	v = y1 * (x1 * (float)(b00 ? x0y0 : (b10 ? x1y0 : (b01 ? x0y1 : x1y1))) + x * (float)(b10 ? x1y0 : (b00 ? x0y0 : (b11 ? x1y1 : x0y1)))) +
	    y * (x1 * (float)(b01 ? x0y1 : (b11 ? x1y1 : (b00 ? x0y0 : x1y0))) + x * (float)(b11 ? x1y1 : (b01 ? x0y1 : (b10 ? x1y0 : x0y0))));
	return true;
}
void projectVertex(const double* H, const int* X, float* pt) {   // ProjectVertex_3x3_2_2, Util.inl:389-393
	const double z = H[6] * X[0] + H[7] * X[1] + H[8];
	const double invZ = z == 0 ? 1e+14 : 1.0 / z;
	pt[0] = (float)((H[0] * X[0] + H[1] * X[1] + H[2]) * invZ);
	pt[1] = (float)((H[3] * X[0] + H[4] * X[1] + H[5]) * invZ);
}
}
extern "C" {
unsigned long long orc_sgm_disparity2range_map(const int16_t* disparityMap, int cols, int rows, const uint8_t* maskMap, int w2, int h2,
		int minNumDisp, int minNumDispInvalid, OrcSgmPixel* imagePixels, int* outMaxNumDisp) {
	unsigned long long numCosts = 0;
	int maxNumDisp = 0;
	std::vector<int16_t> disps;
	for (int r = 0; r < rows; ++r) {
		const int r2 = (r == 0 ? 0 : r * 2 + HW);
		const int offset = r2 * w2;
		int c2e = HW;
		const uint8_t* pm = maskMap + (size_t)(r * 2 + HW) * w2 + HW;
		int c2 = 0;
		for (int c = 0; c < cols; ++c, pm += 2) {
			int16_t numDisp; int16_t rmin, rmax;
			if (*pm == INVALID) { rmin = rmax = NO_DISP; numDisp = 0; }
			else {
				const bool bInvalid = disparityMap[(size_t)r * cols + c] == NO_DISP;
				disps.clear();
				const int hw = bInvalid ? 20 : 3;
				for (int i = -hw; i <= hw; ++i) for (int j = -hw; j <= hw; ++j) {
					const int ux = c + j, uy = r + i;
					if (ux >= 0 && uy >= 0 && ux < cols && uy < rows) { const int16_t d = disparityMap[(size_t)uy * cols + ux]; if (d != NO_DISP) disps.push_back(d); }
				}
				if (disps.size() < 3) {
					const int16_t a = (int16_t)(cols * 2 / 3);
					rmax = a < (int16_t)minNumDispInvalid ? a : (int16_t)minNumDispInvalid; rmin = (int16_t)-rmax; numDisp = (int16_t)(rmax - rmin);
				} else {
					int16_t mn = *std::min_element(disps.begin(), disps.end()), mx = *std::max_element(disps.begin(), disps.end());
					const int16_t disp = (int16_t)(getMedian(disps) * 2);
					numDisp = (int16_t)((mx - mn) * 2);
					if (numDisp < minNumDisp) { numDisp = (int16_t)minNumDisp; rmin = (int16_t)(disp - numDisp / 2); rmax = (int16_t)(disp + (numDisp + 1) / 2); }
					else {
						const int16_t maxNum = bInvalid ? 64 : 32;
						if (numDisp > maxNum) {
							rmin = (int16_t)(disp - (maxNum * (disp - mn * 2) + 1) / numDisp);
							rmax = (int16_t)(disp + (maxNum * (mx * 2 + 1 - disp) + 1) / numDisp);
							numDisp = (int16_t)(rmax - rmin);
						} else { rmin = (int16_t)(disp - numDisp / 2); rmax = (int16_t)(disp + (numDisp + 1) / 2); }
					}
				}
				if (maxNumDisp < numDisp) maxNumDisp = numDisp;
			}
			c2e += 2;
			do { OrcSgmPixel& pixel = imagePixels[offset + c2]; pixel.minDisp = rmin; pixel.maxDisp = rmax; pixel.idx = numCosts; numCosts += numDisp; } while (++c2 < c2e);
		}
		do {
			const OrcSgmPixel& pixel = imagePixels[offset + c2e - 1];
			OrcSgmPixel& _pixel = imagePixels[offset + c2e];
			_pixel.minDisp = pixel.minDisp; _pixel.maxDisp = pixel.maxDisp; _pixel.idx = numCosts;
			numCosts += (int16_t)(pixel.maxDisp - pixel.minDisp);
		} while (++c2e < w2);
		const int _offsete = (r + 1 == rows ? h2 : r * 2 + HW + 2) * w2;
		for (int _offset = offset + w2; _offset < _offsete; _offset += w2) for (int cc = 0; cc < w2; ++cc) {
			const OrcSgmPixel& pixel = imagePixels[offset + cc];
			OrcSgmPixel& _pixel = imagePixels[_offset + cc];
			_pixel.minDisp = pixel.minDisp; _pixel.maxDisp = pixel.maxDisp; _pixel.idx = numCosts;
			numCosts += (int16_t)(pixel.maxDisp - pixel.minDisp);
		}
	}
	if (outMaxNumDisp) *outMaxNumDisp = maxNumDisp;
	return numCosts;
}
void orc_sgm_depth2disparity_map(const float* depthMap, int dw, int dh, const double* invH, const double* invQ, int subpixelSteps, int16_t* disparityMap, int w, int h) {
	for (int r = 0; r < h; ++r) for (int c = 0; c < w; ++c) {
		const int x[2] = {c + HW, r + HW}; float u[2];
		projectVertex(invH, x, u);
		float depth, disparity = 0;
		bool ok = sampleSafe(depthMap, dw, dh, u[0], u[1], [](float d) { return d > 0; }, depth);
		if (ok) {   // Image::Depth2Disparity, Image.cpp:425-433
			const double ww = (invQ[12] * u[0] + invQ[13] * u[1] + invQ[14]) * depth + invQ[15];
			if (fabs(ww) < 1e-7) ok = false;
			else { const double z = (invQ[8] * u[0] + invQ[9] * u[1] + invQ[10]) * depth + invQ[11]; disparity = -(float)(z / ww); }
		}
		disparityMap[(size_t)r * w + c] = ok ? (int16_t)sgmp_f2i(floorf(disparity * subpixelSteps + .5f)) : NO_DISP;
	}
}
void orc_sgm_disparity2depth_map(const int16_t* disparityMap, const uint16_t* costMap, int w, int h, const double* H, const double* Q, int subpixelSteps,
		float* depthMap, float* confMap, int dw, int dh) {
	for (int r = 0; r < dh; ++r) for (int c = 0; c < dw; ++c) {
		const int x[2] = {c, r}; float u[2];
		projectVertex(H, x, u);
		u[0] -= (float)HW; u[1] -= (float)HW;
		float disparity;
		const size_t i = (size_t)r * dw + c;
		if (!sampleSafe(disparityMap, w, h, u[0], u[1], [](int16_t d) { return d != NO_DISP; }, disparity)) { depthMap[i] = 0; if (costMap) confMap[i] = 0; continue; }
		float cost = 0;
		if (costMap) sampleSafe(costMap, w, h, u[0], u[1], [](uint16_t cc) { return cc != 65535; }, cost);
		const float d = disparity / subpixelSteps;
		const double ww = Q[12] * u[0] + Q[13] * u[1] - Q[14] * d + Q[15];   // TDisparity2Depth, Image.cpp:371-381
		float depth = 0;
		if (!(fabs(ww) < 1e-7)) { const double z = Q[8] * u[0] + Q[9] * u[1] - Q[10] * d + Q[11]; depth = (float)(z / ww); if (depth < 0.0001f) depth = 0; }
		depthMap[i] = depth;
		if (costMap) confMap[i] = 1.f / (cost + 1);
	}
}
} // extern "C"

// ---- ProjectDisparity2DepthMap (:1925-2039) and the per-pixel part of SemiGlobalMatcher::Fuse (:797-849) --------------------------------
namespace {
float disparity2depth(const double* Q, int ux, int uy, float d) {   // TDisparity2Depth(Q, ImageRef, d), Image.cpp:371-381
	const double w = Q[12] * ux + Q[13] * uy - Q[14] * d + Q[15];
	if (fabs(w) < 1e-7) return 0;
	const double z = Q[8] * ux + Q[9] * uy - Q[10] * d + Q[11];
	const float depth = (float)(z / w);
	return depth < 0.0001f ? 0.f : depth;
}
float disparity2depthPt(const double* Q, int ux, int uy, float d, float* pt) {   // :391-404
	const double w = Q[12] * ux + Q[13] * uy - Q[14] * d + Q[15];
	if (fabs(w) < 1e-7) return 0;
	const double z = (Q[8] * ux + Q[9] * uy - Q[10] * d + Q[11]) / w;
	if (z < 1e-7) return 0;
	const double nrm = 1.0 / (w * z);
	pt[0] = (float)((Q[0] * ux + Q[1] * uy - Q[2] * d + Q[3]) * nrm);
	pt[1] = (float)((Q[4] * ux + Q[5] * uy - Q[6] * d + Q[7]) * nrm);
	return (float)z;
}
}
extern "C" {
int orc_sgm_project_disparity2depth_map(const int16_t* disparityMap, const uint16_t* costMap, int w, int h, const double* Q, int subpixelSteps,
		float* depthMap, float* depthRangeMap, float* confMap, int dw, int dh) {
	const float overlapBorder = 0.5f + 0.25f;
	const size_t nd = (size_t)dw * dh;
	struct DD { std::vector<float> dist, depth, rx, ry, conf; } dd[4];
	for (auto& d : dd) { d.dist.assign(nd, 0); d.depth.assign(nd, 0); d.rx.assign(nd, 0); d.ry.assign(nd, 0); d.conf.assign(nd, 0); }
	for (int r = 0; r < h; ++r) for (int c = 0; c < w; ++c) {
		const int16_t disparityInt = disparityMap[(size_t)r * w + c];
		if (disparityInt == NO_DISP) continue;
		const float disparity = (float)disparityInt / subpixelSteps;
		float u[2] = {0, 0};
		const int dx[2] = {c + HW, r + HW};
		const float depth = disparity2depthPt(Q, dx[0], dx[1], disparity, u);
		if (depth <= 0) continue;
		const int16_t disparityCenter = (int16_t)sgmp_f2i(floorf(disparity));
		const float rangeX = disparity2depth(Q, dx[0], dx[1], (float)(disparityCenter - 1)), rangeY = disparity2depth(Q, dx[0], dx[1], (float)(disparityCenter + 1));
		const float cost = costMap ? 1.f / (costMap[(size_t)r * w + c] + 1) : 0.f;
		const int x[2] = {sgmp_f2i(floorf(u[0])), sgmp_f2i(floorf(u[1]))};
		u[0] -= 0.5f; u[1] -= 0.5f;
		for (int i = -1; i <= 1; ++i) for (int j = -1; j <= 1; ++j) {
			const int nx[2] = {sgmp_addw(x[0], j), sgmp_addw(x[1], i)};
			if (!(nx[0] >= 0 && nx[1] >= 0 && nx[0] < dw && nx[1] < dh)) continue;
			const float dist[2] = {(float)nx[0] - u[0], (float)nx[1] - u[1]};
			if (fabsf(dist[0]) > overlapBorder || fabsf(dist[1]) > overlapBorder) continue;
			const int idx = (dist[0] < 0 ? 1 : 0) + (dist[1] < 0 ? 2 : 0);
			DD& D = dd[idx];
			const float deistSq = dist[0] * dist[0] + dist[1] * dist[1];
			const size_t p = (size_t)nx[1] * dw + nx[0];
			if (D.depth[p] > 0 && D.dist[p] <= deistSq) continue;
			D.dist[p] = deistSq; D.depth[p] = depth; D.rx[p] = rangeX; D.ry[p] = rangeY; D.conf[p] = cost;
		}
	}
	const float thDist = 0.75f * 0.75f, thDepth = 0.02f;
	unsigned numDepths = 0;
	for (size_t p = 0; p < nd; ++p) {
		depthRangeMap[p * 2] = depthRangeMap[p * 2 + 1] = 0; if (confMap) confMap[p] = 0;      // (uninitialised in the reference where depth == 0)
		float distCenter = 3.402823466e+38f, depthCenter = 0;
		for (int i = 0; i < 4; ++i) { const float depth = dd[i].depth[p]; if (depth <= 0) continue; if (distCenter > dd[i].dist[p]) { distCenter = dd[i].dist[p]; depthCenter = depth; } }
		if (distCenter > thDist) { depthMap[p] = 0; continue; }
		float value[4] = {0, 0, 0, 0}, weight = 0;
		for (int i = 0; i < 4; ++i) {
			const float depth = dd[i].depth[p];
			if (depth <= 0 || !(fabsf(depthCenter - depth) / depthCenter < thDepth)) continue;
			const float wq = sqrtf(dd[i].dist[p]);
			const float v[4] = {depth, dd[i].rx[p], dd[i].ry[p], dd[i].conf[p]};
			for (int k = 0; k < 4; ++k) value[k] += v[k] * wq;
			weight += wq;
		}
		const float inv = 1.f / weight;
		depthMap[p] = value[0] * inv; depthRangeMap[p * 2] = value[1] * inv; depthRangeMap[p * 2 + 1] = value[2] * inv;
		if (confMap) confMap[p] = value[3] * inv;
		++numDepths;
	}
	return numDepths > 0 ? 1 : 0;
}

void orc_sgm_fuse_pairs(const float* const* depthMaps, const float* const* rangeMaps, const float* const* confMaps, int nPairs, int dw, int dh, unsigned minViews,
		float* depthMap, float* confMap) {
	struct Cluster { std::vector<int> views; float x, y; };
	for (size_t i = 0; i < (size_t)dw * dh; ++i) {
		std::vector<Cluster> clusters;
		for (int p = 0; p < nPairs; ++p) {
			const float depth = depthMaps[p][i];
			if (depth <= 0) continue;
			const float rx = rangeMaps[p][i * 2], ry = rangeMaps[p][i * 2 + 1];
			unsigned numClusters = 0;
			for (Cluster& cl : clusters) {
				if (!(cl.x <= depth && depth < cl.y)) continue;
				cl.views.push_back(p);
				if (cl.x < rx) cl.x = rx;
				if (cl.y > ry) cl.y = ry;
				++numClusters;
			}
			if (numClusters == 0) clusters.push_back(Cluster{{p}, rx, ry});
		}
		if (clusters.empty()) { depthMap[i] = 0; confMap[i] = 0; continue; }
		const Cluster& cluster = *std::max_element(clusters.begin(), clusters.end(), [](const Cluster& a, const Cluster& b) { return a.views.size() < b.views.size(); });
		if (cluster.views.size() < minViews) { depthMap[i] = 0; confMap[i] = 0; continue; }
		float depth = 0, conf = 0; unsigned numDepths = 0;
		for (int p : cluster.views) { depth += depthMaps[p][i]; conf += confMaps[p][i]; ++numDepths; }
		depth /= numDepths; conf /= numDepths;
		depthMap[i] = depth; confMap[i] = conf;
	}
}
} // extern "C"

// ---- cv::filterSpeckles for CV_16S (OpenCV calib3d/src/stereosgbm.cpp, filterSpecklesImpl; OpenCV is a dependency that is not vendored in the
// reference tree): the published algorithm restated -- scan in raster order, flood-fill every unlabelled pixel != newVal over 4-neighbours whose
// value differs by at most maxDiff from the pixel being expanded, and overwrite regions of at most maxSpeckleSize pixels with newVal.
extern "C" void orc_sgm_filter_speckles(int16_t* img, int w, int h, int16_t newVal, int maxSpeckleSize, int maxDiff) {
	std::vector<int> labels((size_t)w * h, 0);
	std::vector<unsigned char> rtype(1, 0);           // rtype[label] = 1: small region
	std::vector<int> ws;
	int curlabel = 0;
	for (int i = 0; i < h; ++i) for (int j = 0; j < w; ++j) {
		const size_t p0 = (size_t)i * w + j;
		if (img[p0] == newVal) continue;
		if (labels[p0]) { if (rtype[labels[p0]]) img[p0] = newVal; continue; }
		++curlabel; rtype.push_back(0);
		labels[p0] = curlabel;
		ws.clear(); ws.push_back((int)p0);
		int count = 0;
		while (!ws.empty()) {
			const int p = ws.back(); ws.pop_back();
			++count;
			const int x = p % w, y = p / w; const int dp = img[p];
			const int nb[4][2] = {{x, y + 1}, {x, y - 1}, {x + 1, y}, {x - 1, y}};
			for (const auto& q : nb) {
				if (q[0] < 0 || q[1] < 0 || q[0] >= w || q[1] >= h) continue;
				const size_t pq = (size_t)q[1] * w + q[0];
				if (labels[pq] || img[pq] == newVal || abs(dp - img[pq]) > maxDiff) continue;
				labels[pq] = curlabel; ws.push_back((int)pq);
			}
		}
		if (count <= maxSpeckleSize) { rtype[curlabel] = 1; img[p0] = newVal; }
	}
}
