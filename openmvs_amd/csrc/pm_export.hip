// pm_export.hip -- the reference's image and PLY outputs made from what is resident on the device (host side: pm_host_export.hip).
//
//   pmex_hist_kernel / pmex_pick_kernel   ComputeX84Threshold<float,float> (libs/Common/Util.inl:1001-1024) with GetMinMax (libs/Common/List.h:700), exact: the element
//                                         at index n/2 of the sorted valid values, then the element at the same index of |v - median|, by a most-significant-digit radix
//                                         select over the 32-bit patterns (positive floats and +0 order like their patterns): four 8-bit digits, per digit one LDS histogram
//                                         per workgroup merged with global atomics, then one workgroup that picks the digit and the remaining rank.  Nothing crosses to the
//                                         host between the eight passes.
//   pmex_depth_image_kernel               DepthMap2Image (libs/MVS/DepthMap.cpp:1662-1690) with Pixel8U::gray2color (libs/Common/Types.inl:2222-2247; ALT is float for
//                                         Pixel8U, Types.h:1844) and TPixel<uint8_t>::set(float, float, float) (Types.h:1991)
//   pmex_normal_image_kernel              the pixel rule of ExportNormalMap (DepthMap.cpp:1700-1715)
//   pmex_conf_image_kernel                ExportConfidenceMap (DepthMap.cpp:1721-1749)
//   pmex_valid_flags / pmex_cloud_scatter MVS::ExportPointCloud (DepthMap.cpp:1753-1870): the valid pixels in row-major order as packed records, through the tile sums and the
//                                         tile scan of pm_fuse.hip
//   pmex_scale_kernel                     the per-point rule of PointCloud::SaveWithScale (libs/MVS/PointCloud.cpp:504-531) with Camera::GetFootprintWorld (Camera.h:458-471)
//
// Every result equals its numpy statement in openmvs_amd/mapexport.py bit for bit: the same float and double expressions in the same order, no contraction, IEEE
// division and square root.  MINF / MAXF are std::min / std::max (Types.h:312-315), written out here because a NaN operand decides by its position.
// Plain loads and stores; the only atomics are the histogram's and the first pass's count / min / max, all integer, so no result depends on an arrival order.
// What the reference leaves undefined is defined in include/pmhip_export.h.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "pm_fuse.hip"

#define PMEX_TB 256
#define PMEX_ITEMS 4                         // values (pixels) per thread and trip
#define PMEX_Q (PMEX_TB * PMEX_ITEMS)        // ... per workgroup and trip: the quantum pmhip_export_get_stats reports
#ifndef PMEX_MAX_BLOCKS
#define PMEX_MAX_BLOCKS 512                  // grid cap: a 1920 x 1080 map takes four trips
#endif
// the selection's state, 32-bit words in device memory
enum { PMEX_PREFIX = 0, PMEX_RANK, PMEX_COUNT, PMEX_MIN, PMEX_MAX, PMEX_MEDIAN, PMEX_MAD, PMEX_RMIN, PMEX_RMAX, PMEX_HIST = 16, PMEX_WORDS = PMEX_HIST + 256 };

__device__ __forceinline__ float pmex_minf(float a, float b) { return b < a ? b : a; }   // std::min(a, b)
__device__ __forceinline__ float pmex_maxf(float a, float b) { return a < b ? b : a; }   // std::max(a, b)

// The key of value v in selection `mode` (0: the value, 1: |v - median|), or false for a value that does not count (zeros, negatives, -0, NaN).  inf - inf has no order in
// the reference's nth_element; here it is one NaN pattern that ranks above +inf.
__device__ __forceinline__ bool pmex_key(float v, int mode, float median, uint32_t* key) {
	if (!(v > 0)) return false;
	if (mode == 0) { *key = __float_as_uint(v); return true; }
	const float a = fabsf(v - median);
	*key = a != a ? 0x7FC00000u : __float_as_uint(a);
	return true;
}

// Digit `pass` (0 = the highest eight bits) of every key that agrees with the digits picked so far goes into the histogram st[PMEX_HIST ..]; the first pass of the first
// selection also counts the valid values and takes their minimum and maximum.  Workgroup b takes values [b Q, (b + 1) Q) and strides by the grid.
__global__ __launch_bounds__(PMEX_TB) void pmex_hist_kernel(const float* __restrict__ v, size_t n, int mode, int pass, uint32_t* st) {
	__shared__ uint32_t h[256];
	__shared__ uint32_t red[3];
	const uint32_t t = threadIdx.x;
	h[t] = 0;
	if (t == 0) { red[0] = 0; red[1] = 0xFFFFFFFFu; red[2] = 0; }
	__syncthreads();
	const int shift = 24 - 8 * pass;
	const uint32_t hiMask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
	const uint32_t prefix = pass ? st[PMEX_PREFIX] & hiMask : 0u;
	const float median = __uint_as_float(st[PMEX_MEDIAN]);
	const bool first = mode == 0 && pass == 0;
	uint32_t cnt = 0, mn = 0xFFFFFFFFu, mx = 0;
	for (size_t base = (size_t)blockIdx.x * PMEX_Q; base < n; base += (size_t)gridDim.x * PMEX_Q) {
		#pragma unroll
		for (int k = 0; k < PMEX_ITEMS; ++k) {
			const size_t i = base + (size_t)k * PMEX_TB + t;
			uint32_t key;
			if (i >= n || !pmex_key(v[i], mode, median, &key) || (key & hiMask) != prefix) continue;
			atomicAdd(&h[(key >> shift) & 255u], 1u);
			if (first) { ++cnt; mn = key < mn ? key : mn; mx = key > mx ? key : mx; }
		}
	}
	if (first && cnt) { atomicAdd(&red[0], cnt); atomicMin(&red[1], mn); atomicMax(&red[2], mx); }
	__syncthreads();
	if (h[t]) atomicAdd(&st[PMEX_HIST + t], h[t]);
	if (first && t == 0 && red[0]) { atomicAdd(&st[PMEX_COUNT], red[0]); atomicMin(&st[PMEX_MIN], red[1]); atomicMax(&st[PMEX_MAX], red[2]); }
}

// One workgroup: the digit whose bin holds rank k (n / 2 at the first digit), the rank inside that bin, and the histogram cleared for the next pass.  After the last
// digit the pattern is the selected value.  n == 0: no bin holds a rank and nothing is written.
__global__ __launch_bounds__(256) void pmex_pick_kernel(int mode, int pass, uint32_t* st) {
	__shared__ uint32_t sc[256];
	const uint32_t t = threadIdx.x;
	const uint32_t c = st[PMEX_HIST + t];
	const uint32_t k = pass ? st[PMEX_RANK] : st[PMEX_COUNT] / 2u;
	const uint32_t prefix = pass ? st[PMEX_PREFIX] : 0u;
	sc[t] = c;
	__syncthreads();
	for (uint32_t off = 1; off < 256; off <<= 1) {
		const uint32_t a = t >= off ? sc[t - off] : 0u;
		__syncthreads();
		sc[t] += a;
		__syncthreads();
	}
	const uint32_t excl = sc[t] - c;
	st[PMEX_HIST + t] = 0;
	if (c && excl <= k && k - excl < c) {
		const uint32_t p = prefix | (t << (24 - 8 * pass));
		st[PMEX_PREFIX] = p; st[PMEX_RANK] = k - excl;
		if (pass == 3) st[mode ? PMEX_MAD : PMEX_MEDIAN] = p;
	}
}

// ---- images: a thread makes four consecutive pixels and stores them as whole words (the image buffers are the engine's own, rounded up to four pixels) ----------------
// Pixel8U::gray2color, every step in float
__device__ __forceinline__ float pmex_interpolate(float val, float y0, float x0, float y1, float x1) { return (val - x0) * (y1 - y0) / (x1 - x0) + y0; }
__device__ __forceinline__ float pmex_base(float val) {
	if (val <= 0.125f) return 0.f;
	if (val <= 0.375f) return pmex_interpolate(2.f * val - 1.f, 0.f, -0.75f, 1.f, -0.25f);
	if (val <= 0.625f) return 1.f;
	if (val <= 0.87f) return pmex_interpolate(2.f * val - 1.f, 1.f, 0.25f, 0.f, 0.75f);
	return 0.f;                                                              // (a NaN gray -- 0 * inf when minDepth == maxDepth -- fails every test above: black)
}
// r | g << 8 | b << 16 of one depth
__device__ __forceinline__ uint32_t pmex_depth_rgb(float depth, float maxDepth, float sclDepth) {
	if (!(depth > 0)) return 0u;
	const float gray = pmex_minf(pmex_maxf((maxDepth - depth) * sclDepth, 0.f), 1.f);         // CLAMP = MINF(MAXF(v, l0), l1), Types.h:1198
	return (uint32_t)pmfu_toU8(pmex_base(gray + 0.25f) * 255.f) | (uint32_t)pmfu_toU8(pmex_base(gray) * 255.f) << 8 | (uint32_t)pmfu_toU8(pmex_base(gray - 0.25f) * 255.f) << 16;
}
__device__ __forceinline__ uint32_t pmex_normal_rgb(float x, float y, float z) {
	if (fabsf(x) < 0.0001f && fabsf(y) < 0.0001f && fabsf(z) < 0.0001f) return 0u;           // ISZERO(Point3f): FZERO_TOLERANCE per component (Types.h:579, :1222, Types.inl:540)
	return (uint32_t)pmfu_toU8((1.f - x) * 127.5f) | (uint32_t)pmfu_toU8((1.f - y) * 127.5f) << 8 | (uint32_t)pmfu_toU8(-z * 255.0f) << 16;
}
// four pixels' r | g << 8 | b << 16 into twelve bytes
__device__ __forceinline__ void pmex_store_rgb4(uint32_t* out, size_t q, const uint32_t c[4]) {
	out[q * 3] = c[0] | c[1] << 24; out[q * 3 + 1] = c[1] >> 8 | c[2] << 16; out[q * 3 + 2] = c[2] >> 16 | c[3] << 8;
}

// The range DepthMap2Image finds (auto != 0; from the selection's state) or was given; (FLT_MAX, 0) stays when no depth is valid.  Written to st for the host.
__global__ __launch_bounds__(PMEX_TB) void pmex_depth_image_kernel(const float* __restrict__ depth, size_t n, int autoRange, float minDepth, float maxDepth, uint32_t* st, uint32_t* __restrict__ rgb) {
	if (autoRange && st[PMEX_COUNT]) {
		const float med = __uint_as_float(st[PMEX_MEDIAN]), th = 5.2f * __uint_as_float(st[PMEX_MAD]);
		maxDepth = pmex_minf(med + th, __uint_as_float(st[PMEX_MAX]));
		minDepth = pmex_maxf(med - th, __uint_as_float(st[PMEX_MIN]));
	}
	const float sclDepth = 1.f / (maxDepth - minDepth);
	const size_t nq = (n + 3) / 4;
	for (size_t q = (size_t)blockIdx.x * PMEX_TB + threadIdx.x; q < nq; q += (size_t)gridDim.x * PMEX_TB) {
		uint32_t c[4];
		#pragma unroll
		for (int k = 0; k < 4; ++k) c[k] = q * 4 + k < n ? pmex_depth_rgb(depth[q * 4 + k], maxDepth, sclDepth) : 0u;
		pmex_store_rgb4(rgb, q, c);
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) { st[PMEX_RMIN] = __float_as_uint(minDepth); st[PMEX_RMAX] = __float_as_uint(maxDepth); }
}

__global__ __launch_bounds__(PMEX_TB) void pmex_normal_image_kernel(const float* __restrict__ normal, size_t n, uint32_t* __restrict__ rgb) {
	const size_t nq = (n + 3) / 4;
	for (size_t q = (size_t)blockIdx.x * PMEX_TB + threadIdx.x; q < nq; q += (size_t)gridDim.x * PMEX_TB) {
		uint32_t c[4];
		#pragma unroll
		for (int k = 0; k < 4; ++k) { const size_t i = q * 4 + k; c[k] = i < n ? pmex_normal_rgb(normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]) : 0u; }
		pmex_store_rgb4(rgb, q, c);
	}
}

// ExportConfidenceMap's range from the selection's state, and (uint8_t)CLAMP((conf - minConf) * 255.f / deltaConf, 0.f, 255.f).  A NaN (0 / 0 when deltaConf == 0) has no
// conversion in the reference; here it is 0.
__global__ __launch_bounds__(PMEX_TB) void pmex_conf_image_kernel(const float* __restrict__ conf, size_t n, uint32_t* st, uint32_t* __restrict__ gray) {
	const float med = __uint_as_float(st[PMEX_MEDIAN]), th = 5.2f * __uint_as_float(st[PMEX_MAD]);
	float minConf = med - th, maxConf = med + th;
	if (minConf < 0.1f) minConf = 0.1f;
	if (maxConf < 0.1f) maxConf = 30.f;
	const float deltaConf = maxConf - minConf;
	const size_t nq = (n + 3) / 4;
	for (size_t q = (size_t)blockIdx.x * PMEX_TB + threadIdx.x; q < nq; q += (size_t)gridDim.x * PMEX_TB) {
		uint32_t word = 0;
		#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const size_t i = q * 4 + k;
			const float c = i < n ? conf[i] : 0.f;
			if (!(c > 0)) continue;
			const float s = pmex_minf(pmex_maxf((c - minConf) * 255.f / deltaConf, 0.f), 255.f);
			word |= (s != s ? 0u : (uint32_t)(int)s) << (8 * k);
		}
		gray[q] = word;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) { st[PMEX_RMIN] = __float_as_uint(minConf); st[PMEX_RMAX] = __float_as_uint(maxConf); }
}

// ---- the cloud of one view ---------------------------------------------------------------------------------------------------------------------------------------------
// recN[p] = 1 for a valid pixel (depth > 0, DepthMap.cpp:1795 / :1851), the input of pmfu_tile_sums
__global__ __launch_bounds__(256) void pmex_valid_flags(const float* __restrict__ depth, uint32_t P, uint8_t* __restrict__ recN) {
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < P; p += gridDim.x * 256u) recN[p] = depth[p] > 0 ? 1 : 0;
}

// One workgroup per scan tile (PMFU_TILE pixels, as pmfu_tile_sums counted them), four rounds of one pixel per lane: a valid pixel's record goes to
// tileOff[tile].x + (valid pixels before it in the tile), which is its rank in row-major order.  Records are the reference's packed Vertex structs: x y z [nx ny nz] r g b,
// 15 or 27 bytes.  X = (float) TransformPointI2W(Point3(i, j, depth)) in double (pmfu_I2W), N = R^T n (pmfu_normalW), the colour is the view's resident BGR image at the
// same pixel -- the resident image has the map's size, so the ROUND2INT(scaleImage * i) lookup of the branch without normals (DepthMap.cpp:1790, :1799) is the identity --
// or white.
__global__ __launch_bounds__(PMFU_TB) void pmex_cloud_scatter(const float* __restrict__ depth, const float* __restrict__ normal, const uint8_t* __restrict__ bgr, uint32_t P, uint32_t w,
                                                               PMFuseCam cam, const uint2* __restrict__ tileOff, uint8_t* __restrict__ rec) {
	__shared__ uint32_t waveCount[PMFU_TB / 64];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t recBytes = normal ? 27u : 15u;
	uint32_t base = tileOff[blockIdx.x].x;
	for (uint32_t r = 0; r < PMFU_TILE / PMFU_TB; ++r) {
		const uint32_t p = blockIdx.x * PMFU_TILE + r * PMFU_TB + t;
		const float d = p < P ? depth[p] : 0.f;
		const bool valid = d > 0;
		const unsigned long long m = __ballot(valid);
		if (lane == 0) waveCount[wave] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, total = 0;
		for (uint32_t k = 0; k < PMFU_TB / 64; ++k) { const uint32_t c = waveCount[k]; before += k < wave ? c : 0u; total += c; }
		__syncthreads();
		if (valid) {
			const uint32_t i = p % w, j = p / w;
			double X[3]; pmfu_I2W(cam, (double)i, (double)j, (double)d, X);
			float o[6] = {(float)X[0], (float)X[1], (float)X[2], 0.f, 0.f, 0.f};
			if (normal) pmfu_normalW(cam, normal + (size_t)p * 3, o + 3);
			uint8_t* out = rec + (size_t)(base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) * recBytes;
			__builtin_memcpy(out, o, normal ? 24 : 12);
			out += normal ? 24 : 12;
			out[0] = bgr ? bgr[(size_t)p * 3 + 2] : (uint8_t)255; out[1] = bgr ? bgr[(size_t)p * 3 + 1] : (uint8_t)255; out[2] = bgr ? bgr[(size_t)p * 3] : (uint8_t)255;
		}
		base += total;
	}
}

// ---- PointCloud::SaveWithScale, one thread per point ---------------------------------------------------------------------------------------------------------------------
// Camera::GetFootprintWorld(TPoint3<double>): camX = R (X - C) (cv::Matx product: sums from 0, left to right), x = (camX.x / camX.z, camX.y / camX.z), and
// camX.z / sqrt(f^2 + |x - principal point|^2) -- TransformPointI2V on the normalised point, as the reference has it
__device__ __forceinline__ double pmex_footprint(const PMFuseCam& c, const float* p) {
	const double d0 = (double)p[0] - c.C[0], d1 = (double)p[1] - c.C[1], d2 = (double)p[2] - c.C[2];
	const double cx = ((0.0 + c.R[0] * d0) + c.R[1] * d1) + c.R[2] * d2;
	const double cy = ((0.0 + c.R[3] * d0) + c.R[4] * d1) + c.R[5] * d2;
	const double cz = ((0.0 + c.R[6] * d0) + c.R[7] * d1) + c.R[8] * d2;
	const double vx = cx / cz - c.K[2], vy = cy / cz - c.K[5];
	return cz / __builtin_sqrt(c.K[0] * c.K[0] + (vx * vx + vy * vy));
}
// weights == null: the smallest scale and the number of views; otherwise the scale whose scale / weight is smallest (the first on a tie: the test is a strict >) with
// that weight.  A view behind the point gives the negative scale the arithmetic gives (the reference only asserts).
__global__ __launch_bounds__(256) void pmex_scale_kernel(const float* __restrict__ points, const uint32_t* __restrict__ viewStart, const uint32_t* __restrict__ views, const float* __restrict__ weights,
                                                          const PMFuseCam* __restrict__ cams, uint32_t n, float scaleMult, float* __restrict__ outScale, float* __restrict__ outConf) {
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const uint32_t a = viewStart[i], b = viewStart[i + 1];
		float best = FLT_MAX, conf = weights ? 0.f : (float)(b - a), bestRatio = FLT_MAX;
		for (uint32_t v = a; v < b; ++v) {
			const float scale = (float)pmex_footprint(cams[views[v]], points + (size_t)i * 3);
			if (!weights) { if (best > scale) best = scale; continue; }
			const float cw = weights[v], ratio = scale / cw;
			if (bestRatio > ratio) { bestRatio = ratio; best = scale; conf = cw; }
		}
		outScale[i] = best * scaleMult; outConf[i] = conf;
	}
}
