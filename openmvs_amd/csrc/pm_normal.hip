// pm_normal.hip -- MVS::EstimateNormalMap (libs/MVS/DepthMap.cpp:1522-1613, the active least-squares branch) on the device: a normal map from a depth map alone.
//
//   pm_normal_map_kernel   one pixel per lane; the least-squares depth gradient over the depth-similar pixels of the 3 x 3 neighbourhood, back-projected through K
//
// Every result equals mvsf_estimate_normal_map (csrc/mvs_front.cpp) bit for bit: the same float and double expressions in the same order, no contraction
// (-ffp-contract=off), IEEE division and square root (float: -fhip-fp32-correctly-rounded-divide-sqrt; double: the compiler's expansions are correctly rounded).
// Plain loads and stores.  A lane owns its output pixel and reads only the depth map, which nothing writes during the launch, so there is nothing to synchronise.
// Layout: pixel i of the row-major map goes to lane i of the launch, so a wave reads three runs of 66 consecutive depths (256 B each, shared with its neighbours through
// L1 / L2) and stores 768 consecutive bytes, 12 per lane (one global_store_dwordx3: the normal map has no alignment beyond a float's, so a wider store per lane is not
// available for every view of a scene).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

struct PMNormal3 { float x, y, z; };

// The normal of pixel (c, r), or zeros: d <= 0 (or NaN, which is similar to nothing), fewer than three similar neighbours, or collinear ones (det == 0)
__device__ __forceinline__ PMNormal3 pm_normal_px(const float* __restrict__ depth, int w, int h, int c, int r, float k00, float k11, float k02, float k12) {
	PMNormal3 o = {0.f, 0.f, 0.f};
	const float d = depth[(size_t)r * w + c];
	if (d <= 0) return o;
	int sxx = 0, sxy = 0, syy = 0, count = 0;
	float gx = 0, gy = 0;
	#pragma unroll
	for (int y = -1; y <= 1; ++y) {
		#pragma unroll
		for (int x = -1; x <= 1; ++x) {
			if ((x == 0 && y == 0) || c + x < 0 || r + y < 0 || c + x >= w || r + y >= h) continue;
			const float di = depth[(size_t)(r + y) * w + (c + x)];
			if (!(di > 0 && fabsf(d - di) / d < 0.03f)) continue;          // IsDepthSimilar(d, di, 0.03f), libs/Common/Util.inl:797-809
			sxx += x * x; sxy += x * y; syy += y * y;
			gx += (di - d) * (float)x; gy += (di - d) * (float)y;
			++count;
		}
	}
	const int det = sxx * syy - sxy * sxy;
	if (count < 3 || det == 0) return o;
	const float inv = 1.f / (float)det;
	const float dx = ((float)syy * gx - (float)sxy * gy) * inv, dy = ((float)(-sxy) * gx + (float)sxx * gy) * inv;
	const float v0 = k00 * dx, v1 = k11 * dy, v2 = (k02 - (float)c) * dx + (k12 - (float)r) * dy - d;
	const double nv = __builtin_sqrt((double)v0 * v0 + (double)v1 * v1 + (double)v2 * v2);      // cv::normalize: v * (1 / |v|), norm and product in double
	const double a = nv ? 1. / nv : 0.;
	o.x = (float)(v0 * a); o.y = (float)(v1 * a); o.z = (float)(v2 * a);
	return o;
}

// normal[3 i ..] of every pixel i of the w x h map is written; the grid strides
__global__ __launch_bounds__(256) void pm_normal_map_kernel(const float* __restrict__ depth, float* __restrict__ normal, int w, int h, float k00, float k11, float k02, float k12) {
	const size_t n = (size_t)w * (size_t)h;
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
		const int r = (n >> 32) ? (int)(i / (size_t)w) : (int)((unsigned)i / (unsigned)w);   // (a 64-bit division only for maps that need one)
		const int c = (int)(i - (size_t)r * (size_t)w);
		*(PMNormal3*)(normal + i * 3) = pm_normal_px(depth, w, h, c, r, k00, k11, k02, k12);
	}
}
