// sgm_rectify.hip -- the front of SemiGlobalMatcher::Match(scene, ...) for one image pair on the device: Image::StereoRectifyImages' two
// cv::warpPerspective calls with their validity masks (libs/MVS/Image.cpp:296-322) and the toGray(bNormalize, bSRGB) of both rectified images
// (libs/MVS/SemiGlobalMatcher.cpp:579-582) in one pass over the destination.  Included by sgm_engine.hip.
//
// The contract is the host code it replaces, bit for bit: openmvs_amd/rectify.py `warp_perspective_u8` (a float bilinear resample with constant
// border 0, rounded to 8 bits; the mask is the set of pixels whose centre maps inside the source) followed by openmvs_amd/sgm_pipeline.py
// `to_gray_linear` (the 256-entry sRGB -> linear table, built on the host with libm's powf and handed in, then 0.114 B + 0.587 G + 0.299 R).
// Coordinates are evaluated per pixel in double, summed left to right (the build has -ffp-contract=off): no incremental row sums.  Plain loads
// only -- no texture sampler, whose fixed-point weights would be another arithmetic.
#pragma once
#include <hip/hip_runtime.h>

struct SGMRectSide {
	const unsigned char* src; int W0, H0;       // source BGR image (each side has its own size)
	double Hi[9];                               // inverse homography: destination pixel -> source position
	unsigned char* bgr; float* gray; unsigned char* mask;   // w x h outputs
};
struct SGMRectPair { SGMRectSide s[2]; };

// block (64, 4): one wave covers 64 consecutive x of one row, so the three stores of a wave are contiguous and the four taps of neighbouring
// lanes share cache lines; grid (ceil(w / 64), ceil(h / 4), 2 sides)
__global__ void __launch_bounds__(256) sgm_rectify_pair_kernel(const SGMRectPair pair, int w, int h, const float* __restrict__ srgb2lin) {
	__shared__ float T[256];
	T[threadIdx.y * 64 + threadIdx.x] = srgb2lin[threadIdx.y * 64 + threadIdx.x];
	__syncthreads();
	const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
	if (x >= w || y >= h) return;
	const SGMRectSide& s = pair.s[blockIdx.z];
	const int W0 = s.W0, H0 = s.H0;
	const double xd = (double)x, yd = (double)y;
	const double Z = s.Hi[6] * xd + s.Hi[7] * yd + s.Hi[8];
	const double X = (s.Hi[0] * xd + s.Hi[1] * yd + s.Hi[2]) / Z, Y = (s.Hi[3] * xd + s.Hi[4] * yd + s.Hi[5]) / Z;
	int b = 0, g = 0, r = 0;
	if (X > -1.0 && Y > -1.0 && X < (double)W0 && Y < (double)H0) {       // at least one tap inside; false for a non-finite X or Y
		const double xf = floor(X), yf = floor(Y);
		const int x0 = (int)xf, y0 = (int)yf;
		const float fx = (float)(X - xf), fy = (float)(Y - yf), gx = 1.f - fx, gy = 1.f - fy;
		const bool xa = x0 >= 0, xb = x0 + 1 < W0, ya = y0 >= 0, yb = y0 + 1 < H0;
		const unsigned char* p0 = s.src + ((size_t)(ya ? y0 : 0) * W0 + (xa ? x0 : 0)) * 3;      // clamped addresses; a tap outside counts as 0
		const unsigned char* p1 = s.src + ((size_t)(ya ? y0 : 0) * W0 + (xb ? x0 + 1 : 0)) * 3;
		const unsigned char* p2 = s.src + ((size_t)(yb ? y0 + 1 : 0) * W0 + (xa ? x0 : 0)) * 3;
		const unsigned char* p3 = s.src + ((size_t)(yb ? y0 + 1 : 0) * W0 + (xb ? x0 + 1 : 0)) * 3;
		int o[3];
		for (int c = 0; c < 3; ++c) {
			const float t00 = (ya && xa) ? (float)p0[c] : 0.f, t01 = (ya && xb) ? (float)p1[c] : 0.f;
			const float t10 = (yb && xa) ? (float)p2[c] : 0.f, t11 = (yb && xb) ? (float)p3[c] : 0.f;
			float v = ((t00 * gx + t01 * fx) * gy) + ((t10 * gx + t11 * fx) * fy);
			v = floorf(v + 0.5f);
			o[c] = v < 0.f ? 0 : (v > 255.f ? 255 : (int)v);
		}
		b = o[0]; g = o[1]; r = o[2];
	}
	const size_t i = (size_t)y * w + x;
	s.bgr[i * 3] = (unsigned char)b; s.bgr[i * 3 + 1] = (unsigned char)g; s.bgr[i * 3 + 2] = (unsigned char)r;
	s.gray[i] = (0.114f * T[b] + 0.587f * T[g]) + 0.299f * T[r];
	s.mask[i] = (X >= 0.0 && Y >= 0.0 && X <= (double)W0 && Y <= (double)H0) ? 255 : 0;
}
