// seed_raster.hip -- TriangulatePoints2DepthMap's rasteriser (libs/MVS/DepthMap.cpp:1117-1251) on the device: the rough depth (and normal) map that seeds PatchMatch and
// SGM, made from the small mesh of an image's sparse points.  Included by pm_engine.hip and sgm_engine.hip; the Delaunay triangulation, the vertex normals and the corner
// depths of bAddCorners stay on the host (a few thousand points), so what crosses to the device is the mesh and never a map.
//
//   seed_face_kernel      one face per lane: the reject, the box, the area; a box of at most `boxMax` pixels is walked by the lane, a larger one is appended to the list
//   seed_large_kernel     SEED_LARGE_SPLIT workgroups per listed face (grid.y), their lanes striding over the box together
//   seed_point_kernel     one vertex per lane: the 2x2 block at floor(projection)
//   seed_resolve_kernel   one pixel per lane: depth and normal recomputed from the winning face or vertex
//
// The reference walks the faces (the vertices) in index order and every covered pixel is overwritten: a pixel ends with the values of the HIGHEST index that covers it.
// Pass 1 writes that winner into a 32-bit key map cleared to 0 with atomicMax(key, index + 1) -- whatever order the lanes run in, and whichever of the two face routes
// takes a face; pass 2 recomputes the winner's values with the float and double expressions of TImage::RasterizeTriangleBary, EdgeFunction, the perspective-correct
// barycentrics and the RasterDepth functor in the reference's order (no contraction, IEEE division: the build flags).  Both passes call seed_setup / seed_pixel, so a
// pixel pass 1 found covered is covered in pass 2.  Plain loads, stores and atomicMax only: the wave64 emulator build of the tests runs this source.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include "hip_buf.h"

#define SEED_MODE_POINTS 0       // bInitSparse: every vertex on the 2x2 block around its projection
#define SEED_MODE_FACES 1        // the faces rasterised
#ifndef SEED_BOX_PIXELS
#define SEED_BOX_PIXELS 64       // a face whose clipped box holds more pixels goes to the workgroup route (the threshold of pm_mesh.hip; the maps never depend on it)
#endif
#define SEED_MAX_BLOCKS 16384    // grid.x of the strided kernels
#define SEED_LARGE_BLOCKS 2048   // workgroups (grid.x) that share the listed faces
#define SEED_LARGE_SPLIT 8       // ... each face's box cut among this many workgroups (grid.y): with the image corners four faces cover most of the image

struct SeedTri { float x[3], y[3], z[3], inv; int x0, y0, x1, y1; };

// EdgeFunction(a, b, c), libs/Common/Util.inl:602-604: (c - a).cross(b - a) -- the differences in float, the cross product in double (cv::Point_::cross), narrowed once
__device__ __forceinline__ float seed_edge(float ax, float ay, float bx, float by, float cx, float cy) {
	return (float)((double)(cx - ax) * (double)(by - ay) - (double)(cy - ay) * (double)(bx - ax));
}

// RasterizeTriangleBary up to its pixel loop for face f: false = nothing is drawn (the box misses the image, or area <= 0)
__device__ __forceinline__ bool seed_setup(const float* __restrict__ proj, const float* __restrict__ z, const uint32_t* __restrict__ faces, size_t f, int w, int h, SeedTri& t) {
	for (int k = 0; k < 3; ++k) { const size_t v = faces[3 * f + k]; t.x[k] = proj[2 * v]; t.y[k] = proj[2 * v + 1]; t.z[k] = z[v]; }
	const float mnx = fminf(fminf(t.x[0], t.x[1]), t.x[2]), mxx = fmaxf(fmaxf(t.x[0], t.x[1]), t.x[2]);
	const float mny = fminf(fminf(t.y[0], t.y[1]), t.y[2]), mxy = fmaxf(fmaxf(t.y[0], t.y[1]), t.y[2]);
	if (mxx < 0.f || mnx > (float)(w - 1) || mxy < 0.f || mny > (float)(h - 1)) return false;
	t.x0 = max((int)floorf(mnx), 0); t.y0 = max((int)floorf(mny), 0); t.x1 = min((int)ceilf(mxx), w - 1); t.y1 = min((int)ceilf(mxy), h - 1);
	const float area = seed_edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
	if (area <= 0.f) return false;
	t.inv = 1.f / area;
	return true;
}

// whether the centre of (px, py) is inside: the three barycentrics, each dropped when < 0
__device__ __forceinline__ bool seed_inside(const SeedTri& t, int px, int py, float b[3]) {
	const float fx = (float)px, fy = (float)py;
	b[0] = seed_edge(t.x[1], t.y[1], t.x[2], t.y[2], fx, fy) * t.inv;
	if (b[0] < 0.f) return false;
	b[1] = seed_edge(t.x[2], t.y[2], t.x[0], t.y[0], fx, fy) * t.inv;
	if (b[1] < 0.f) return false;
	b[2] = seed_edge(t.x[0], t.y[0], t.x[1], t.y[1], fx, fy) * t.inv;
	return !(b[2] < 0.f);
}

// ... and its values: the perspective-correct barycentrics (Util.inl:746-749; TPoint3 / scalar multiplies by the reciprocal) and the RasterDepth functor's depth
__device__ __forceinline__ bool seed_pixel(const SeedTri& t, int px, int py, float pb[3], float& depth) {
	float b[3];
	if (!seed_inside(t, px, py, b)) return false;
	const float p0 = b[0] * t.z[1] * t.z[2], p1 = b[1] * t.z[0] * t.z[2], p2 = b[2] * t.z[0] * t.z[1];
	const float invd = 1.f / ((p0 + p1) + p2);
	pb[0] = p0 * invd; pb[1] = p1 * invd; pb[2] = p2 * invd;
	depth = (pb[0] * t.z[0] + pb[1] * t.z[1]) + pb[2] * t.z[2];
	return true;
}

__device__ __forceinline__ void seed_offer(uint32_t* __restrict__ keys, const SeedTri& t, int w, int px, int py, uint32_t f) {
	float b[3];
	if (seed_inside(t, px, py, b)) atomicMax(keys + ((size_t)py * w + px), f + 1u);
}

// large[0]: the number of listed faces, large[1 ...]: the list
__global__ __launch_bounds__(256) void seed_face_kernel(const float* __restrict__ proj, const float* __restrict__ z, const uint32_t* __restrict__ faces, uint32_t nFaces, int w, int h,
		int boxMax, uint32_t* __restrict__ keys, uint32_t* __restrict__ large) {
	for (size_t f = (size_t)blockIdx.x * 256u + threadIdx.x; f < nFaces; f += (size_t)gridDim.x * 256u) {
		SeedTri t;
		if (!seed_setup(proj, z, faces, f, w, h, t)) continue;
		if ((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > boxMax) {                  // (an image has at most INT_MAX pixels: seedCheck)
			large[1u + atomicAdd(large, 1u)] = (uint32_t)f;
			continue;
		}
		for (int y = t.y0; y <= t.y1; ++y) for (int x = t.x0; x <= t.x1; ++x) seed_offer(keys, t, w, x, y, (uint32_t)f);
	}
}

__global__ __launch_bounds__(256) void seed_large_kernel(const float* __restrict__ proj, const float* __restrict__ z, const uint32_t* __restrict__ faces, int w, int h,
		uint32_t* __restrict__ keys, const uint32_t* __restrict__ large) {
	const uint32_t n = large[0];
	for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
		const uint32_t f = large[1u + e];
		SeedTri t;
		if (!seed_setup(proj, z, faces, f, w, h, t)) continue;               // (listed faces passed this already)
		const int bw = t.x1 - t.x0 + 1;
		const int np = bw * (t.y1 - t.y0 + 1);
		for (long long p = (long long)blockIdx.y * 256 + threadIdx.x; p < np; p += 256ll * gridDim.y) {
			const int y = (int)(p / bw);
			seed_offer(keys, t, w, t.x0 + ((int)p - y * bw), t.y0 + y, f);
		}
	}
}

// DepthMap.cpp:1139-1153: vertex i on the pixels floor(proj[i]) + {0,1}^2 that lie inside the image (the coordinates' floors fit an int: seedCheck)
__global__ __launch_bounds__(256) void seed_point_kernel(const float* __restrict__ proj, uint32_t nVerts, int w, int h, uint32_t* __restrict__ keys) {
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nVerts; i += (size_t)gridDim.x * 256u) {
		const long long x = (long long)floorf(proj[2 * i]), y = (long long)floorf(proj[2 * i + 1]);
		for (int d = 0; d < 4; ++d) {
			const long long ax = x + (d & 1), ay = y + (d >> 1);
			if (ax >= 0 && ax < w && ay >= 0 && ay < h) atomicMax(keys + ((size_t)ay * w + (size_t)ax), (uint32_t)i + 1u);
		}
	}
}

// normal == nullptr: depth only
__global__ __launch_bounds__(256) void seed_resolve_kernel(int mode, const float* __restrict__ proj, const float* __restrict__ z, const float* __restrict__ vnormals,
		const uint32_t* __restrict__ faces, int w, int h, const uint32_t* __restrict__ keys, float* __restrict__ depth, float* __restrict__ normal) {
	const size_t n = (size_t)w * (size_t)h;
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
		const uint32_t key = keys[i];
		float d = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f;
		if (key && mode == SEED_MODE_POINTS) {
			const size_t v = key - 1u;
			d = z[v];
			if (normal) { o0 = vnormals[3 * v]; o1 = vnormals[3 * v + 1]; o2 = vnormals[3 * v + 2]; }
		} else if (key) {
			const size_t f = key - 1u;
			const int py = (int)((unsigned)i / (unsigned)w), px = (int)i - py * w;
			SeedTri t; float pb[3];
			if (seed_setup(proj, z, faces, f, w, h, t) && seed_pixel(t, px, py, pb, d) && normal) {
				const float* n0 = vnormals + 3 * (size_t)faces[3 * f]; const float* n1 = vnormals + 3 * (size_t)faces[3 * f + 1]; const float* n2 = vnormals + 3 * (size_t)faces[3 * f + 2];
				const float a0 = (n0[0] * pb[0] + n1[0] * pb[1]) + n2[0] * pb[2], a1 = (n0[1] * pb[0] + n1[1] * pb[1]) + n2[1] * pb[2], a2 = (n0[2] * pb[0] + n1[2] * pb[1]) + n2[2] * pb[2];
				const double nv = __builtin_sqrt(((double)a0 * a0 + (double)a1 * a1) + (double)a2 * a2);        // cv::normalize: v * (1 / |v|), norm and product in double
				const double s = nv ? 1. / nv : 0.;
				o0 = (float)(a0 * s); o1 = (float)(a1 * s); o2 = (float)(a2 * s);
			}
		}
		depth[i] = d;
		if (normal) { normal[3 * i] = o0; normal[3 * i + 1] = o1; normal[3 * i + 2] = o2; }
	}
}

// ---- host side, shared by the two engines --------------------------------------------------------------------------------------------------------------------------

// the resident mesh of the last call and the working buffers (grow only); the tuning and the statistics of the last call
struct SeedWork {
	DevBuf<float> proj, z, normals; DevBuf<uint32_t> faces, keys, large;
	int boxMax = SEED_BOX_PIXELS;
	uint64_t statLarge = 0, statUs = 0, statBytes = 0;
	hipEvent_t ev[2] = {nullptr, nullptr};                  // bracket the clears and kernels of a call
	void free() { for (hipEvent_t& e : ev) { if (e) hipEventDestroy(e); e = nullptr; } const int box = boxMax; *this = SeedWork{}; boxMax = box; }
};

// What a call checks before anything is uploaded: empty = fine, else the reason.  `who` names the entry point.
static std::string seedCheck(const char* who, int mode, int w, int h, const float* proj, const float* z, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces) {
	const std::string p = std::string(who) + ": ";
	if (mode != SEED_MODE_POINTS && mode != SEED_MODE_FACES) return p + "mode " + std::to_string(mode) + " is neither points (0) nor faces (1)";
	if (w < 1 || h < 1) return p + "a map of " + std::to_string(w) + " x " + std::to_string(h);
	if ((uint64_t)w * (uint64_t)h > (uint64_t)INT_MAX) return p + std::to_string(w) + " x " + std::to_string(h) + " is more than INT_MAX pixels";
	if (nVerts && (!proj || !z)) return p + "no projections or depths for " + std::to_string(nVerts) + " vertices";
	if (mode == SEED_MODE_FACES && nFaces && !faces) return p + "no indices for " + std::to_string(nFaces) + " faces";
	if (nVerts == UINT32_MAX || nFaces == UINT32_MAX) return p + "too many vertices or faces for a 32-bit key";
	for (size_t i = 0; i < nVerts; ++i) {
		const float x = proj[2 * i], y = proj[2 * i + 1], d = z[i];
		if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(d)) return p + "vertex " + std::to_string(i) + " is not finite";
		if (!(d > 0.f)) return p + "vertex " + std::to_string(i) + " has depth " + std::to_string(d) + " (the reference asserts z > 0)";
		if (!(x >= -2147483648.f && x < 2147483648.f && y >= -2147483648.f && y < 2147483648.f)) return p + "vertex " + std::to_string(i) + " projects outside the range of int";
	}
	if (mode == SEED_MODE_FACES)
		for (size_t k = 0; k < 3 * (size_t)nFaces; ++k)
			if (faces[k] >= nVerts) return p + "face " + std::to_string(k / 3) + " names vertex " + std::to_string(faces[k]) + " of " + std::to_string(nVerts);
	return std::string();
}

// The maps of a checked mesh into dDepth (w * h) and, with vertex normals and dNormal, dNormal (3 * w * h), both on the device.  Leaves the stream running with ev[1]
// recorded behind the last kernel; the host arrays are pageable and have been consumed on return.
static hipError_t seedRun(SeedWork& s, hipStream_t st, int mode, int w, int h, const float* proj, const float* z, const float* normals, uint32_t nVerts,
		const uint32_t* faces, uint32_t nFaces, float* dDepth, float* dNormal) {
	hipError_t r;
	const size_t P = (size_t)w * h;
	if (!normals) dNormal = nullptr;
	for (hipEvent_t& e : s.ev) if (!e && (r = hipEventCreate(&e)) != hipSuccess) return r;
	s.statLarge = s.statUs = s.statBytes = 0;
	const bool empty = nVerts == 0 || (mode == SEED_MODE_FACES && nFaces == 0);
	if (!empty) {
		if ((r = s.proj.reserve(2 * (size_t)nVerts)) != hipSuccess || (r = s.z.reserve(nVerts)) != hipSuccess || (r = s.keys.reserve(P)) != hipSuccess) return r;
		if ((r = hipMemcpyAsync(s.proj, proj, sizeof(float) * 2 * nVerts, hipMemcpyHostToDevice, st)) != hipSuccess) return r;
		if ((r = hipMemcpyAsync(s.z, z, sizeof(float) * nVerts, hipMemcpyHostToDevice, st)) != hipSuccess) return r;
		s.statBytes = sizeof(float) * 3 * (uint64_t)nVerts;
		if (dNormal) {
			if ((r = s.normals.reserve(3 * (size_t)nVerts)) != hipSuccess) return r;
			if ((r = hipMemcpyAsync(s.normals, normals, sizeof(float) * 3 * nVerts, hipMemcpyHostToDevice, st)) != hipSuccess) return r;
			s.statBytes += sizeof(float) * 3 * (uint64_t)nVerts;
		}
		if (mode == SEED_MODE_FACES) {
			if ((r = s.faces.reserve(3 * (size_t)nFaces)) != hipSuccess || (r = s.large.reserve(1 + (size_t)nFaces)) != hipSuccess) return r;
			if ((r = hipMemcpyAsync(s.faces, faces, sizeof(uint32_t) * 3 * nFaces, hipMemcpyHostToDevice, st)) != hipSuccess) return r;
			s.statBytes += sizeof(uint32_t) * 3 * (uint64_t)nFaces;
		}
		if ((r = hipStreamSynchronize(st)) != hipSuccess) return r;            // (the host arrays are pageable and the caller's)
	}
	if ((r = hipEventRecord(s.ev[0], st)) != hipSuccess) return r;
	if (empty) {
		if ((r = hipMemsetAsync(dDepth, 0, sizeof(float) * P, st)) != hipSuccess) return r;
		if (dNormal && (r = hipMemsetAsync(dNormal, 0, sizeof(float) * 3 * P, st)) != hipSuccess) return r;
		return hipEventRecord(s.ev[1], st);
	}
	if ((r = hipMemsetAsync(s.keys, 0, sizeof(uint32_t) * P, st)) != hipSuccess) return r;
	if (mode == SEED_MODE_FACES) {
		if ((r = hipMemsetAsync(s.large, 0, sizeof(uint32_t), st)) != hipSuccess) return r;
		hipLaunchKernelGGL(seed_face_kernel, dim3((unsigned)std::min<size_t>(((size_t)nFaces + 255) / 256, SEED_MAX_BLOCKS)), dim3(256), 0, st, s.proj, s.z, s.faces, nFaces, w, h,
		                   s.boxMax, s.keys, s.large);
		hipLaunchKernelGGL(seed_large_kernel, dim3(std::min<uint32_t>(nFaces, SEED_LARGE_BLOCKS), SEED_LARGE_SPLIT), dim3(256), 0, st, s.proj, s.z, s.faces, w, h, s.keys, s.large);
	} else {
		hipLaunchKernelGGL(seed_point_kernel, dim3((unsigned)std::min<size_t>(((size_t)nVerts + 255) / 256, SEED_MAX_BLOCKS)), dim3(256), 0, st, s.proj, nVerts, w, h, s.keys);
	}
	hipLaunchKernelGGL(seed_resolve_kernel, dim3((unsigned)std::min<size_t>((P + 255) / 256, SEED_MAX_BLOCKS)), dim3(256), 0, st, mode, s.proj, s.z, dNormal ? s.normals.p : nullptr,
	                   s.faces, w, h, s.keys, dDepth, dNormal);
	if ((r = hipGetLastError()) != hipSuccess) return r;
	return hipEventRecord(s.ev[1], st);
}

// the statistics of the call just run (the stream is synchronised)
static hipError_t seedCollect(SeedWork& s, int mode, bool empty) {
	float ms = 0;
	if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) s.statUs = (uint64_t)(ms * 1e3 + .5);
	if (mode == SEED_MODE_FACES && !empty) {
		uint32_t n = 0;
		const hipError_t r = hipMemcpy(&n, s.large, sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (r != hipSuccess) return r;
		s.statLarge = n;
	}
	return hipSuccess;
}
