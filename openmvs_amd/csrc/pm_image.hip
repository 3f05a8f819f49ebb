// pm_image.hip -- preparing a view's images on the device from the decoded 8-bit image (the engine's image store, pm_host_image.hip):
//
//   pmimg_area_u8_kernel<MODE, PPL>   cv::resize(..., INTER_AREA) of an 8-bit 3-channel image that shrinks on both axes (Image::ResizeImage, libs/MVS/Image.cpp:139-155)
//                                      fused with TImage::toGray (libs/Common/Types.inl:2377-2425): the working-resolution BGR image (u8) and the gray float image
//   pmimg_area_f32_block_kernel        DepthData::ViewData::ScaleImage (libs/MVS/DepthMap.h:198-204), INTER_AREA with an integer factor (OpenCV's "area fast" path)
//   pmimg_area_f32_tab_kernel          ... with any other factor (computeResizeAreaTab + ResizeArea_Invoker, imgproc/src/resize.cpp)
//   pmimg_cubic_f32                    ... enlarging, INTER_CUBIC (HResizeCubic / VResizeCubic in their scalar form)
//
// Every result equals, bit for bit, the host statement it replaces (openmvs_amd/densify.py: _resize_area_u8, scale_image; views.to_gray): float multiply, then add, in the
// order written there, no contraction (-ffp-contract=off is part of the build).  The tables (area cells, cubic taps and weights) are built on the host in double / float as
// those functions build them (pmimg_area_tab, pmimg_cubic_tab below) and uploaded: the kernels only read them.
// Plain loads and stores; every thread owns its output pixels, so there is nothing to synchronise.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#ifndef PMIMG_PPL
#define PMIMG_PPL 4   // output pixels per lane of pmimg_area_u8_kernel: 4 = one 12-byte BGR store and one 16-byte gray store per lane, 1 = three byte stores and a dword
#endif

// One axis of an area table on the device: destination cell d reads the entries [ofs[d], ofs[d + 1]) -- source index si, weight al -- in that order
struct PMImgTab { const int* ofs; const int* si; const float* al; };
// One axis of a cubic table: destination d reads the four (clamped) source indices idx[4 d ..] with the weights c[4 d ..]
struct PMImgCubicTab { const int* idx; const float* c; };

struct PMImgU8 {
	const uint8_t* src; int W, H;      // the decoded image, 3 interleaved channels
	int w, h;                          // the working size
	int swapRB;                        // channelOrder 1: the source is R, G, B
	int fx, fy; float inv;             // MODE 2: the integer factors and float(1.0 / (fx fy))
	PMImgTab tx, ty;                   // MODE 3
	uint8_t* bgr; float* gray;         // out: w*h*3, w*h
};

enum { PMIMG_COPY = 0, PMIMG_HALF = 1, PMIMG_INT = 2, PMIMG_TAB = 3 };

// saturate_cast<uchar>(float): round to nearest, ties to even, then clamp
__device__ __forceinline__ uint8_t pmimg_sat_u8(float v) {
	const float r = rintf(v);
	return (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// the B, G, R bytes of destination pixel (x, y)
template <int MODE> __device__ __forceinline__ void pmimg_px_u8(const PMImgU8& a, int x, int y, uint8_t out[3]) {
	const size_t pitch = (size_t)a.W * 3;
	#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const int sc = a.swapRB ? 2 - c : c;
		if (MODE == PMIMG_COPY) {
			out[c] = a.src[(size_t)y * pitch + (size_t)x * 3 + sc];
		} else if (MODE == PMIMG_HALF) {          // ResizeAreaFastVec for integer pixels: (a + b + c + d + 2) >> 2
			const uint8_t* p = a.src + (size_t)(2 * y) * pitch + (size_t)(2 * x) * 3 + sc;
			out[c] = (uint8_t)(((unsigned)p[0] + p[3] + p[pitch] + p[pitch + 3] + 2u) >> 2);
		} else if (MODE == PMIMG_INT) {           // integer box sum times float(1 / (fx fy)), saturate_cast
			unsigned long long s = 0;
			const uint8_t* p = a.src + (size_t)(y * a.fy) * pitch + (size_t)(x * a.fx) * 3 + sc;
			for (int j = 0; j < a.fy; ++j, p += pitch) for (int i = 0; i < a.fx; ++i) s += p[i * 3];
			out[c] = pmimg_sat_u8((float)s * a.inv);
		} else {                                   // the general path: rows weighted in x in table order, then the rows in y, all in float
			float sum = 0.f;
			const int x0 = a.tx.ofs[x], x1 = a.tx.ofs[x + 1];
			for (int k = a.ty.ofs[y], k1 = a.ty.ofs[y + 1]; k < k1; ++k) {
				const uint8_t* row = a.src + (size_t)a.ty.si[k] * pitch + sc;
				float buf = 0.f;
				for (int j = x0; j < x1; ++j) buf = buf + (float)row[(size_t)a.tx.si[j] * 3] * a.tx.al[j];
				sum = sum + a.ty.al[k] * buf;
			}
			out[c] = pmimg_sat_u8(sum);
		}
	}
}

// TImage::toGray with CONVERT::NormRGB_t: the bytes times (1.f / 255.f), then 0.114 B + 0.587 G + 0.299 R summed in that order
__device__ __forceinline__ float pmimg_gray(const uint8_t p[3]) {
	const float n = 1.f / 255.f;
	const float b = (float)p[0] * n, g = (float)p[1] * n, r = (float)p[2] * n;
	return (0.114f * b + 0.587f * g) + 0.299f * r;
}

struct PMImgU3 { uint32_t a, b, c; };

// The destination as one run of w*h pixels, PPL consecutive ones per lane: with PPL = 4 a lane's BGR bytes are 12 bytes at a multiple of 12 and its gray values 16 bytes at
// a multiple of 16, whatever w is (a group may cross a row end), so a wave stores 768 + 1024 contiguous bytes.
template <int MODE, int PPL> __global__ __launch_bounds__(256) void pmimg_area_u8_kernel(PMImgU8 a) {
	const unsigned n = (unsigned)a.w * (unsigned)a.h;
	const unsigned groups = (n + PPL - 1) / PPL;
	for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
		const unsigned p0 = g * PPL;
		const int cnt = n - p0 < (unsigned)PPL ? (int)(n - p0) : PPL;
		uint8_t px[PPL * 3]; float gr[PPL];
		#pragma unroll
		for (int k = 0; k < PPL; ++k) {
			if (k < cnt) {
				const unsigned p = p0 + k;
				pmimg_px_u8<MODE>(a, (int)(p % (unsigned)a.w), (int)(p / (unsigned)a.w), px + 3 * k);
				gr[k] = pmimg_gray(px + 3 * k);
			} else { px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = 0; gr[k] = 0.f; }
		}
		if (PPL == 4 && cnt == 4) {
			PMImgU3 u;
			u.a = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16 | (uint32_t)px[3] << 24;
			u.b = (uint32_t)px[4] | (uint32_t)px[5] << 8 | (uint32_t)px[6] << 16 | (uint32_t)px[7] << 24;
			u.c = (uint32_t)px[8] | (uint32_t)px[9] << 8 | (uint32_t)px[10] << 16 | (uint32_t)px[11] << 24;
			*(PMImgU3*)(a.bgr + (size_t)p0 * 3) = u;
			*(float4*)(a.gray + p0) = make_float4(gr[0], gr[1], gr[2], gr[3]);
		} else {
			for (int k = 0; k < cnt; ++k) {
				uint8_t* o = a.bgr + (size_t)(p0 + k) * 3;
				o[0] = px[3 * k]; o[1] = px[3 * k + 1]; o[2] = px[3 * k + 2];
				a.gray[p0 + k] = gr[k];
			}
		}
	}
}

// ScaleImage, scale = 1 / f: complete f x f blocks are ((a + b) + (c + d)) * 0.25f for f = 2, else the row-major running sum times inv = float(1 / f^2); blocks cut by the
// right / bottom border are the running sum of what is there DIVIDED by the count
__global__ __launch_bounds__(256) void pmimg_area_f32_block_kernel(const float* __restrict__ src, int W, int H, float* __restrict__ dst, int w, int h, int f, float inv) {
	const unsigned n = (unsigned)w * (unsigned)h;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const int x = (int)(i % (unsigned)w), y = (int)(i / (unsigned)w);
		const int x0 = x * f, y0 = y * f;
		const int x1 = x0 + f < W ? x0 + f : W, y1 = y0 + f < H ? y0 + f : H;
		float o = 0.f;
		if (x1 - x0 == f && y1 - y0 == f && f == 2) {
			const float* p = src + (size_t)y0 * W + x0;
			o = ((p[0] + p[1]) + (p[W] + p[W + 1])) * 0.25f;
		} else if (x1 > x0 && y1 > y0) {
			float acc = 0.f;
			for (int yy = y0; yy < y1; ++yy) for (int xx = x0; xx < x1; ++xx) acc = acc + src[(size_t)yy * W + xx];
			o = (x1 - x0 == f && y1 - y0 == f) ? acc * inv : acc / (float)((x1 - x0) * (y1 - y0));
		}
		dst[i] = o;
	}
}

// ScaleImage, any other scale < 1: pmimg_area_u8_kernel's general path on floats, without the final rounding
__global__ __launch_bounds__(256) void pmimg_area_f32_tab_kernel(const float* __restrict__ src, int W, float* __restrict__ dst, int w, int h, PMImgTab tx, PMImgTab ty) {
	const unsigned n = (unsigned)w * (unsigned)h;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const int x = (int)(i % (unsigned)w), y = (int)(i / (unsigned)w);
		const int x0 = tx.ofs[x], x1 = tx.ofs[x + 1];
		float sum = 0.f;
		for (int k = ty.ofs[y], k1 = ty.ofs[y + 1]; k < k1; ++k) {
			const float* row = src + (size_t)ty.si[k] * W;
			float buf = 0.f;
			for (int j = x0; j < x1; ++j) buf = buf + row[tx.si[j]] * tx.al[j];
			sum = sum + ty.al[k] * buf;
		}
		dst[i] = sum;
	}
}

// ScaleImage, scale > 1: four clamped taps per axis, rows first, then columns, each pass ((t0 c0 + t1 c1) + t2 c2) + t3 c3
__global__ __launch_bounds__(256) void pmimg_cubic_f32(const float* __restrict__ src, int W, float* __restrict__ dst, int w, int h, PMImgCubicTab tx, PMImgCubicTab ty) {
	const unsigned n = (unsigned)w * (unsigned)h;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const int x = (int)(i % (unsigned)w), y = (int)(i / (unsigned)w);
		const int i0 = tx.idx[4 * x], i1 = tx.idx[4 * x + 1], i2 = tx.idx[4 * x + 2], i3 = tx.idx[4 * x + 3];
		const float a0 = tx.c[4 * x], a1 = tx.c[4 * x + 1], a2 = tx.c[4 * x + 2], a3 = tx.c[4 * x + 3];
		float r[4];
		for (int k = 0; k < 4; ++k) {
			const float* row = src + (size_t)ty.idx[4 * y + k] * W;
			r[k] = ((row[i0] * a0 + row[i1] * a1) + row[i2] * a2) + row[i3] * a3;
		}
		dst[i] = ((r[0] * ty.c[4 * y] + r[1] * ty.c[4 * y + 1]) + r[2] * ty.c[4 * y + 2]) + r[3] * ty.c[4 * y + 3];
	}
}

// ---- the tables, on the host -----------------------------------------------------------------------------------------------------------------------

struct PMImgHostTab { std::vector<int> ofs, si; std::vector<float> al; };

// OpenCV's computeResizeAreaTab for one axis (densify._area_tab): scale = ssize / dsize in double, the partial cells at both ends weighted by the fraction of the cell
// they cover, a partial cell of less than 1e-3 dropped.  Returns false if an entry would lie outside the source (never, for a shrinking axis).
static bool pmimg_area_tab(int ssize, int dsize, double scale, PMImgHostTab& t) {
	t.ofs.assign(1, 0); t.si.clear(); t.al.clear();
	for (int dx = 0; dx < dsize; ++dx) {
		const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
		const double cell = std::min(scale, ssize - fsx1);
		int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
		sx2 = std::min(sx2, ssize - 1);
		sx1 = std::min(sx1, sx2);
		if (sx1 - fsx1 > 1e-3) { t.si.push_back(sx1 - 1); t.al.push_back((float)((sx1 - fsx1) / cell)); }
		for (int sx = sx1; sx < sx2; ++sx) { t.si.push_back(sx); t.al.push_back((float)(1.0 / cell)); }
		if (fsx2 - sx2 > 1e-3) { t.si.push_back(sx2); t.al.push_back((float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell)); }
		t.ofs.push_back((int)t.si.size());
	}
	for (int s : t.si) if (s < 0 || s >= ssize) return false;
	return true;
}

struct PMImgHostCubic { std::vector<int> idx; std::vector<float> c; };

// The taps of resizeGeneric_'s cubic pass for one axis (densify._resize_cubic_f32.taps, _cubic_coeffs): position (d + 0.5) scale - 0.5 in double, rounded to float; its
// floor; interpolateCubic's weights (A = -0.75) of the fraction in float; taps outside the image clamped to the border
static void pmimg_cubic_tab(int ndst, int nsrc, double scale, PMImgHostCubic& t) {
	t.idx.resize((size_t)ndst * 4); t.c.resize((size_t)ndst * 4);
	const float A = -0.75f;
	for (int d = 0; d < ndst; ++d) {
		float fx = (float)((d + 0.5) * scale - 0.5);
		const float fl = floorf(fx);
		const long long sx = (long long)fl;
		fx = fx - fl;
		for (int k = 0; k < 4; ++k) t.idx[(size_t)d * 4 + k] = (int)std::min<long long>(std::max<long long>(sx + k - 1, 0), nsrc - 1);
		const float x1 = fx + 1.f, u = 1.f - fx;
		const float c0 = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
		const float c1 = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
		const float c2 = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
		const float c3 = 1.f - c0 - c1 - c2;
		float* c = &t.c[(size_t)d * 4];
		c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
	}
}
