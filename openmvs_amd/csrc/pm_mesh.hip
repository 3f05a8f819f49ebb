// pm_mesh.hip -- Mesh::Project (libs/MVS/Mesh.cpp:3874-3968, TRasterMesh in Mesh.h:283-353) on the device: a triangle mesh rendered into the depth and normal maps
// of many views at once, and the vertex visibility test of Scene::SampleMeshWithVisibility (libs/MVS/Scene.cpp:656-667) against those maps.
//
//   pm_mesh_vertex_kernel     one (view, vertex) per lane: TRasterMeshBase::ProjectVertex in double, a 16-byte record out
//   pm_mesh_face_kernel       one (view, face) per lane: the reject, the box, the area; a box of at most `boxMax` pixels is walked by the lane, a larger one is appended
//                             to the view's list
//   pm_mesh_large_kernel      one workgroup per listed face, its 256 lanes striding over the box
//   pm_mesh_resolve_kernel    one pixel per lane: depth from the key, the winner's barycentrics recomputed for the normal
//   pm_mesh_visible_kernel    one (vertex, word of 32 views) per lane: the bitset word composed in a register, one plain store
//
// The reference visits the faces in index order and keeps a pixel's depth when `depth == 0 || depth > z`: a pixel ends with the smallest z over the faces that cover
// its centre, and among bit-equal z with the lowest face index.  z is a positive finite float, so its bit pattern orders as its value, and that winner is the minimum of
// the 64-bit key (z bits << 32 | face index): one atomicMin per (face, pixel) on a buffer cleared to all ones gives it whatever order the lanes run in (the idiom of
// FilterDepthMap's splat, pm_filter.hip).  Both face routes and the resolve pass call pm_mesh_setup / pm_mesh_pixel, the float and double expressions of
// TImage::RasterizeTriangleBary and the raster functor in the reference's order (no contraction, IEEE division): the keys of the two routes and the barycentrics the
// resolve pass recomputes are the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define PM_MESH_OK 1u        // every test of ProjectVertex passed: ptc.z > 0 (the double) and the projection inside the image with a border of 3
#define PM_MESH_FRONT 2u     // ptc.z > 0: x and y hold the projection

struct PMMeshVert { float x, y, z; uint32_t flags; };            // pti, (float)ptc.z
struct PMMeshView {
	double R[9], C[3], k00, k11, k02, k12;
	float Rf[9];                                                  // Matrix3x3f(camera.R), the normal map's rotation
	int w, h, wantNormal, pad;
	unsigned long long pix;                                       // first pixel of this view in the batch's key / depth / normal buffers
};
struct PMMeshTri { float x[3], y[3], z[3], inv; int x0, y0, x1, y1; };

// EdgeFunction(a, b, c), libs/Common/Util.inl:602-604: (c - a).cross(b - a) -- the differences in float, the cross product in double (cv::Point_::cross), narrowed
__device__ __forceinline__ float pm_mesh_edge(float ax, float ay, float bx, float by, float cx, float cy) {
	return (float)((double)(cx - ax) * (double)(by - ay) - (double)(cy - ay) * (double)(bx - ax));
}

// RasterizeTriangleBary up to its pixel loop: false = nothing is drawn (the box misses the image, or area <= 0)
__device__ __forceinline__ bool pm_mesh_setup(const PMMeshVert& a, const PMMeshVert& b, const PMMeshVert& c, int w, int h, PMMeshTri& t) {
	t.x[0] = a.x; t.y[0] = a.y; t.z[0] = a.z; t.x[1] = b.x; t.y[1] = b.y; t.z[1] = b.z; t.x[2] = c.x; t.y[2] = c.y; t.z[2] = c.z;
	const float mnx = fminf(fminf(a.x, b.x), c.x), mxx = fmaxf(fmaxf(a.x, b.x), c.x), mny = fminf(fminf(a.y, b.y), c.y), mxy = fmaxf(fmaxf(a.y, b.y), c.y);
	if (mxx < 0.f || mnx > (float)(w - 1) || mxy < 0.f || mny > (float)(h - 1)) return false;
	t.x0 = max((int)floorf(mnx), 0); t.y0 = max((int)floorf(mny), 0); t.x1 = min((int)ceilf(mxx), w - 1); t.y1 = min((int)ceilf(mxy), h - 1);
	const float area = pm_mesh_edge(a.x, a.y, b.x, b.y, c.x, c.y);
	if (area <= 0.f) return false;
	t.inv = 1.f / area;
	return true;
}

// One pixel of the loop: false = its centre is outside; else the perspective-correct barycentrics (Util.inl:746-749) and z (TRasterMeshBase::ComputeDepth)
__device__ __forceinline__ bool pm_mesh_pixel(const PMMeshTri& t, int px, int py, float pb[3], float& z) {
	const float fx = (float)px, fy = (float)py;
	const float b1 = pm_mesh_edge(t.x[1], t.y[1], t.x[2], t.y[2], fx, fy) * t.inv;
	if (b1 < 0.f) return false;
	const float b2 = pm_mesh_edge(t.x[2], t.y[2], t.x[0], t.y[0], fx, fy) * t.inv;
	if (b2 < 0.f) return false;
	const float b3 = pm_mesh_edge(t.x[0], t.y[0], t.x[1], t.y[1], fx, fy) * t.inv;
	if (b3 < 0.f) return false;
	const float p0 = b1 * t.z[1] * t.z[2], p1 = b2 * t.z[0] * t.z[2], p2 = b3 * t.z[0] * t.z[1];
	const float invd = 1.f / (p0 + p1 + p2);
	pb[0] = invd * p0; pb[1] = invd * p1; pb[2] = invd * p2;
	z = pb[0] * t.z[0] + pb[1] * t.z[1] + pb[2] * t.z[2];
	return true;
}

__device__ __forceinline__ void pm_mesh_offer(unsigned long long* __restrict__ keys, const PMMeshTri& t, int w, int px, int py, uint32_t face) {
	float pb[3], z;
	if (pm_mesh_pixel(t, px, py, pb, z)) atomicMin(keys + ((size_t)py * w + px), ((unsigned long long)__float_as_uint(z) << 32) | face);
}

// rec[view][vertex] for the views of the batch (blockIdx.y) and every vertex
__global__ __launch_bounds__(256) void pm_mesh_vertex_kernel(const PMMeshView* __restrict__ views, const float* __restrict__ verts, uint32_t nVerts, PMMeshVert* __restrict__ rec) {
	const PMMeshView& v = views[blockIdx.y];
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nVerts; i += (size_t)gridDim.x * 256u) {
		const double dx = (double)verts[3 * i] - v.C[0], dy = (double)verts[3 * i + 1] - v.C[1], dz = (double)verts[3 * i + 2] - v.C[2];
		const double cx = 0. + v.R[0] * dx + v.R[1] * dy + v.R[2] * dz, cy = 0. + v.R[3] * dx + v.R[4] * dy + v.R[5] * dz, cz = 0. + v.R[6] * dx + v.R[7] * dy + v.R[8] * dz;
		PMMeshVert o = {0.f, 0.f, (float)cz, 0u};
		if (cz > 0.) {
			o.x = (float)(v.k02 + v.k00 * (cx / cz)); o.y = (float)(v.k12 + v.k11 * (cy / cz));
			o.flags = PM_MESH_FRONT | ((o.x >= 3.f && o.y >= 3.f && o.x <= (float)(v.w - 4) && o.y <= (float)(v.h - 4)) ? PM_MESH_OK : 0u);
		}
		rec[(size_t)blockIdx.y * nVerts + i] = o;
	}
}

// the three records of a face, or false when a vertex fails ProjectVertex (the face is skipped whole) or nothing is drawn
__device__ __forceinline__ bool pm_mesh_face(const PMMeshVert* __restrict__ rec, const uint32_t* __restrict__ faces, size_t f, int w, int h, PMMeshTri& t) {
	const PMMeshVert a = rec[faces[3 * f]], b = rec[faces[3 * f + 1]], c = rec[faces[3 * f + 2]];
	if (!(a.flags & b.flags & c.flags & PM_MESH_OK)) return false;
	return pm_mesh_setup(a, b, c, w, h, t);
}

__global__ __launch_bounds__(256) void pm_mesh_face_kernel(const PMMeshView* __restrict__ views, const PMMeshVert* __restrict__ rec, uint32_t nVerts, const uint32_t* __restrict__ faces,
		uint32_t nFaces, int boxMax, unsigned long long* __restrict__ keys, uint32_t* __restrict__ largeCount, uint32_t* __restrict__ largeList) {
	const PMMeshView& v = views[blockIdx.y];
	const PMMeshVert* r = rec + (size_t)blockIdx.y * nVerts;
	unsigned long long* k = keys + v.pix;
	for (size_t f = (size_t)blockIdx.x * 256u + threadIdx.x; f < nFaces; f += (size_t)gridDim.x * 256u) {
		PMMeshTri t;
		if (!pm_mesh_face(r, faces, f, v.w, v.h, t)) continue;
		if ((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > boxMax) {
			largeList[(size_t)blockIdx.y * nFaces + atomicAdd(largeCount + blockIdx.y, 1u)] = (uint32_t)f;
			continue;
		}
		for (int y = t.y0; y <= t.y1; ++y) for (int x = t.x0; x <= t.x1; ++x) pm_mesh_offer(k, t, v.w, x, y, (uint32_t)f);
	}
}

__global__ __launch_bounds__(256) void pm_mesh_large_kernel(const PMMeshView* __restrict__ views, const PMMeshVert* __restrict__ rec, uint32_t nVerts, const uint32_t* __restrict__ faces,
		uint32_t nFaces, unsigned long long* __restrict__ keys, const uint32_t* __restrict__ largeCount, const uint32_t* __restrict__ largeList) {
	const PMMeshView& v = views[blockIdx.y];
	const PMMeshVert* r = rec + (size_t)blockIdx.y * nVerts;
	unsigned long long* k = keys + v.pix;
	const uint32_t n = largeCount[blockIdx.y];
	for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
		const uint32_t f = largeList[(size_t)blockIdx.y * nFaces + e];
		PMMeshTri t;
		if (!pm_mesh_face(r, faces, f, v.w, v.h, t)) continue;          // (listed faces passed this already)
		const int bw = t.x1 - t.x0 + 1;
		const int np = bw * (t.y1 - t.y0 + 1);                          // (a view has at most INT_MAX pixels: pm_host_mesh.hip)
		for (int p = threadIdx.x; p < np; p += 256) {
			const int y = p / bw;
			pm_mesh_offer(k, t, v.w, t.x0 + (p - y * bw), t.y0 + y, f);
		}
	}
}

__global__ __launch_bounds__(256) void pm_mesh_resolve_kernel(const PMMeshView* __restrict__ views, const PMMeshVert* __restrict__ rec, uint32_t nVerts, const uint32_t* __restrict__ faces,
		const float* __restrict__ vnormals, const unsigned long long* __restrict__ keys, float* __restrict__ depth, float* __restrict__ normal) {
	const PMMeshView& v = views[blockIdx.y];
	const PMMeshVert* r = rec + (size_t)blockIdx.y * nVerts;
	const size_t n = (size_t)v.w * (size_t)v.h;
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
		const unsigned long long key = keys[v.pix + i];
		const bool hit = key != ~0ull;
		depth[v.pix + i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
		if (!v.wantNormal) continue;
		float o0 = 0.f, o1 = 0.f, o2 = 0.f;
		if (hit) {
			const size_t f = (uint32_t)key;
			const int py = (int)((unsigned)i / (unsigned)v.w), px = (int)i - py * v.w;
			PMMeshTri t; float pb[3], z;
			if (pm_mesh_face(r, faces, f, v.w, v.h, t) && pm_mesh_pixel(t, px, py, pb, z)) {
				const float* n0 = vnormals + 3 * (size_t)faces[3 * f]; const float* n1 = vnormals + 3 * (size_t)faces[3 * f + 1]; const float* n2 = vnormals + 3 * (size_t)faces[3 * f + 2];
				const float a0 = n0[0] * pb[0] + n1[0] * pb[1] + n2[0] * pb[2], a1 = n0[1] * pb[0] + n1[1] * pb[1] + n2[1] * pb[2], a2 = n0[2] * pb[0] + n1[2] * pb[1] + n2[2] * pb[2];
				const double nv = __builtin_sqrt((double)a0 * a0 + (double)a1 * a1 + (double)a2 * a2);      // cv::normalize: v * (1 / |v|), norm and product in double
				const double s = nv ? 1. / nv : 0.;
				const float u0 = (float)(a0 * s), u1 = (float)(a1 * s), u2 = (float)(a2 * s);
				o0 = 0.f + v.Rf[0] * u0 + v.Rf[1] * u1 + v.Rf[2] * u2;                                      // cv::Matx product: accumulated from 0, left to right
				o1 = 0.f + v.Rf[3] * u0 + v.Rf[4] * u1 + v.Rf[5] * u2;
				o2 = 0.f + v.Rf[6] * u0 + v.Rf[7] * u1 + v.Rf[8] * u2;
			}
		}
		float* o = normal + 3 * (v.pix + i);
		o[0] = o0; o[1] = o1; o[2] = o2;
	}
}

// Word `word0 + blockIdx.y` of every vertex's bitset: bit (view & 31) for the views [viewLo, viewHi) of the batch that fall into it (batch view b is scene view
// view0 + b).  A batch starts on a word boundary or inside a word earlier launches began: then the word is read first.  One writer per word in a launch.
__global__ __launch_bounds__(256) void pm_mesh_visible_kernel(const PMMeshView* __restrict__ views, const PMMeshVert* __restrict__ rec, uint32_t nVerts, const float* __restrict__ depth,
		int view0, int nBatch, int nWords, float thFrontDepth, uint32_t* __restrict__ bits) {
	const int word = view0 / 32 + (int)blockIdx.y;
	const int lo = max(word * 32, view0), hi = min(word * 32 + 32, view0 + nBatch);
	for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nVerts; i += (size_t)gridDim.x * 256u) {
		uint32_t* out = bits + i * (size_t)nWords + word;
		uint32_t m = (lo & 31) ? *out : 0u;
		for (int g = lo; g < hi; ++g) {
			const PMMeshView& v = views[g - view0];
			const PMMeshVert p = rec[(size_t)(g - view0) * nVerts + i];
			if (!(p.flags & PM_MESH_FRONT) || !(p.z > 0.f)) continue;                                       // xz.z <= 0 (the float)
			if (!(p.x >= 1.f && p.y >= 1.f && p.x <= (float)(v.w - 2) && p.y <= (float)(v.h - 2))) continue;   // isInsideWithBorder<float,1>
			const int px = (int)floorf(p.x + .5f), py = (int)floorf(p.y + .5f);                             // ROUND2INT
			if (p.z * thFrontDepth < depth[v.pix + (size_t)py * v.w + px]) m |= 1u << (g & 31);
		}
		*out = m;
	}
}
