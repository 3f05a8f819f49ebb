// pm_cloud.hip -- the last block of Scene::DenseReconstruction on the fused cloud (libs/MVS/SceneDensify.cpp:1724-1737 in the reference),
// run where the cloud already lies (PMFuseOut, see pm_fuse.hip):
//
//   crop     PointCloud::RemovePointsOutside(OBB) (PointCloud.cpp:82-87): a backward loop whose RemoveAt moves the current last point into
//            the hole.  Position q is processed when the array holds s(q) = n - #{holes above q} points; a hole q < s(q)-1 receives the
//            content of position s(q)-1, which was itself settled when that position was processed and never changes afterwards.  So the
//            point that ends at q is c(q) = q for a kept point and c(s(q)-1) for a hole: chains that only climb and end at a kept point
//            (a hole with s(q)-1 == q is dropped and no chain reaches it).  pmcl_crop_next builds the links from one scan of the hole
//            flags, pmcl_jump resolves them by pointer jumping, pmcl_crop_scatter gathers points / views / weights / colours / normals.
//   colours  EstimatePointColors (DepthMap.cpp:1429-1465): one thread per point, the view of smallest PointDepth, ProjectPointP and
//            TImage<Pixel8U>::sample with the byte truncations of TPixel's operators.  Bit-exact.
//   normals  EstimatePointNormals (DepthMap.cpp:1469-1519): k nearest points of the whole cloud (the point itself included), ordered by
//            double squared distance then index; PCA of the neighbourhood in double (cyclic Jacobi), cast to float, oriented towards the
//            camera centre of the point's first view.
//            Spatial index: a uniform grid, points counting-sorted by cell (histogram, scan, scatter).  One lane per query, queries in
//            cell order; rings of cells around the query's cell are searched until the nearest a cell of the next ring can be is strictly
//            farther than the current k-th distance.  Candidates are screened in f32 with a margin; membership and order are decided on
//            the double distance with the index tie-break, so the result does not depend on the grid, its density or the visit order.
#pragma once
#include "pm_fuse.h"

#define PMCL_TILE 1024
#define PMCL_TB 256
#define PMCL_NONE 0xFFFFFFFFu

struct PMClObb { float rot[9], pos[3], ext[3]; };
struct PMClImg { const uint8_t* bgr; int w, h; };
struct PMClGrid {
	double ox, oy, oz, h, invh;
	int nx, ny, nz;
	const uint32_t* cellStart;     // [nx*ny*nz + 1]
	const float4* spts;            // points sorted by cell: x, y, z, index (bits)
};

// TOBB<float,3>::Intersects (OBB.inl:388-400): dist = rot * (pt - pos), |dist| <= ext on every axis
PM_HD bool pmcl_inside(const PMClObb& b, const float* p) {
	const float d0 = p[0] - b.pos[0], d1 = p[1] - b.pos[1], d2 = p[2] - b.pos[2];
	for (int r = 0; r < 3; ++r) {
		const float v = (b.rot[r*3+0] * d0 + b.rot[r*3+1] * d1) + b.rot[r*3+2] * d2;
		if (!(pm_fabsf(v) <= b.ext[r])) return false;
	}
	return true;
}

// ---- crop --------------------------------------------------------------------------------------------------------------------------
// hole flags and the holes per tile
__global__ __launch_bounds__(PMCL_TB) void pmcl_crop_flags(const float* points, uint32_t n, PMClObb b, uint8_t* hole, uint2* tileSums) {
	__shared__ uint32_t sc[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t cc = 0;
	for (uint32_t k = 0; k < 4; ++k) if (b0 + k < n) {
		const uint8_t h = pmcl_inside(b, points + (size_t)(b0 + k) * 3) ? 0 : 1;
		hole[b0 + k] = h; cc += h;
	}
	sc[t] = cc;
	__syncthreads();
	for (uint32_t s = PMCL_TB / 2; s > 0; s >>= 1) {
		if (t < s) sc[t] += sc[t + s];
		__syncthreads();
	}
	if (t == 0) tileSums[blockIdx.x] = make_uint2(sc[0], 0u);
}

// links: nxt[q] = q for a kept point, s(q)-1 for a hole that receives a point, PMCL_NONE for a hole that is the last point when it is removed
__global__ __launch_bounds__(PMCL_TB) void pmcl_crop_next(const uint8_t* hole, uint32_t n, const uint2* tileOff, const uint32_t* totals, uint32_t* nxt) {
	__shared__ uint32_t sc[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t h4[4], cc = 0;
	for (uint32_t k = 0; k < 4; ++k) { h4[k] = b0 + k < n ? hole[b0 + k] : 0u; cc += h4[k]; }
	sc[t] = cc;
	__syncthreads();
	for (uint32_t off = 1; off < PMCL_TB; off <<= 1) {
		const uint32_t a = t >= off ? sc[t - off] : 0u;
		__syncthreads();
		sc[t] += a;
		__syncthreads();
	}
	const uint32_t H = totals[0];
	uint32_t upto = tileOff[blockIdx.x].x + sc[t] - cc;       // holes before b0
	for (uint32_t k = 0; k < 4; ++k) {
		const uint32_t q = b0 + k;
		if (q >= n) break;
		upto += h4[k];                                           // holes at or below q
		if (!h4[k]) { nxt[q] = q; continue; }
		const uint32_t last = n - (H - upto) - 1;                // s(q) - 1
		nxt[q] = last > q ? last : PMCL_NONE;
	}
}

// one round of pointer jumping (in place: a lane reading an already advanced link only jumps further along the same chain)
__global__ __launch_bounds__(256) void pmcl_jump(uint32_t* nxt, uint32_t n, uint32_t* changed) {
	uint32_t ch = 0;
	for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
		const uint32_t x = nxt[q];
		if (x == q || x == PMCL_NONE) continue;
		const uint32_t y = nxt[x];
		if (y != x) { nxt[q] = y; ch = 1; }
	}
	if (ch) atomicOr(changed, 1u);
}

PM_HD uint32_t pmcl_nv(const uint32_t* vs, uint32_t src) { return vs[src + 1] - vs[src]; }

__global__ __launch_bounds__(PMCL_TB) void pmcl_crop_tile_sums(const uint32_t* src, const uint32_t* vs, uint32_t m, uint2* tileSums) {
	__shared__ uint32_t sv[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t vv = 0;
	for (uint32_t k = 0; k < 4; ++k) if (b0 + k < m) vv += pmcl_nv(vs, src[b0 + k]);
	sv[t] = vv;
	__syncthreads();
	for (uint32_t s = PMCL_TB / 2; s > 0; s >>= 1) {
		if (t < s) sv[t] += sv[t + s];
		__syncthreads();
	}
	if (t == 0) tileSums[blockIdx.x] = make_uint2(sv[0], 0u);
}

__global__ __launch_bounds__(PMCL_TB) void pmcl_crop_scatter(PMFuseOut in, const uint32_t* src, uint32_t m, const uint2* tileOff, PMFuseOut o) {
	__shared__ uint32_t sv[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t n4[4], s4[4], vv = 0;
	for (uint32_t k = 0; k < 4; ++k) { s4[k] = b0 + k < m ? src[b0 + k] : 0u; n4[k] = b0 + k < m ? pmcl_nv(in.viewStart, s4[k]) : 0u; vv += n4[k]; }
	sv[t] = vv;
	__syncthreads();
	for (uint32_t off = 1; off < PMCL_TB; off <<= 1) {
		const uint32_t a = t >= off ? sv[t - off] : 0u;
		__syncthreads();
		sv[t] += a;
		__syncthreads();
	}
	uint32_t vs = tileOff[blockIdx.x].x + sv[t] - vv;
	for (uint32_t k = 0; k < 4; ++k) {
		const uint32_t p = b0 + k;
		if (p >= m) break;
		const uint32_t s = s4[k], v0 = in.viewStart[s];
		o.viewStart[p] = vs;
		for (int c = 0; c < 3; ++c) o.points[(size_t)p * 3 + c] = in.points[(size_t)s * 3 + c];
		if (o.colors) for (int c = 0; c < 3; ++c) o.colors[(size_t)p * 3 + c] = in.colors[(size_t)s * 3 + c];
		if (o.normals) for (int c = 0; c < 3; ++c) o.normals[(size_t)p * 3 + c] = in.normals[(size_t)s * 3 + c];
		for (uint32_t v = 0; v < n4[k]; ++v) {
			o.views[vs + v] = in.views[v0 + v]; o.weights[vs + v] = in.weights[v0 + v];
			o.projs[(size_t)(vs + v) * 2] = in.projs[(size_t)(v0 + v) * 2]; o.projs[(size_t)(vs + v) * 2 + 1] = in.projs[(size_t)(v0 + v) * 2 + 1];
		}
		vs += n4[k];
	}
}

// ---- colours -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pmcl_mark_views(const uint32_t* views, uint32_t nV, uint32_t nImages, uint32_t* used) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nV; i += gridDim.x * blockDim.x) {
		const uint32_t v = views[i];
		used[v < nImages ? v : nImages] = 1u;                    // slot nImages: a view index outside the scene
	}
}

// Pixel8U * float (TPixel::operator*: (uint8_t)(v * r)) and Pixel8U + Pixel8U (int sum narrowed), TImage<Pixel8U>::sample (Types.inl:2271-2281)
PM_HD uint8_t pmcl_mulu8(uint8_t a, float v) { return (uint8_t)(v * (float)a); }

PM_HD void pmcl_point_color(const PMFuseOut& o, uint32_t i, const PMFuseCam* cams, const PMClImg* imgs, uint8_t* col) {
	const float* X = o.points + (size_t)i * 3;
	double best = (double)3.402823466e+38f;                      // REAL bestDistance(FLT_MAX)
	int bi = -1;
	for (uint32_t v = o.viewStart[i]; v < o.viewStart[i + 1]; ++v) {
		const uint32_t img = o.views[v];
		if (!imgs[img].bgr) continue;
		const double* P = cams[img].P;
		const double d = P[8] * (double)X[0] + P[9] * (double)X[1] + P[10] * (double)X[2] + P[11];   // Camera::PointDepth
		if (best > d) { best = d; bi = (int)img; }
	}
	col[0] = col[1] = col[2] = 255;
	if (bi < 0) return;
	float q[3]; pmfu_projectP3(cams[bi], X, q);                  // ProjectPointP3<float>
	if (q[2] == 0.f) return;
	const float invZ = 1.f / q[2];
	const float px = q[0] * invZ, py = q[1] * invZ;
	const PMClImg im = imgs[bi];
	if (!(px >= 1.f && py >= 1.f && px <= (float)(im.w - 2) && py <= (float)(im.h - 2))) return;   // isInsideWithBorder<float,1>
	const int lx = (int)px, ly = (int)py;
	const float x = px - (float)lx, x1 = 1.f - x, y = py - (float)ly, y1 = 1.f - y;
	const uint8_t* r0 = im.bgr + ((size_t)ly * im.w + lx) * 3;
	const uint8_t* r1 = r0 + (size_t)im.w * 3;
	for (int c = 0; c < 3; ++c) {
		const uint8_t top = (uint8_t)(pmcl_mulu8(r0[c], x1) + pmcl_mulu8(r0[3 + c], x));
		const uint8_t bot = (uint8_t)(pmcl_mulu8(r1[c], x1) + pmcl_mulu8(r1[3 + c], x));
		col[c] = (uint8_t)(pmcl_mulu8(top, y1) + pmcl_mulu8(bot, y));
	}
}

__global__ __launch_bounds__(256) void pmcl_color_kernel(PMFuseOut o, uint32_t n, const PMFuseCam* cams, const PMClImg* imgs) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) pmcl_point_color(o, i, cams, imgs, o.colors + (size_t)i * 3);
}

// ---- grid ----------------------------------------------------------------------------------------------------------------------------
PM_HD uint32_t pmcl_ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// bb[0..2] = ordered min, bb[3..5] = ordered max (initialised to 0xFFFFFFFF / 0)
__global__ __launch_bounds__(256) void pmcl_bbox_kernel(const float* points, uint32_t n, uint32_t* bb) {
	uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
		for (int c = 0; c < 3; ++c) { const uint32_t u = pmcl_ord(points[(size_t)i * 3 + c]); mn[c] = u < mn[c] ? u : mn[c]; mx[c] = u > mx[c] ? u : mx[c]; }
	for (int off = 32; off > 0; off >>= 1)
		for (int c = 0; c < 3; ++c) {
			const uint32_t a = __shfl_down(mn[c], off), b = __shfl_down(mx[c], off);
			mn[c] = a < mn[c] ? a : mn[c]; mx[c] = b > mx[c] ? b : mx[c];
		}
	if ((threadIdx.x & 63) == 0) for (int c = 0; c < 3; ++c) { atomicMin(bb + c, mn[c]); atomicMax(bb + 3 + c, mx[c]); }
}

__global__ __launch_bounds__(256) void pmcl_sample_kernel(const float* points, uint32_t n, uint32_t S, float* out) {
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= S) return;
	const uint32_t i = (uint32_t)(((uint64_t)j * n) / S);
	for (int c = 0; c < 3; ++c) out[j * 3 + c] = points[(size_t)i * 3 + c];
}

PM_HD int pmcl_axis(double v, double o, double invh, int n) {
	const double t = floor((v - o) * invh);
	return t < 0. ? 0 : t >= (double)(n - 1) ? n - 1 : (int)t;
}
PM_HD uint32_t pmcl_cell(const PMClGrid& g, const float* p) {
	const int x = pmcl_axis((double)p[0], g.ox, g.invh, g.nx), y = pmcl_axis((double)p[1], g.oy, g.invh, g.ny), z = pmcl_axis((double)p[2], g.oz, g.invh, g.nz);
	return ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx + (uint32_t)x;
}

__global__ __launch_bounds__(256) void pmcl_count_kernel(const float* points, uint32_t n, PMClGrid g, uint32_t* cellOf, uint32_t* counts) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t c = pmcl_cell(g, points + (size_t)i * 3);
		cellOf[i] = c;
		atomicAdd(counts + c, 1u);
	}
}

__global__ __launch_bounds__(PMCL_TB) void pmcl_tile_sums_u32(const uint32_t* a, uint32_t n, uint2* tileSums) {
	__shared__ uint32_t sv[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t vv = 0;
	for (uint32_t k = 0; k < 4; ++k) if (b0 + k < n) vv += a[b0 + k];
	sv[t] = vv;
	__syncthreads();
	for (uint32_t s = PMCL_TB / 2; s > 0; s >>= 1) {
		if (t < s) sv[t] += sv[t + s];
		__syncthreads();
	}
	if (t == 0) tileSums[blockIdx.x] = make_uint2(sv[0], 0u);
}

// counts -> exclusive offsets, written to cellStart and back into counts (the scatter's cursors)
__global__ __launch_bounds__(PMCL_TB) void pmcl_scan_apply(uint32_t* counts, uint32_t n, const uint2* tileOff, uint32_t* cellStart) {
	__shared__ uint32_t sv[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t c4[4], vv = 0;
	for (uint32_t k = 0; k < 4; ++k) { c4[k] = b0 + k < n ? counts[b0 + k] : 0u; vv += c4[k]; }
	sv[t] = vv;
	__syncthreads();
	for (uint32_t off = 1; off < PMCL_TB; off <<= 1) {
		const uint32_t a = t >= off ? sv[t - off] : 0u;
		__syncthreads();
		sv[t] += a;
		__syncthreads();
	}
	uint32_t s = tileOff[blockIdx.x].x + sv[t] - vv;
	for (uint32_t k = 0; k < 4; ++k) {
		if (b0 + k >= n) break;
		cellStart[b0 + k] = s; counts[b0 + k] = s; s += c4[k];
	}
}

__global__ __launch_bounds__(256) void pmcl_scatter_kernel(const float* points, uint32_t n, const uint32_t* cellOf, uint32_t* cursor, float4* spts) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t pos = atomicAdd(cursor + cellOf[i], 1u);
		const float* p = points + (size_t)i * 3;
		spts[pos] = make_float4(p[0], p[1], p[2], __uint_as_float(i));
	}
}

// ---- k nearest neighbours + PCA ------------------------------------------------------------------------------------------------------
PM_HD bool pmcl_lt(double da, uint32_t ia, double db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// one Jacobi rotation zeroing a[p][q] of the symmetric 3x3 `a` (row-major), accumulated into the columns of v
template <int p, int q>
PM_HD void pmcl_rot(double* a, double* v) {
	const double apq = a[p*3+q];
	if (apq == 0.) return;
	const double theta = (a[q*3+q] - a[p*3+p]) / (2. * apq);
	const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
	const double c = 1. / sqrt(t * t + 1.), s = t * c;
	const int r = 3 - p - q;
	const double arp = a[r*3+p], arq = a[r*3+q];
	a[p*3+p] -= t * apq; a[q*3+q] += t * apq;
	a[p*3+q] = a[q*3+p] = 0.;
	a[r*3+p] = a[p*3+r] = c * arp - s * arq;
	a[r*3+q] = a[q*3+r] = s * arp + c * arq;
	for (int k = 0; k < 3; ++k) {
		const double vkp = v[k*3+p], vkq = v[k*3+q];
		v[k*3+p] = c * vkp - s * vkq; v[k*3+q] = s * vkp + c * vkq;
	}
}

// unit eigenvector of the smallest eigenvalue of the symmetric 3x3 `a` (cyclic Jacobi, double)
PM_HD void pmcl_smallest_eigvec(double* a, double* e) {
	double v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	for (int sweep = 0; sweep < 16; ++sweep) {
		const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
		const double dg = a[0] * a[0] + a[4] * a[4] + a[8] * a[8];
		if (!(off > 1e-40 * dg)) break;
		pmcl_rot<0, 1>(a, v); pmcl_rot<0, 2>(a, v); pmcl_rot<1, 2>(a, v);
	}
	const int m = a[0] <= a[4] ? (a[0] <= a[8] ? 0 : 2) : (a[4] <= a[8] ? 1 : 2);
	double x = v[m], y = v[3 + m], z = v[6 + m];
	const double l = sqrt(x * x + y * y + z * z);
	e[0] = x / l; e[1] = y / l; e[2] = z / l;
}

// PCA normal of the neighbourhood I[KM-k..KM) (linear_least_squares_fitting_3 over the points promoted to double), cast and oriented
template <int KM>
PM_HD void pmcl_pca_normal(const float* points, const uint32_t* I, int k, const float* Xq, const float* Cfirst, float* out) {
	double c[3] = {0., 0., 0.};
	#pragma unroll
	for (int j = 0; j < KM; ++j) if (j >= KM - k) { const float* p = points + (size_t)I[j] * 3; c[0] += (double)p[0]; c[1] += (double)p[1]; c[2] += (double)p[2]; }
	for (int d = 0; d < 3; ++d) c[d] /= (double)k;
	double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	#pragma unroll
	for (int j = 0; j < KM; ++j) if (j >= KM - k) {
		const float* p = points + (size_t)I[j] * 3;
		const double dx = (double)p[0] - c[0], dy = (double)p[1] - c[1], dz = (double)p[2] - c[2];
		a[0] += dx * dx; a[1] += dx * dy; a[2] += dx * dz; a[4] += dy * dy; a[5] += dy * dz; a[8] += dz * dz;
	}
	a[3] = a[1]; a[6] = a[2]; a[7] = a[5];
	double e[3]; pmcl_smallest_eigvec(a, e);
	float n[3] = {(float)e[0], (float)e[1], (float)e[2]};
	const float d0 = Cfirst[0] - Xq[0], d1 = Cfirst[1] - Xq[1], d2 = Cfirst[2] - Xq[2];
	if ((n[0] * d0 + n[1] * d1) + n[2] * d2 < 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }   // normal.dot(Cast<float>(C) - point) < 0
	out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
}

struct PMClKnnOut {
	const uint32_t* queries; uint32_t* idx;                   // knn mode: query list, [nq][k] indices
	float* normals; const uint32_t* viewStart; const uint32_t* views; const PMFuseCam* cams;   // normal mode
};

// one lane per query; PCA: queries are the sorted points (cell order), else the listed ones
template <int KM, bool PCA>
__global__ __launch_bounds__(256) void pmcl_knn_kernel(PMClGrid g, const float* points, int k, uint32_t nq, PMClKnnOut o) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nq) return;
	const uint32_t qi = PCA ? __float_as_uint(g.spts[t].w) : o.queries[t];
	const float* Xq = points + (size_t)qi * 3;
	const float qx = Xq[0], qy = Xq[1], qz = Xq[2];
	const double dqx = (double)qx, dqy = (double)qy, dqz = (double)qz;
	const double INF = 1.0 / 0.0;
	double D[KM]; uint32_t I[KM];
	// the k-list occupies D[KM-k .. KM-1] (nearest first), so that its k-th entry is D[KM-1], a fixed register; the entries in front of it
	// hold -1, which no distance undercuts, and never move
	#pragma unroll
	for (int j = 0; j < KM; ++j) { D[j] = j < KM - k ? -1. : INF; I[j] = PMCL_NONE; }
	float thr = 1.f / 0.f;
	const int cx = pmcl_axis(dqx, g.ox, g.invh, g.nx), cy = pmcl_axis(dqy, g.oy, g.invh, g.ny), cz = pmcl_axis(dqz, g.oz, g.invh, g.nz);
	auto visit = [&](int x, int y, int z) {
		const uint32_t cell = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx + (uint32_t)x;
		const uint32_t e = g.cellStart[cell + 1];
		for (uint32_t s = g.cellStart[cell]; s < e; ++s) {
			const float4 p = g.spts[s];
			const float fx = p.x - qx, fy = p.y - qy, fz = p.z - qz;
			if ((fx * fx + fy * fy) + fz * fz > thr) continue;          // f32 screen, safe margin (see thr below)
			const double dx = (double)p.x - dqx, dy = (double)p.y - dqy, dz = (double)p.z - dqz;
			const double d = (dx * dx + dy * dy) + dz * dz;
			const uint32_t id = __float_as_uint(p.w);
			if (!pmcl_lt(d, id, D[KM - 1], I[KM - 1])) continue;
			#pragma unroll
			for (int j = KM - 1; j > 0; --j) {
				if (pmcl_lt(d, id, D[j - 1], I[j - 1])) { D[j] = D[j - 1]; I[j] = I[j - 1]; }
				else if (pmcl_lt(d, id, D[j], I[j])) { D[j] = d; I[j] = id; }
			}
			if (pmcl_lt(d, id, D[0], I[0])) { D[0] = d; I[0] = id; }
			const double kth = D[KM - 1];
			// a candidate is skipped only if its f32 distance exceeds the k-th by 1e-4 relative: the f32 distance is within a few 1e-7 of the
			// double one (underflow only lowers it), so a skipped candidate is strictly farther than the k-th
			thr = kth > 1e38 ? 1.f / 0.f : pm_fmaxf((float)kth * 1.0001f, 1e-37f);
		}
	};
	for (int r = 0;; ++r) {
		const int x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r >= g.nx ? g.nx - 1 : cx + r;
		const int y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r >= g.ny ? g.ny - 1 : cy + r;
		const int z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r >= g.nz ? g.nz - 1 : cz + r;
		for (int z = z0; z <= z1; ++z)
			for (int y = y0; y <= y1; ++y) {
				if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) { for (int x = x0; x <= x1; ++x) visit(x, y, z); }
				else { if (cx - r >= 0) visit(cx - r, y, z); if (r > 0 && cx + r < g.nx) visit(cx + r, y, z); }
			}
		// nearest any cell of ring r+1 can be: the distance to the faces of the (2r+1)^3 block, sides without further cells excluded
		double m = INF;
		if (cx - r > 0) m = fmin(m, dqx - (g.ox + (double)(cx - r) * g.h));
		if (cx + r < g.nx - 1) m = fmin(m, (g.ox + (double)(cx + r + 1) * g.h) - dqx);
		if (cy - r > 0) m = fmin(m, dqy - (g.oy + (double)(cy - r) * g.h));
		if (cy + r < g.ny - 1) m = fmin(m, (g.oy + (double)(cy + r + 1) * g.h) - dqy);
		if (cz - r > 0) m = fmin(m, dqz - (g.oz + (double)(cz - r) * g.h));
		if (cz + r < g.nz - 1) m = fmin(m, (g.oz + (double)(cz + r + 1) * g.h) - dqz);
		if (m == INF) break;                                             // the block covers the grid
		m -= g.h * 1e-6;                                                 // cell assignment rounds; never overestimate
		if (m > 0. && m * m > D[KM - 1]) break;                           // strictly farther: an equal distance with a lower index could still enter
	}
	if (!PCA) {
		#pragma unroll
		for (int j = 0; j < KM; ++j) if (j >= KM - k) o.idx[(size_t)t * k + j - (KM - k)] = I[j];
		return;
	}
	const PMFuseCam& cam = o.cams[o.views[o.viewStart[qi]]];
	const float Cf[3] = {(float)cam.C[0], (float)cam.C[1], (float)cam.C[2]};
	pmcl_pca_normal<KM>(points, I, k, Xq, Cf, o.normals + (size_t)qi * 3);
}
