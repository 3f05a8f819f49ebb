// pm_cloud_filter.hip -- Scene::PointCloudFilter(thRemove) (libs/MVS/SceneDensify.cpp:2225-2359 in the reference) and PointCloud::RemoveMinViews
// (PointCloud.cpp:88-93) on the resident cloud (PMFuseOut, see pm_fuse.hip / pm_cloud.hip).
//
// The contract.  For every point i and every view v it lists, a cone from the camera centre O_v = Cast<float>(C_v) through X_i:
//     D = X_i - O_v, distance = sqrt(D.D), dir = D / distance, maxHeight = distance * 1.02f           (Collector::Init, :2258-2266)
// and EVERY point j of the cloud is classified against it (TConeIntersect::Classify, Ray.inl:905-920), all in float, three-term dot products
// summed left to right:
//     E = X_j - O_v, t = dir.E;  counted iff |t| >= 1e-4f, 0 <= t <= maxHeight, t*t > cosAngleSq_v * (E.E), and not |distance - t| / distance < 0.01f
//     visibility[j] += n_j if t > distance, else visibility[j] -= n_i                                  (n = number of views of the point)
// visibility is int32 and only takes integer additions, so it does not depend on the order of the pairs.  The reference reaches its candidates
// through an octree pruned with a conservative cone-sphere test; the sum over all j is what that computes up to the float rounding of the pruning.
// Afterwards RFOREACH(i) if (visibility[i] <= thRemove) RemovePoint(i): the backward swap-remove order of the crop (pm_cloud.hip), whose kernels
// do the removal from the hole flags written here.
//
// The accelerator: one pass per view.  The directions E / |E| of all points are binned on a cube map around O_v: face = the axis of largest |E_k|
// and its sign, (a, b) = the two other components divided by |E_k| (|a|, |b| <= 1), R x R bins of width w = 2 / R per face, every direction
// covered (a view may list a point that lies outside its image or behind it).  The points are counting-sorted by bin (pm_cloud.hip's histogram /
// tile scan / scatter) into (x, y, z, index) with their original float coordinates.  One lane per sorted point that lists v forms its cone and
// visits, on every face f on which its own direction has gnomonic coordinates q = (a_f, b_f) within [-lim, lim]^2, the (2 rad + 1)^2 bins around
// them, rad chosen per lane and face from q (below).
//
// Why no counted candidate is missed.
//  (1) What the float test accepts.  t, t*t, E.E and cosAngleSq * (E.E) carry at most 17 roundings of relative size u = 2^-24 between them, the
//      norm of dir included (products and sums of like-signed terms near the axis; |dir| is 1 within 3u).  So a counted j has a true angle
//      alpha to the axis with sin^2(alpha) <= (1 - cosAngleSq) + 17u, and the axis dir is within 2u radians of D.  PMCLF_SLACK = 1.5e-6 > 17u
//      (1.02e-6) is added to 1 - cosAngleSq and 1e-6 rad to the angle: theta = asin(sqrt(1 - cosAngleSq + 1.5e-6)) + 1e-6 bounds the angle
//      between D and E_j of every counted j (pmclf_plan).  Candidates with t < 0 are never counted, so the cone's mirror image needs no visit.
//      At the 2.1e-4 rad of a 3840-wide view with a 45 degree field the slack is most of theta (1.23e-3): float rounding, not the pixel, sizes the search.
//  (2) Footprint.  The gnomonic map of a face has derivative norm 1 + r^2 at radius r, and along the arc of length <= theta between two directions
//      r stays below tan(atan(r0) + theta) = (r0 + T) / (1 - r0 T), T = tan(theta), r0 the radius of either end.  Take a counted j whose direction
//      lies on face f at c, |c|^2 <= 2.  From c: for theta <= 0.1 the derivative is at most 1 + tan^2(atan(sqrt 2) + 0.1) = 4.13, so q differs
//      from c by less than 4.13 theta on each axis and lies within lim = 1 + 4.5 theta: face f is visited.  From q: the derivative is at most
//      L = 1 + ((|q| + T) / (1 - |q| T))^2, so q and c differ by at most L theta / w bins on each axis.
//  (3) Rounding.  a is one float division, (a + 1) * (R / 2) two more roundings of values <= R <= 2048: an error below 2048 * 2^-22 < 0.0005 bins
//      for either point; T and theta / w are rounded up by 1e-3 and L's float evaluation errs by parts in 1e-6.  rad = floor(L theta / w + 0.02)
//      + 1 exceeds the distance in bins by more than 0.02, so the floors of the two bin coordinates differ by at most rad and j's bin, which
//      lies on its face, is among the (2 rad + 1)^2 around the query's unclamped bin.
//  (4) theta > 0.1 (a cone wider than any camera pixel, test clouds): R = 1 and every lane visits all six bins, that is the whole cloud.
// The bin width is 0.8 theta (R <= 2048): rad is 2 over most of an image and 3 in its corners, 16 to 31 theta^2 searched per cone.
// Each point lies in exactly one bin, and the bins of different faces are different bins, so no candidate is classified twice.
// A direction that is not a number (X_j == O_v, or a query with distance 0) is binned at bin 0 and visits nothing: its t is NaN and never counted.
#pragma once
#include "pm_cloud.hip"

#define PMCLF_SLACK 1.5e-6
#define PMCLF_MAXR 2048

struct PMClfView {
	float ox, oy, oz, cosSq;       // Cast<float>(camera.C), SQUARE(cosf(angle))
	float halfR, lim;              // R / 2, 1 + 4.5 theta
	float T, perBin;               // tan(theta), theta / w in bins, both rounded up
	int R, all;                    // bins per face edge; all: visit every bin (R == 1)
	uint32_t view;
};

// the bin grid of a cone whose cosAngleSq is cosSq (host: once per view)
static inline void pmclf_plan(float cosSq, PMClfView& V) {
	double s2 = 1. - (double)cosSq + PMCLF_SLACK;
	V.all = 1; V.R = 1; V.T = 0.f; V.perBin = 0.f; V.lim = 0.f;
	if (s2 < 0.0099) {                                               // sin^2(0.0996): theta <= 0.1 below
		const double theta = asin(sqrt(s2)) + 1e-6;
		const double r = floor(2. / (0.8 * theta));
		V.R = r > (double)PMCLF_MAXR ? PMCLF_MAXR : (int)r; V.all = 0;
		V.T = (float)(tan(theta) * 1.001); V.perBin = (float)(theta * (double)V.R * 0.5 * 1.001); V.lim = (float)(1. + 4.5 * theta);
	}
	V.halfR = (float)V.R * 0.5f;
}

// gnomonic coordinates of E on cube face f (axis f >> 1, negative side if f & 1); false if E does not point into the face's half-space
PM_HD bool pmclf_face_coords(const float* E, int f, float& a, float& b) {
	const int ax = f >> 1;
	const float m = (f & 1) ? -E[ax] : E[ax];
	if (!(m > 0.f)) return false;
	a = E[ax == 2 ? 0 : ax + 1] / m; b = E[ax == 0 ? 2 : ax - 1] / m;
	return true;
}
PM_HD int pmclf_major_face(const float* E) {
	const float x = pm_fabsf(E[0]), y = pm_fabsf(E[1]), z = pm_fabsf(E[2]);
	const int ax = (x >= y && x >= z) ? 0 : (y >= z ? 1 : 2);
	return ax * 2 + (E[ax] < 0.f ? 1 : 0);
}
PM_HD int pmclf_clampi(float f, int R) { return !(f >= 0.f) ? 0 : f >= (float)R ? R - 1 : (int)f; }   // (NaN -> 0)

PM_HD uint32_t pmclf_bin(const PMClfView& V, const float* X) {
	const float E[3] = {X[0] - V.ox, X[1] - V.oy, X[2] - V.oz};
	const int f = pmclf_major_face(E);
	float a = 0.f, b = 0.f;
	if (!pmclf_face_coords(E, f, a, b)) return 0u;
	const int ia = pmclf_clampi((a + 1.f) * V.halfR, V.R), ib = pmclf_clampi((b + 1.f) * V.halfR, V.R);
	return ((uint32_t)f * (uint32_t)V.R + (uint32_t)ib) * (uint32_t)V.R + (uint32_t)ia;
}

__global__ __launch_bounds__(256) void pmclf_count_kernel(const float* points, uint32_t n, PMClfView V, uint32_t* binOf, uint32_t* counts) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t c = pmclf_bin(V, points + (size_t)i * 3);
		binOf[i] = c;
		atomicAdd(counts + c, 1u);
	}
}

struct PMClfCone { float ox, oy, oz, d0, d1, d2, distance, maxHeight, cosSq; int wi; };

// Classify + IsDepthSimilar + the vote for the sorted points [s0, s1)
PM_HD void pmclf_visit(const PMClfCone& c, const float4* spts, uint32_t s0, uint32_t s1, const uint32_t* viewStart, int mult, int* visibility) {
	for (uint32_t s = s0; s < s1; ++s) {
		const float4 p = spts[s];
		const float e0 = p.x - c.ox, e1 = p.y - c.oy, e2 = p.z - c.oz;
		const float t = (c.d0 * e0 + c.d1 * e1) + c.d2 * e2;
		if (!(pm_fabsf(t) >= 1e-4f)) continue;                           // ISZERO(t): PLANAR
		if (!(t >= 0.f && t <= c.maxHeight)) continue;                   // BACK / FRONT
		const float dSq = c.cosSq * ((e0 * e0 + e1 * e1) + e2 * e2);
		if (!(t * t > dSq)) continue;                                    // CULLED / PLANAR
		if (pm_fabsf(c.distance - t) / c.distance < 0.01f) continue;     // IsDepthSimilar(distance, t, 0.01f)
		const uint32_t j = __float_as_uint(p.w);
		if (t > c.distance) atomicAdd(visibility + j, (int)pmcl_nv(viewStart, j) * mult);
		else atomicAdd(visibility + j, -c.wi * mult);
	}
}

// one lane per sorted point; a point that lists the view `mult` times votes `mult` times.  stats[0] += cones, stats[1] += candidates classified (one atomic per wave)
__global__ __launch_bounds__(256) void pmclf_cone_kernel(PMClfView V, const float4* spts, const uint32_t* binStart, uint32_t n, const uint32_t* viewStart, const uint32_t* views, int* visibility,
                                                         unsigned long long* stats) {
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	int mult = 0;
	uint32_t nCand = 0;
	if (s < n) {
		const float4 q = spts[s];
		const uint32_t i = __float_as_uint(q.w), v0 = viewStart[i], v1 = viewStart[i + 1];
		for (uint32_t v = v0; v < v1; ++v) mult += views[v] == V.view ? 1 : 0;
		if (mult) {
			const float D[3] = {q.x - V.ox, q.y - V.oy, q.z - V.oz};
			PMClfCone c;
			c.ox = V.ox; c.oy = V.oy; c.oz = V.oz; c.cosSq = V.cosSq; c.wi = (int)(v1 - v0);
			c.distance = sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
			c.d0 = D[0] / c.distance; c.d1 = D[1] / c.distance; c.d2 = D[2] / c.distance;
			c.maxHeight = c.distance * 1.02f;
			if (V.all) { pmclf_visit(c, spts, 0u, n, viewStart, mult, visibility); nCand = n; }
			else for (int f = 0; f < 6; ++f) {
				float a, b;
				if (!pmclf_face_coords(D, f, a, b)) continue;
				if (!(pm_fabsf(a) <= V.lim && pm_fabsf(b) <= V.lim)) continue;
				const float rq = sqrtf(a * a + b * b), rp = (rq + V.T) / (1.f - rq * V.T);
				const int rad = (int)((1.f + rp * rp) * V.perBin + 0.02f) + 1;
				const int ia = (int)floorf((a + 1.f) * V.halfR), ib = (int)floorf((b + 1.f) * V.halfR);       // within 6 bins of [0, R)
				const int a0 = ia - rad < 0 ? 0 : ia - rad, a1 = ia + rad >= V.R ? V.R - 1 : ia + rad;
				const int b0 = ib - rad < 0 ? 0 : ib - rad, b1 = ib + rad >= V.R ? V.R - 1 : ib + rad;
				if (a0 > a1 || b0 > b1) continue;
				for (int y = b0; y <= b1; ++y) {
					const uint32_t row = ((uint32_t)f * (uint32_t)V.R + (uint32_t)y) * (uint32_t)V.R;
					const uint32_t s0 = binStart[row + (uint32_t)a0], s1 = binStart[row + (uint32_t)a1 + 1u];   // the bins of a row are consecutive
					pmclf_visit(c, spts, s0, s1, viewStart, mult, visibility);
					nCand += s1 - s0;
				}
			}
		}
	}
	unsigned long long cones = (unsigned long long)mult, cand = (unsigned long long)nCand * (unsigned long long)mult;
	for (int off = 32; off > 0; off >>= 1) { cones += __shfl_down(cones, off); cand += __shfl_down(cand, off); }
	if ((threadIdx.x & 63) == 0 && cones) { atomicAdd(stats, cones); atomicAdd(stats + 1, cand); }
}

// hole flags and the holes per tile (the layout of pmcl_crop_flags): vis != nullptr: visibility[i] <= th; else fewer than nMin views
__global__ __launch_bounds__(PMCL_TB) void pmclf_flags(const int* vis, int th, const uint32_t* viewStart, uint32_t nMin, uint32_t n, uint8_t* hole, uint2* tileSums) {
	__shared__ uint32_t sc[PMCL_TB];
	const uint32_t t = threadIdx.x, b0 = blockIdx.x * PMCL_TILE + t * 4;
	uint32_t cc = 0;
	for (uint32_t k = 0; k < 4; ++k) if (b0 + k < n) {
		const uint8_t h = vis ? (vis[b0 + k] <= th ? 1 : 0) : (pmcl_nv(viewStart, b0 + k) < nMin ? 1 : 0);
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
