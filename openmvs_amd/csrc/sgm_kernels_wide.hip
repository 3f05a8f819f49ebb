// sgm_kernels_wide.hip -- Match for ONE disparity range shared by every pixel and up to SGMHIP_MAX_UNIFORM_DISP (1024) wide: plain SGM
// (SemiGlobalMatcher.cpp:643-684 gives every pixel [minDisp, maxDisp) of the seed's global range, D = 2 (max - min + 16) -- several hundred at 2-12 MP).
//
// The kernels of sgm_kernels.hip stop at 256 disparities: four entries per lane in the line-buffer path kernel, a 256-wide LDS strip in the cost kernel.  Here
//  * the range is two integers: the pixel table that winner-take-all, refinement and get_results read is filled on the device (sgm_fill_uniform_table_kernel);
//  * the cost kernel is sgm_cost_uni_kernel walking the range in slices of SGM_WIDE_SLICE disparities: the left-window prologue once, the strip of the right image
//    reloaded per slice (same 47 KB of LDS), same arithmetic in the same order;
//  * the path kernel is the register-resident recurrence of sgm_path_uniform_kernel with 8 or 16 contiguous entries per lane (D <= 512 / <= 1024): Lp(d-1) and
//    Lp(d+1) across lanes by DPP wave shifts with SGM_INF shifted in at both ends, the wave minimum subtracted, the 64 penalties of a chunk computed at once.
//    A step is ~9 VALU instructions per entry of a lane plus the ~12 of the wave minimum: ~150 for 1024 entries against ~90 (+ ~50 scalar) for 256 entries in
//    sgm_path_kernel<4>.
// Every index into the volumes is 64-bit: a 4K pair at D = 1024 has more than 2^32 costs.
#pragma once
#include "sgm_kernels.hip"

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
typedef const unsigned __attribute__((address_space(1)))* sgm_gcw;
#else
typedef const unsigned* sgm_gcw;
#endif
#define SGM_WIDE_SLICE 256   // disparities per strip of the cost kernel

// PixelData of a uniform problem: idx = pixel * D, [minDisp, maxDisp) -- what the host would upload
__global__ __launch_bounds__(256) void sgm_fill_uniform_table_kernel(SGMPixel* __restrict__ pixels, long nPix, int minDisp, int maxDisp) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nPix; i += (long)gridDim.x * blockDim.x) {
		SGMPixel px; px.idx = (unsigned long long)i * (unsigned long long)(maxDisp - minDisp); px.minDisp = (short)minDisp; px.maxDisp = (short)maxDisp; px.pad = 0;
		pixels[i] = px;
	}
}

// ---- cost volume: sgm_cost_uni_kernel (pair loop) over slices of the range ------------------------------------------------------------------------------
__global__ __launch_bounds__(256, SGM_UNI_WAVES) void sgm_cost_uni_wide_kernel(const unsigned char* __restrict__ colorL, const float* __restrict__ grayL,
		const float* __restrict__ grayR, int w, int h, int vw, int vh, int minDisp, int nDall, unsigned char* __restrict__ costs) {
	constexpr int MD = SGM_WIDE_SLICE, NCOL = 64 + MD + 8, CS = 9;       // (the layout of sgm_cost_uni_kernel<256>)
	__shared__ float s_r[4][NCOL * CS];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tpr = (vw + 63) >> 6;                                     // 64-pixel tiles per row
	const long tile = (long)blockIdx.x * 4 + wave;
	if (tile >= (long)tpr * vh) return;                                 // (no workgroup barrier below: each wave owns its LDS slice)
	const int row = (int)(tile / tpr), col0 = (int)(tile % tpr) * 64, col = col0 + lane;
	const bool have = col < vw;
	const int nD = have ? nDall : 0;
	const unsigned long long idx = (unsigned long long)((long)row * vw + (have ? col : vw - 1)) * (unsigned long long)nDall;
	const unsigned idxLow = (unsigned)(idx & 3ull);
	const int ux = (have ? col : vw - 1) + SGM_HW, uy = row + SGM_HW;
	// left window: weights, weighted mean, t = w * (v - mean), normSq0 (:905-935, the sums in tap order)
	float wk[SGM_NT], tk[SGM_NT];
	float sumW = 0.f, normSq0 = 0.f;
	{
		float acc = 0.f;
#pragma unroll
		for (int n = 0; n < SGM_NT; ++n) {
			const int i = n / 7 - SGM_HW, j = n % 7 - SGM_HW;
			wk[n] = sgm_weight(colorL, w, ux, uy, i, j);
			tk[n] = grayL[(size_t)(uy + i) * w + (ux + j)];
			acc += tk[n] * wk[n]; sumW += wk[n];
		}
		const float tm = acc / sumW;
#pragma unroll
		for (int n = 0; n < SGM_NT; ++n) { const float t = tk[n] - tm; const float tw = wk[n] * t; normSq0 += tw * t; tk[n] = tw; }
	}
	unsigned packed = 0u;
	const float* strip = &s_r[wave][(have ? lane : vw - 1 - col0) * CS];   // a lane without a pixel repeats the row's last one
	auto emit = [&](int k, unsigned c) {                                 // one cost byte into the pixel's run of the volume: collected four to a dword
		if (k < nD) {
			const unsigned pos = (idxLow + (unsigned)k) & 3u;
			packed |= c << (8u * pos);
			if (pos == 3u || k == nD - 1) {
				unsigned char* at = costs + idx + (unsigned)k;
				const unsigned first = (unsigned)k < pos ? pos - (unsigned)k : 0u;
				if (pos == 3u && first == 0u) *reinterpret_cast<unsigned*>(at - 3) = packed;
				else for (unsigned bb = first; bb <= pos; ++bb) at[(int)bb - (int)pos] = (unsigned char)(packed >> (8u * bb));
				packed = 0u;
			}
		}
	};
#pragma unroll 1
	for (int ks = 0; ks < nDall; ks += MD) {
		const int nS = min(MD, nDall - ks);                             // disparities of this slice
		// the strip: columns cb .. cb + 64 + nS + 6 of rows uy-3 .. uy+3 (clamped into the image; a clamped column only feeds costs that are 255 anyway).  Every lane
		// is done with the slice before (a wave's LDS instructions execute in order; the barrier is the emulator's rendezvous)
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		const int cb = col0 + minDisp + ks;
		for (int c = lane; c < 64 + nS + 7; c += 64) {                  // (+1: the pair loop reads one column past an odd slice; that cost is never stored)
			const int cc = cb + c < 0 ? 0 : (cb + c >= w ? w - 1 : cb + c);
#pragma unroll
			for (int i = 0; i < 7; ++i) s_r[wave][c * CS + i] = grayR[(size_t)(uy - SGM_HW + i) * w + cc];
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
#pragma unroll 1
		for (int kk = 0; kk < nS; kk += 2) {                            // two disparities per trip, as sgm_cost_uni_kernel
			float sumA = 0.f, sumSqA = 0.f, nomA = 0.f, sumB = 0.f, sumSqB = 0.f, nomB = 0.f;
			const float* sk = strip + kk * CS;
			float fa[8], fb[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) fa[j] = sk[j * CS];
#pragma unroll
			for (int r = 0; r < 7; ++r) {
				float (&cur)[8] = (r & 1) ? fb : fa;
				float (&nxt)[8] = (r & 1) ? fa : fb;
				if (r < 6) {
#pragma unroll
					for (int j = 0; j < 8; ++j) nxt[j] = sk[j * CS + r + 1];
				}
				SGM_SCHED_BARRIER();
#pragma unroll
				for (int j = 0; j < 7; ++j) {
					const float f = cur[j];
					const float fw = f * wk[r * 7 + j];
					sumA += fw; sumSqA += f * fw; nomA += f * tk[r * 7 + j];
				}
				SGM_PIN3(sumA, sumSqA, nomA);
#pragma unroll
				for (int j = 0; j < 7; ++j) {
					const float f = cur[j + 1];
					const float fw = f * wk[r * 7 + j];
					sumB += fw; sumSqB += f * fw; nomB += f * tk[r * 7 + j];
				}
				SGM_PIN3(sumB, sumSqB, nomB);
				SGM_SCHED_BARRIER();
			}
			const int k = ks + kk, d = minDisp + k;
			const bool inA = !(ux - SGM_HW + d < 0 || ux + SGM_HW + d >= w), inB = !(ux - SGM_HW + d + 1 < 0 || ux + SGM_HW + d + 1 >= w);
			emit(k, inA ? (unsigned)sgm_cost_of(sumA, sumSqA, nomA, sumW, normSq0) : 255u);
			if (kk + 1 < nS) emit(k + 1, inB ? (unsigned)sgm_cost_of(sumB, sumSqB, nomB, sumW, normSq0) : 255u);
		}
	}
}

// ---- 8-path aggregation: sgm_path_uniform_kernel with NK = 8 or 16 contiguous entries per lane ------------------------------------------------------------
// ALIGN: the largest of 4, 2, 1 that divides nD.  idx = pixel * nD and a lane's first entry lane * NK are multiples of it, so a pixel's run is read and its delta
// bytes are written in units of ALIGN bytes that lie wholly inside or wholly outside the range; a unit outside is read from the last unit inside instead (no
// predicate on the loads, nothing read past the volume) and never used.  An odd nD (ALIGN 1) works byte by byte: the plain range is always even.
// DELTA as in sgm_path_uniform_kernel: L - C as a byte per direction, summed by sgm_sum_wta_kernel; otherwise L is added into the u16 sums, two to a 32-bit word --
// with an odd nD every other pixel's sums start on the high half of a word.
template <int NK, int ALIGN, bool DELTA>
__global__ __launch_bounds__(64) void sgm_path_wide_kernel(const float* __restrict__ grayL, int w, int vw, int vh, int nD,
		const unsigned char* __restrict__ costs, unsigned* __restrict__ accumWords, const unsigned short* __restrict__ P2s, int P1, SGMDirs dirs,
		unsigned char* __restrict__ deltas, unsigned long long numCosts) {
	static_assert(NK % 4 == 0 && (ALIGN == 1 || ALIGN == 2 || ALIGN == 4), "a lane's entries are whole dwords of cost bytes");
	constexpr int NW = NK / 4;
	__shared__ unsigned short s_P2[256];
	const int lane = threadIdx.x;
	int dir = 0;
#pragma unroll
	for (int i = 1; i < 8; ++i) dir += (int)blockIdx.x >= dirs.first[i] ? 1 : 0;
	const int line = (int)blockIdx.x - dirs.first[dir];
	const int dx = dirs.dx[dir], dy = dirs.dy[dir];
	const SGMLines ln = dirs.ln[dir];
	int x, y;
	if (line < ln.nA) { x = ln.ax + line * ln.adx; y = ln.ay + line * ln.ady; }
	else { const int i = line - ln.nA; x = ln.bx + i * ln.bdx; y = ln.by + i * ln.bdy; }
	for (int k = lane; k < 256; k += 64) s_P2[k] = P2s[k];
	__syncthreads();
	if (x < 0 || y < 0 || x >= vw || y >= vh) return;
	int n = 0x7fffffff;                                               // pixels on the line
	if (dx > 0) n = min(n, vw - x); else if (dx < 0) n = min(n, x + 1);
	if (dy > 0) n = min(n, vh - y); else if (dy < 0) n = min(n, y + 1);
	const long long idx0 = ((long long)y * vw + x) * nD;              // PixelData::idx of the first pixel, and its step along the line
	const long long dIdx = ((long long)dy * vw + dx) * nD;
	const int k0 = lane * NK;
	auto grayLoad = [&](int i0) -> float {                           // grey value of pixel i0 + lane of the line (valid-grid coordinate on the full image: the reference's quirk, :1078)
		const int i = i0 + lane;
		return i < n ? grayL[(size_t)(y + i * dy) * w + (x + i * dx)] : 0.f;
	};
	// cost bytes of pixels i0 .. i0+SGM_UT-1 of the line, four to a register; the address of a pixel's costs is wave-uniform and pinned to a scalar register pair
	// (see sgm_path_uniform_kernel)
	auto costLoad = [&](int i0, unsigned (*cw)[NW]) {
		unsigned long long base = (unsigned long long)costs + (unsigned long long)(idx0 + (long long)i0 * dIdx);
		const bool all = i0 + SGM_UT <= n;                              // (uniform) all of them on the line
#pragma unroll
		for (int t = 0; t < SGM_UT; ++t) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
			asm volatile("" : "+s"(base));
#endif
#pragma unroll
			for (int j = 0; j < NW; ++j) cw[t][j] = 0u;
			if (all || i0 + t < n) {
				if (ALIGN == 4) {
#pragma unroll
					for (int j = 0; j < NW; ++j) cw[t][j] = ((sgm_gcw)base)[(unsigned)min(k0 + 4 * j, nD - 4) >> 2];
				} else if (ALIGN == 2) {
#pragma unroll
					for (int j = 0; j < NK / 2; ++j) cw[t][j >> 1] |= (unsigned)((sgm_gcs)base)[(unsigned)min(k0 + 2 * j, nD - 2) >> 1] << (16 * (j & 1));
				} else {
#pragma unroll
					for (int q = 0; q < NK; ++q) cw[t][q >> 2] |= (unsigned)((sgm_gcb)base)[(unsigned)min(k0 + q, nD - 1)] << (8 * (q & 3));
				}
			}
			base += (unsigned long long)dIdx;
		}
	};
	int L[NK];
#pragma unroll
	for (int q = 0; q < NK; ++q) L[q] = SGM_INF;
	auto step = [&](int i, int P2, const unsigned* cw) {
		if (i >= n) return;
		const long long idx = idx0 + (long long)i * dIdx;
		int dl[NK];
		if (i == 0) {                                                   // no previous pixel: L = C + P2 (:1012-1021)
#pragma unroll
			for (int q = 0; q < NK; ++q) dl[q] = P2;
		} else {
			int m = L[0];
#pragma unroll
			for (int q = 1; q < NK; ++q) m = min(m, L[q]);
			m = sgm_wave_min(m);
			const int mP2 = m + P2;
			const int fromLeft = __builtin_amdgcn_update_dpp(SGM_INF, L[NK - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1: entry k0-1 (lane 0: none)
			const int fromRight = __builtin_amdgcn_update_dpp(SGM_INF, L[0], 0x130, 0xf, 0xf, false);        // wave_shl:1: entry k0+NK (lane 63: none)
#pragma unroll
			for (int q = 0; q < NK; ++q) {
				const int am = q == 0 ? fromLeft : L[q - 1], ap = q == NK - 1 ? fromRight : L[q + 1];
				dl[q] = min(min(mP2, L[q]), min(am, ap) + P1) - m;
			}
		}
#pragma unroll
		for (int q = 0; q < NK; ++q) L[q] = k0 + q < nD ? (int)((cw[q >> 2] >> (8 * (q & 3))) & 255u) + dl[q] : SGM_INF;
		if (DELTA) {
			unsigned char* out = deltas + (unsigned long long)dir * numCosts + idx + k0;   // numCosts = pixels * nD: a multiple of ALIGN, as idx and k0
			unsigned dw[NW];
#pragma unroll
			for (int j = 0; j < NW; ++j) dw[j] = (unsigned)dl[4 * j] | ((unsigned)dl[4 * j + 1] << 8) | ((unsigned)dl[4 * j + 2] << 16) | ((unsigned)dl[4 * j + 3] << 24);
			if (ALIGN == 4) {
#pragma unroll
				for (int j = 0; j < NW; ++j) if (k0 + 4 * j < nD) reinterpret_cast<unsigned*>(out)[j] = dw[j];
			} else if (ALIGN == 2) {
#pragma unroll
				for (int j = 0; j < NK / 2; ++j) if (k0 + 2 * j < nD) reinterpret_cast<unsigned short*>(out)[j] = (unsigned short)(dw[j >> 1] >> (16 * (j & 1)));
			} else {
#pragma unroll
				for (int q = 0; q < NK; ++q) if (k0 + q < nD) out[q] = (unsigned char)dl[q];
			}
			return;
		}
		// accums(d) += L(d), two sums to an atomic.  par == 0: the lane's entries (2j, 2j+1) are the halves of one word; par == 1 (odd nD, odd pixel): the pairs are
		// (2j+1, 2j+2), the last completed by the next lane's first entry, and entry 0 of the pixel -- the high half of the first word -- adds alone
		unsigned* words = accumWords + (idx >> 1) + (k0 >> 1);
		const unsigned par = ALIGN >= 2 ? 0u : (unsigned)(idx & 1ll);
		unsigned v[NK + 1];
#pragma unroll
		for (int q = 0; q < NK; ++q) v[q] = k0 + q < nD ? (unsigned)L[q] : 0u;
		v[NK] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v[0], 0x130, 0xf, 0xf, false);   // the next lane's first entry (lane 63: none)
		if (par == 0u) {
#pragma unroll
			for (int j = 0; j < NK / 2; ++j) if (k0 + 2 * j < nD) atomicAdd(words + j, v[2 * j] | (v[2 * j + 1] << 16));
		} else {
#pragma unroll
			for (int j = 0; j < NK / 2; ++j) if (k0 + 2 * j + 1 < nD) atomicAdd(words + j + 1, v[2 * j + 1] | (v[2 * j + 2] << 16));
			if (lane == 0) atomicAdd(words, v[0] << 16);
		}
	};
	float g = grayLoad(0), gNext = grayLoad(64);
	float carry = 0.5f;                                               // Ip before the first pixel (:1066)
	unsigned cA[SGM_UT][NW], cB[SGM_UT][NW];
	costLoad(0, cA);
#pragma unroll 1
	for (int i0 = 0; i0 < n; i0 += 64) {
		// the 64 penalties of this chunk: lane t has pixel i0 + t, its predecessor's grey value comes from lane t-1 (lane 0: the chunk before)
		const float Ip = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, carry), __builtin_bit_cast(int, g), 0x138, 0xf, 0xf, false));
		const int P2v = (int)s_P2[sgmp_p2_index(g - Ip)];
		carry = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g), 63));
		g = gNext; gNext = grayLoad(i0 + 128);
#pragma unroll 1
		for (int s = 0; s < 64 && i0 + s < n; s += 2 * SGM_UT) {
			costLoad(i0 + s + SGM_UT, cB);
#pragma unroll
			for (int t = 0; t < SGM_UT; ++t) step(i0 + s + t, __builtin_amdgcn_readlane(P2v, s + t), cA[t]);
			costLoad(i0 + s + 2 * SGM_UT, cA);
#pragma unroll
			for (int t = 0; t < SGM_UT; ++t) step(i0 + s + SGM_UT + t, __builtin_amdgcn_readlane(P2v, s + SGM_UT + t), cB[t]);
		}
	}
}
