// sgm_engine.hip -- host side of libsgmhip.so (include/sgmhip.h).
#include "../../include/sgmhip.h"
#include "sgm_kernels.hip"
#include "sgm_kernels_sub.hip"
#include "sgm_kernels_wide.hip"
#include "sgm_post.hip"
#include "sgm_tsgm.hip"
#include "sgm_rectify.hip"
#include "seed_raster.hip"
#include "hip_buf.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define SGMCHK(e, call) do { hipError_t _r = (call); if (_r != hipSuccess) { (e)->err = std::string(#call) + ": " + hipGetErrorString(_r); return SGMHIP_E_HIP; } } while (0)

struct SGMProblemBufs {   // buffers of the resident problem and what they hold: grown together, never shrunk (sgmReserve)
	size_t capImg = 0, capPix = 0, capCosts = 0;
	DevBuf<unsigned char> d_color; DevBuf<float> d_grayL, d_grayR;
	DevBuf<SGMPixel> d_pixels; DevBuf<unsigned char> d_costs; DevBuf<unsigned short> d_accums;
	DevBuf<short> d_disp; DevBuf<unsigned short> d_cost;
};
struct sgmhip_engine : SGMProblemBufs {
	int device = 0; hipStream_t stream = nullptr; std::string err;
	int w = 0, h = 0, vw = 0, vh = 0, maxNumDisp = 0; uint64_t numCosts = 0;
	DevBuf<unsigned short> d_P2s;
	bool statsOn = false; SGMHipStats stats{};
	DevBuf<unsigned char> d_deltas; size_t capDeltas = 0; int maxP2 = 65535;   // DELTA aggregation (uniform ranges, max P2 <= 255): 8 byte volumes instead of atomic u16 sums
	bool uniformEntry = false;    // the problem came as two integers (sgmhip_set_problem_uniform, the plain loop): 129 .. 256 disparities aggregate with sgm_path_wide_kernel<4> too
	bool uniform = false; int uniformMin = 0, uniformMax = 0; DevBuf<SGMUniform> d_uniform;   // every pixel has [uniformMin, uniformMax) and idx = pixel * nD (checked on the device at set_problem): the register-resident path kernel applies
	int subGroups = 0;            // 0, or the lanes per sub-group (8, 16, 32): Match with the sub-group kernels of sgm_kernels_sub.hip (narrow, ragged ranges); see sgmhip_set_sub_group_kernels
	struct Ev { hipEvent_t a, b; int kind; }; std::vector<Ev> events;
	// the resident scene of the SGM path (sgmhip_scene_*): every image once, each with its own size (w = 0: never set), and the rectified pair of the last
	// sgmhip_rectify_pair (rectW = 0: none) -- BGR, linear gray and validity mask of both sides, grown, never shrunk
	struct SceneImage { DevBuf<unsigned char> bgr; int w = 0, h = 0; }; std::vector<SceneImage> scene;
	DevBuf<unsigned char> d_rectBGR[2], d_rectMask[2]; DevBuf<float> d_rectGray[2], d_srgb; size_t capRect = 0; int rectW = 0, rectH = 0;
	double rectMs = 0; uint64_t rectCalls = 0;     // HIP-event time of the rectification kernel since the last sgmhip_stats_reset
	// the resident seed (include/sgmhip_seed.h): the rasteriser's mesh and keys, the depth map of the last sgmhip_seed_raster (seedW = 0: none) and the initial left
	// disparity of the last sgmhip_seed_disparity (seedDispW = 0: none)
	SeedWork seed; DevBuf<float> d_seedDepth; int seedW = 0, seedH = 0; DevBuf<int16_t> d_seedDisp; int seedDispW = 0, seedDispH = 0;
};
static void sgmFreeSeed(sgmhip_engine* e) {
	hipSetDevice(e->device);
	e->seed.free(); e->d_seedDepth.release(); e->d_seedDisp.release(); e->seedW = e->seedH = e->seedDispW = e->seedDispH = 0;
}

static void sgmFree(sgmhip_engine* e) {
	hipSetDevice(e->device);
	static_cast<SGMProblemBufs&>(*e) = SGMProblemBufs{};
}
static void evB(sgmhip_engine* e, int kind) { if (!e->statsOn) return; sgmhip_engine::Ev ev; ev.kind = kind; hipEventCreate(&ev.a); hipEventCreate(&ev.b); hipEventRecord(ev.a, e->stream); e->events.push_back(ev); }
static void evE(sgmhip_engine* e) { if (!e->statsOn) return; hipEventRecord(e->events.back().b, e->stream); }
static int sgmCollect(sgmhip_engine* e) {
	if (e->events.empty()) return 0;
	SGMCHK(e, hipStreamSynchronize(e->stream));
	for (auto& ev : e->events) { float ms = 0; hipEventElapsedTime(&ms, ev.a, ev.b); (ev.kind == 0 ? e->stats.costMs : ev.kind == 1 ? e->stats.aggrMs : ev.kind == 2 ? e->stats.wtaMs : e->rectMs) += ms; if (ev.kind == 3) ++e->rectCalls; hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
	e->events.clear();
	return 0;
}

// buffers of the resident problem (grown, never shrunk) and its dimensions
static int sgmReserve(sgmhip_engine* e, int w, int h, uint64_t numCosts, int maxNumDisp) {
	const size_t nImg = (size_t)w * h, nPix = (size_t)(w - 2 * SGM_HW) * (h - 2 * SGM_HW);
	if (nImg > e->capImg || nPix > e->capPix || numCosts > e->capCosts) {
		SGMCHK(e, hipStreamSynchronize(e->stream));
		const size_t cI = std::max(nImg, e->capImg), cP = std::max(nPix, e->capPix), cC = std::max<size_t>(numCosts, e->capCosts);
		sgmFree(e);
		SGMCHK(e, e->d_color.alloc(cI * 3)); SGMCHK(e, e->d_grayL.alloc(cI)); SGMCHK(e, e->d_grayR.alloc(cI));
		SGMCHK(e, e->d_pixels.alloc(cP)); SGMCHK(e, e->d_disp.alloc(cP)); SGMCHK(e, e->d_cost.alloc(cP));
		SGMCHK(e, e->d_costs.alloc(cC + 256)); SGMCHK(e, e->d_accums.alloc((cC + 3) / 4 * 4 + 4)); // u16 sums, addressed as 32-bit words by the path kernels
		e->capImg = cI; e->capPix = cP; e->capCosts = cC;
	}
	e->w = w; e->h = h; e->vw = w - 2 * SGM_HW; e->vh = h - 2 * SGM_HW; e->numCosts = numCosts; e->maxNumDisp = maxNumDisp;
	e->uniform = false; e->uniformEntry = false;
	return 0;
}

extern "C" {

int sgmhip_create(int device, sgmhip_engine** out) {
	if (!out) return SGMHIP_E_ARG;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) return SGMHIP_E_NODEVICE;
	if (device < 0) device = 0;
	sgmhip_engine* e = new sgmhip_engine(); e->device = device;
	if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess || e->d_P2s.alloc(256) != hipSuccess) { delete e; return SGMHIP_E_HIP; }
	*out = e;
	return 0;
}
void sgmhip_destroy(sgmhip_engine* e) {
	if (!e) return;
	hipSetDevice(e->device); hipStreamSynchronize(e->stream);
	for (auto& ev : e->events) { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
	sgmFree(e); e->d_P2s.release(); e->d_uniform.release(); e->d_deltas.release();
	sgmFreeSeed(e);
	e->scene.clear(); e->d_srgb.release(); for (int s = 0; s < 2; ++s) { e->d_rectBGR[s].release(); e->d_rectGray[s].release(); e->d_rectMask[s].release(); }
	hipStreamDestroy(e->stream); delete e;
}
const char* sgmhip_last_error(sgmhip_engine* e) { return e ? e->err.c_str() : "null engine"; }

int sgmhip_generate_p2s(uint16_t P2, float alpha, float beta, uint16_t out256[256]) {
	if (!out256) return SGMHIP_E_ARG;
	for (int i = 0; i < 256; ++i) { const float fi = (float)i; out256[i] = (uint16_t)(int)floorf((float)P2 * (1.f + alpha * pm_expf(-(fi * fi) / (2.f * (beta * beta)))) + .5f); }
	return 0;
}

int sgmhip_set_problem(sgmhip_engine* e, const uint8_t* leftBGR, const float* leftGray, const float* rightGray, int w, int h,
		const SGMHipPixelData* pixels, uint64_t numCosts, int maxNumDisp) {
	if (!e || !leftBGR || !leftGray || !rightGray || !pixels || w <= 2 * SGM_HW || h <= 2 * SGM_HW || numCosts == 0 || maxNumDisp <= 0 || maxNumDisp > 256) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	const size_t nImg = (size_t)w * h, nPix = (size_t)(w - 2 * SGM_HW) * (h - 2 * SGM_HW);
	{ const int rc = sgmReserve(e, w, h, numCosts, maxNumDisp); if (rc) return rc; }
	SGMCHK(e, hipMemcpyAsync(e->d_color, leftBGR, nImg * 3, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemcpyAsync(e->d_grayL, leftGray, nImg * 4, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemcpyAsync(e->d_grayR, rightGray, nImg * 4, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemcpyAsync(e->d_pixels, pixels, nPix * sizeof(SGMPixel), hipMemcpyHostToDevice, e->stream));
	// one range for all pixels?  (then Match takes the strip cost kernel and aggregates with sgm_path_uniform_kernel)
	SGMUniform hu = {1, 0, 0, 0};
	if (!e->d_uniform) SGMCHK(e, e->d_uniform.alloc(1));
	SGMCHK(e, hipMemcpyAsync(e->d_uniform, &hu, sizeof(hu), hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(sgm_uniform_check_kernel, dim3((unsigned)((nPix + 255) / 256)), dim3(256), 0, e->stream, e->d_pixels, (long)nPix, e->d_uniform);
	SGMCHK(e, hipMemcpyAsync(&hu, e->d_uniform, sizeof(hu), hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	e->uniform = hu.ok != 0 && hu.maxDisp - hu.minDisp == maxNumDisp && (uint64_t)nPix * (uint64_t)maxNumDisp == numCosts;
	e->uniformMin = hu.minDisp; e->uniformMax = hu.maxDisp;
	return 0;
}

// the resident problem becomes the uniform one of [minDisp, maxDisp): buffers for w x h and its pixels * D costs, the pixel table filled on the device (asynchronous;
// the images are the caller's to copy in).  An error leaves no problem resident.
static int sgmReserveUniform(sgmhip_engine* e, int w, int h, int minDisp, int maxDisp) {
	const int D = maxDisp - minDisp;
	const size_t nPix = (size_t)(w - 2 * SGM_HW) * (h - 2 * SGM_HW);
	const int rc = sgmReserve(e, w, h, (uint64_t)nPix * (uint64_t)D, D);
	if (rc) { e->numCosts = 0; (void)hipGetLastError(); return rc; }
	hipLaunchKernelGGL(sgm_fill_uniform_table_kernel, dim3((unsigned)std::min<size_t>((nPix + 255) / 256, 65535)), dim3(256), 0, e->stream, e->d_pixels.p, (long)nPix, minDisp, maxDisp);
	e->uniform = true; e->uniformEntry = true; e->uniformMin = minDisp; e->uniformMax = maxDisp;
	return 0;
}
// why [minDisp, maxDisp) cannot be a uniform problem ("" if it can): the text every entry point reports
static std::string sgmUniformRefusal(long long minDisp, long long maxDisp) {
	const long long D = maxDisp - minDisp;
	if (D < 1 || D > SGMHIP_MAX_UNIFORM_DISP) return "a uniform range of " + std::to_string(D) + " disparities: it must hold 1 .. " + std::to_string(SGMHIP_MAX_UNIFORM_DISP) + " (SGMHIP_MAX_UNIFORM_DISP)";
	if (minDisp < -32767 || maxDisp > 32767) return "a uniform range [" + std::to_string(minDisp) + ", " + std::to_string(maxDisp) + ") leaves int16 (or its negation does)";
	return "";
}

int sgmhip_set_problem_uniform(sgmhip_engine* e, const uint8_t* leftBGR, const float* leftGray, const float* rightGray, int w, int h, int minDisp, int maxDisp) {
	if (!e) return SGMHIP_E_ARG;
	if (!leftBGR || !leftGray || !rightGray || w <= 2 * SGM_HW || h <= 2 * SGM_HW) { e->err = "set_problem_uniform: null image, or an image no larger than the 7x7 window"; return SGMHIP_E_ARG; }
	{ const std::string why = sgmUniformRefusal(minDisp, maxDisp); if (!why.empty()) { e->err = "set_problem_uniform: " + why; return SGMHIP_E_ARG; } }
	SGMCHK(e, hipSetDevice(e->device));
	const size_t nImg = (size_t)w * h;
	{ const int rc = sgmReserveUniform(e, w, h, minDisp, maxDisp); if (rc) return rc; }
	SGMCHK(e, hipMemcpyAsync(e->d_color, leftBGR, nImg * 3, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemcpyAsync(e->d_grayL, leftGray, nImg * 4, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemcpyAsync(e->d_grayR, rightGray, nImg * 4, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));                       // the images are the caller's memory
	return 0;
}

int sgmhip_plain_range(const int16_t* seed, size_t n, int16_t* minDisp, int16_t* maxDisp) {
	if (!seed || n == 0 || !minDisp || !maxDisp) return SGMHIP_E_ARG;
	int16_t mn = seed[0], mx = seed[0];
	for (size_t i = 1; i < n; ++i) { mn = std::min(mn, seed[i]); mx = std::max(mx, seed[i]); }
	// every intermediate is a Disparity (:645-661): the conversions wrap
	const int16_t numDisp = (int16_t)((int16_t)(mx - mn) + 16);
	const int16_t disp = (int16_t)(mn + mx);
	*minDisp = (int16_t)(disp - numDisp); *maxDisp = (int16_t)(disp + numDisp);
	return 0;
}

// the penalty table of the next Match on the device, and its maximum (which decides between byte deltas and u16 atomic sums).  Penalties that Match would get
// silently wrong are refused here, for sgmhip_match and both resident tSGM entry points alike (nothing has been changed or launched when this returns an error):
//  * P1 above an entry of P2s: the kernels evaluate the recurrence in its O(D) form, min(Lp(d), Lp(d+-1) + P1, min Lp + P2), which equals the reference's loop over all
//    previous disparities only when P1 <= P2 (oracle/sgm_oracle.cpp: orc_sgm_step_forms_agree);
//  * an entry with 8 * (255 + P2) > 65535, i.e. above 7936: a path's L is at most 255 + P2, the sum of the eight paths is the reference's u16 and, on the device, half of
//    a 32-bit word that two neighbouring sums share in one atomic add without carry.
static int sgmSetP2s(sgmhip_engine* e, uint16_t P1, const uint16_t P2s[256]) {
	const int minP2 = *std::min_element(P2s, P2s + 256), maxP2 = *std::max_element(P2s, P2s + 256);
	if ((int)P1 > minP2) { e->err = "P1 = " + std::to_string((int)P1) + " exceeds the smallest entry of P2s (" + std::to_string(minP2) + "): Match needs P1 <= P2"; return SGMHIP_E_ARG; }
	if (!SGMP_SUM_FITS_U16(maxP2)) { e->err = "an entry of P2s is " + std::to_string(maxP2) + ": Match needs 8 * (255 + P2) <= 65535, the sum of eight paths in 16 bits"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipMemcpyAsync(e->d_P2s, P2s, 512, hipMemcpyHostToDevice, e->stream));
	e->maxP2 = *std::max_element(P2s, P2s + 256);
	return 0;
}
// the 8 byte volumes of the DELTA aggregation (kept between calls, grown on demand); false: no room, the caller takes the atomic path
static bool ensureDeltas(sgmhip_engine* e) {
	if (e->capDeltas >= e->numCosts * 8) return true;
	if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
	e->capDeltas = 0;
	if (e->d_deltas.alloc(e->numCosts * 8 + 16) == hipSuccess) { e->capDeltas = e->numCosts * 8; return true; }
	(void)hipGetLastError();
	return false;
}

// the eight paths with the threaded variant's start sets (SemiGlobalMatcher.cpp:1083-1200) as one grid, `linesPerGroup` lines to a workgroup
// (first[] counts workgroups); -> the number of workgroups
static int sgmSchedule(int W, int H, int linesPerGroup, SGMDirs& sd) {
	const struct Dir { int dx, dy; SGMLines ln; } dirs[8] = {
		{0, 1,   {W, 0, 0, 1, 0,      0, 0, 0, 0, 0}},            // width-down
		{1, 0,   {H, 0, 0, 0, 1,      0, 0, 0, 0, 0}},            // height-right
		{0, -1,  {W, 0, H - 1, 1, 0,  0, 0, 0, 0, 0}},            // width-up
		{-1, 0,  {H, W - 1, 0, 0, 1,  0, 0, 0, 0, 0}},            // height-left
		{1, 1,   {W, 0, 0, 1, 0,      H - 1, 0, 1, 0, 1}},        // right-down: top row, then left column y >= 1
		{-1, 1,  {W - 1, 0, 0, 1, 0,  H, W - 1, 0, 0, 1}},        // left-down: top row x < W-1, then right column
		{1, -1,  {W - 1, 1, H - 1, 1, 0,  H, 0, 0, 0, 1}},        // right-up: bottom row x >= 1, then left column
		{-1, -1, {W, 0, H - 1, 1, 0,  H - 1, W - 1, 0, 0, 1}},    // left-up: bottom row, then right column y <= H-2
	};
	// the directions with the longest lines first (their chains bound the kernel's duration)
	const int horizFirst[8] = {1, 3, 0, 2, 4, 5, 6, 7}, vertFirst[8] = {0, 2, 1, 3, 4, 5, 6, 7};
	const int* ord = W >= H ? horizFirst : vertFirst;
	memset(&sd, 0, sizeof(sd));
	int total = 0;
	for (int i = 0; i < 8; ++i) {
		const Dir& d = dirs[ord[i]];
		sd.dx[i] = d.dx; sd.dy[i] = d.dy; sd.ln[i] = d.ln; sd.first[i] = total;
		total += (d.ln.nA + d.ln.nB + linesPerGroup - 1) / linesPerGroup;
	}
	sd.first[8] = total;
	return total;
}

extern "C++" {
// the path kernel of the resident problem.  DL: L - C <= P2 as a byte per direction (a coalesced store per lane and step) instead of an atomic add into
// the shared u16 sums
template <bool DL>
static void sgmLaunchPaths(sgmhip_engine* e, int P1, const SGMDirs& sd, int total) {
	const int D = e->maxNumDisp, NK = D <= 64 ? 1 : (D <= 128 ? 2 : 4);
#define SGM_PATH_TAIL e->d_costs, (unsigned*)e->d_accums.p, e->d_P2s, P1, sd, e->d_deltas, (unsigned long long)e->numCosts
#define SGM_RAGGED(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(total), dim3(64), 0, e->stream, e->d_grayL, e->w, e->vw, e->vh, e->d_pixels, SGM_PATH_TAIL)
#define SGM_UNIFORM(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(total), dim3(64), 0, e->stream, e->d_grayL, e->w, e->vw, e->vh, D, SGM_PATH_TAIL)
#define SGM_SUB(LP_) do { if (D <= 64) SGM_RAGGED(sgm_path_sub_kernel<LP_, 64, DL>); else SGM_RAGGED(sgm_path_sub_kernel<LP_, 256, DL>); } while (0)
	if (e->subGroups == 8) SGM_SUB(8);
	else if (e->subGroups == 32) SGM_SUB(32);
	else if (e->subGroups) SGM_SUB(16);
	else if (e->uniform && NK <= 2) {   // the previous line of L in registers
		if (DL && D % 16 == 0) {        // delta bytes staged through LDS, written out 16 bytes at a time
			if (NK == 1) SGM_UNIFORM(sgm_path_uniform_kernel<1, 2, true, true>); else SGM_UNIFORM(sgm_path_uniform_kernel<2, 2, true, true>);
		} else if (D % 2 == 0) {
			if (NK == 1) SGM_UNIFORM(sgm_path_uniform_kernel<1, 2, DL, false>); else SGM_UNIFORM(sgm_path_uniform_kernel<2, 2, DL, false>);
		} else {
			if (NK == 1) SGM_UNIFORM(sgm_path_uniform_kernel<1, 1, DL, false>); else SGM_UNIFORM(sgm_path_uniform_kernel<2, 1, DL, false>);
		}
	}
	else if (NK == 1) SGM_RAGGED(sgm_path_kernel<1, DL>);
	else if (NK == 2) SGM_RAGGED(sgm_path_kernel<2, DL>);
	else SGM_RAGGED(sgm_path_kernel<4, DL>);
#undef SGM_SUB
#undef SGM_UNIFORM
#undef SGM_RAGGED
#undef SGM_PATH_TAIL
}
// the path kernel of a uniform range of more than 256 disparities (sgm_kernels_wide.hip): 8 entries per lane up to 512, 16 beyond; 4 for the 129 .. 256 of a problem
// stated as two integers, where sgm_path_kernel<4> would serve (measured at 2048x1536, D = 256: profiles/plain_sgm_bench.log)
template <bool DL>
static void sgmLaunchPathsWide(sgmhip_engine* e, int P1, const SGMDirs& sd, int total) {
	const int D = e->maxNumDisp;
#define SGM_WIDE(NK_, A_) hipLaunchKernelGGL((sgm_path_wide_kernel<NK_, A_, DL>), dim3(total), dim3(64), 0, e->stream, e->d_grayL, e->w, e->vw, e->vh, D, \
		e->d_costs, (unsigned*)e->d_accums.p, e->d_P2s, P1, sd, e->d_deltas, (unsigned long long)e->numCosts)
#define SGM_WIDE_A(NK_) do { if (D % 4 == 0) SGM_WIDE(NK_, 4); else if (D % 2 == 0) SGM_WIDE(NK_, 2); else SGM_WIDE(NK_, 1); } while (0)
	if (D <= 256) SGM_WIDE_A(4); else if (D <= 512) SGM_WIDE_A(8); else SGM_WIDE_A(16);
#undef SGM_WIDE_A
#undef SGM_WIDE
}
} // extern "C++"

// cost volume, 8-path aggregation and winner-take-all of the resident problem (P2s already on the device: sgmSetP2s), asynchronous on the engine's stream.
// Two mappings of work to lanes: one wavefront per line (subGroups == 0), or sub-groups of subGroups lanes per line and per pixel (sgm_kernels_sub.hip)
static int sgmMatch(sgmhip_engine* e, uint16_t P1) {
	const bool wide = e->maxNumDisp > 256;                           // only a uniform range gets here (sgmhip_set_problem_uniform): one wavefront per line, whatever subGroups says
	const int W = e->vw, H = e->vh, LP = wide ? 0 : e->subGroups;
	const long nPix = (long)W * H;
	// cost volume: one pixel per lane, 64-pixel tiles of a row per wave -- it serves the narrow ranges of the sub-group mapping too (0.9 against 1.28 ms of a
	// sub-group per pixel pair for 3-12 disparities per pixel at 2048x1536).  One range for all pixels (wide mapping): the right-image strip of a tile sits in LDS
	evB(e, 0);
	{
		const long nTiles = (long)((W + 63) / 64) * H;
		const dim3 g((unsigned)((nTiles + 3) / 4));
		if (wide) hipLaunchKernelGGL(sgm_cost_uni_wide_kernel, g, dim3(256), 0, e->stream, e->d_color, e->d_grayL, e->d_grayR, e->w, e->h, W, H, e->uniformMin, e->maxNumDisp, e->d_costs);
		else if (e->uniform && !LP) {
#define SGM_LAUNCH_UNI(MD_) hipLaunchKernelGGL((sgm_cost_uni_kernel<MD_>), g, dim3(256), 0, e->stream, e->d_color, e->d_grayL, e->d_grayR, e->w, e->h, W, H, e->uniformMin, e->maxNumDisp, e->d_costs)
			if (e->maxNumDisp <= 64) SGM_LAUNCH_UNI(64); else if (e->maxNumDisp <= 128) SGM_LAUNCH_UNI(128); else SGM_LAUNCH_UNI(256);
#undef SGM_LAUNCH_UNI
		} else hipLaunchKernelGGL(sgm_cost_px_kernel, g, dim3(256), 0, e->stream, e->d_color, e->d_grayL, e->d_grayR, e->w, e->h, W, H, e->d_pixels, e->d_costs);
	}
	evE(e);
	// DELTA aggregation: penalties that fit a byte (L - C <= P2), 8 scratch bytes per entry; no room for them: the atomic path
	const bool delta = e->maxP2 <= 255 && ensureDeltas(e);
	if (!delta) SGMCHK(e, hipMemsetAsync(e->d_accums, 0, (e->numCosts + 1) / 2 * 4, e->stream)); // imageAccumCosts.Memset(0), :990
	SGMDirs sd;
	const int total = sgmSchedule(W, H, LP ? 64 / LP : 1, sd);
	evB(e, 1);
	if (total > 0 && (wide || (e->uniformEntry && !LP && e->maxNumDisp > 128))) { if (delta) sgmLaunchPathsWide<true>(e, (int)P1, sd, total); else sgmLaunchPathsWide<false>(e, (int)P1, sd, total); }
	else if (total > 0) { if (delta) sgmLaunchPaths<true>(e, (int)P1, sd, total); else sgmLaunchPaths<false>(e, (int)P1, sd, total); }
	if (e->statsOn) e->stats.aggrLaunches += 1;
	evE(e);
	evB(e, 2);
	if (delta) hipLaunchKernelGGL(sgm_sum_wta_kernel, dim3((unsigned)((nPix + 15) / 16)), dim3(256), 0, e->stream, e->d_pixels, e->d_costs, e->d_deltas, (unsigned long long)e->numCosts, e->d_accums, nPix, e->d_disp, e->d_cost);
	else {
		// winner-take-all over the atomic sums: a sub-group of lanes per pixel with a strided loop over its range.  The wide mapping takes 8 lanes: a wider group spends its
		// instructions on the cross-lane reduction (measured: 0.72 / 0.33 / 0.20 / 0.14 ms at 64 / 32 / 16 / 8 lanes, profiles/r02_sgm_wta_lanes.log)
		const int lanes = LP ? LP : 8;
		const dim3 g((unsigned)((nPix + 4 * (64 / lanes) - 1) / (4 * (64 / lanes))));
#define SGM_LAUNCH_WTA(LP_) hipLaunchKernelGGL((sgm_wta_sub_kernel<LP_>), g, dim3(256), 0, e->stream, e->d_pixels, e->d_accums, nPix, e->d_disp, e->d_cost)
		if (lanes == 8) SGM_LAUNCH_WTA(8); else if (lanes == 32) SGM_LAUNCH_WTA(32); else SGM_LAUNCH_WTA(16);
#undef SGM_LAUNCH_WTA
	}
	evE(e);
	SGMCHK(e, hipGetLastError());
	if (e->statsOn) e->stats.calls += 1;
	return 0;
}

int sgmhip_match(sgmhip_engine* e, uint16_t P1, const uint16_t P2s[256], int sync) {
	if (!e || !P2s || e->numCosts == 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	{ const int rc = sgmSetP2s(e, P1, P2s); if (rc) return rc; }
	{ const int rc = sgmMatch(e, P1); if (rc) return rc; }
	if (sync) SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_get_results(sgmhip_engine* e, int16_t* disparity, uint16_t* cost, uint8_t* costs, uint16_t* accums) {
	if (!e || e->numCosts == 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	const size_t nPix = (size_t)e->vw * e->vh;
	if (disparity) SGMCHK(e, hipMemcpyAsync(disparity, e->d_disp, nPix * 2, hipMemcpyDeviceToHost, e->stream));
	if (cost) SGMCHK(e, hipMemcpyAsync(cost, e->d_cost, nPix * 2, hipMemcpyDeviceToHost, e->stream));
	if (costs) SGMCHK(e, hipMemcpyAsync(costs, e->d_costs, e->numCosts, hipMemcpyDeviceToHost, e->stream));
	if (accums) SGMCHK(e, hipMemcpyAsync(accums, e->d_accums, e->numCosts * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}
int sgmhip_set_sub_group_kernels(sgmhip_engine* e, int lanes) {
	if (!e || (lanes != 0 && lanes != 1 && lanes != 8 && lanes != 16 && lanes != 32)) return SGMHIP_E_ARG;
	e->subGroups = lanes == 1 ? 16 : lanes;
	return 0;
}
int sgmhip_sync(sgmhip_engine* e) { if (!e) return SGMHIP_E_ARG; SGMCHK(e, hipSetDevice(e->device)); SGMCHK(e, hipStreamSynchronize(e->stream)); return 0; }
int sgmhip_stats_reset(sgmhip_engine* e, int enable) { if (!e) return SGMHIP_E_ARG; hipSetDevice(e->device); sgmCollect(e); memset(&e->stats, 0, sizeof(e->stats)); e->rectMs = 0; e->rectCalls = 0; e->statsOn = enable != 0; return 0; }
int sgmhip_stats_get(sgmhip_engine* e, SGMHipStats* out) { if (!e || !out) return SGMHIP_E_ARG; hipSetDevice(e->device); int rc = sgmCollect(e); if (rc) return rc; *out = e->stats; return 0; }

// ---- tSGM steps around Match (SemiGlobalMatcher.cpp:1449-1811), see csrc/sgm_post.h ---------------------------------------------
namespace {
using Scoped = DevBuf<unsigned char>;   // scoped device allocation (bytes) for the stateless helpers
inline unsigned gridFor(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 65535); }

// The steps that both a stateless call (upload, step, download) and a resident loop run: device pointers in, launches on `st`, nothing else.
// FlipDirection: keys is scratch of w * h words
hipError_t sgmFlip(hipStream_t st, const int16_t* l2r, int w, int h, uint32_t* keys, int16_t* r2l) {
	const size_t n = (size_t)w * h;
	const hipError_t r = hipMemsetAsync(keys, 0, n * 4, st);
	if (r != hipSuccess) return r;
	hipLaunchKernelGGL(sgmp_flip_scatter_kernel, dim3(gridFor(n)), dim3(256), 0, st, l2r, keys, w, h);
	hipLaunchKernelGGL(sgmp_flip_decode_kernel, dim3(gridFor(n)), dim3(256), 0, st, (const uint32_t*)keys, r2l, n);
	return hipSuccess;
}
// the speckle filter, in place: parent and size are scratch of w * h ints each
void sgmSpeckles(hipStream_t st, int16_t* disp, int w, int h, int maxSpeckleSize, int maxDiff, int* parent, int* size) {
	const int n = w * h; const unsigned g = gridFor((size_t)n);
	hipLaunchKernelGGL(sgmp_speckle_init_kernel, dim3(g), dim3(256), 0, st, parent, size, n);
	hipLaunchKernelGGL(sgmp_speckle_hook_kernel, dim3(g), dim3(256), 0, st, (const int16_t*)disp, parent, w, h, maxDiff);
	hipLaunchKernelGGL(sgmp_speckle_flatten_kernel, dim3(g), dim3(256), 0, st, parent, size, n);
	hipLaunchKernelGGL(sgmp_speckle_apply_kernel, dim3(g), dim3(256), 0, st, disp, (const int*)parent, (const int*)size, n, maxSpeckleSize);
}
// the device part of Disparity2RangeMap: the range of every pixel of a w x h disparity map
void sgmRanges(hipStream_t st, const int16_t* disp, int w, int h, const uint8_t* mask2x, int w2, int minNumDisp, int minNumDispInvalid, short2* ranges) {
	hipLaunchKernelGGL(sgmp_range_kernel, dim3(gridFor((size_t)w * h)), dim3(256), 0, st, disp, w, h, mask2x, w2, minNumDisp, minNumDispInvalid, ranges);
}
// ProjectDisparity2DepthMap of one pair (cost and conf may both be null): keys is scratch of dw * dh * 4 words, *numDepths (cleared by the caller) counts the depths
hipError_t sgmProject(hipStream_t st, const int16_t* disp, const uint16_t* cost, int w, int h, const double Q[16], int subpixelSteps, unsigned long long* keys, int dw, int dh,
		float* depth, float* range2, float* conf, unsigned* numDepths) {
	const size_t n = (size_t)w * h, nd = (size_t)dw * dh;
	const hipError_t r = hipMemsetAsync(range2, 0, nd * 8, st);
	if (r != hipSuccess) return r;
	SGMPMat mq{}; memcpy(mq.m, Q, 128);
	hipLaunchKernelGGL(sgmp_fill_u64, dim3(gridFor(nd * 4)), dim3(256), 0, st, keys, nd * 4, SGMP_KEY_NONE);
	hipLaunchKernelGGL(sgmp_proj_splat_kernel, dim3(gridFor(n)), dim3(256), 0, st, disp, cost, w, h, mq, subpixelSteps, keys, dw, dh);
	hipLaunchKernelGGL(sgmp_proj_resolve_kernel, dim3(gridFor(nd)), dim3(256), 0, st, disp, cost, w, mq, subpixelSteps, (const unsigned long long*)keys, dw, dh, depth, range2, conf, numDepths);
	return hipSuccess;
}
}

int sgmhip_consistency_cross_check(sgmhip_engine* e, int16_t* l2r, const int16_t* r2l, int wl, int h, int wr, int thCross) {
	if (!e || !l2r || !r2l || wl <= 0 || wr <= 0 || h <= 0 || thCross < 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, b; const size_t nl = (size_t)wl * h, nr = (size_t)wr * h;
	SGMCHK(e, a.alloc(nl * 2)); SGMCHK(e, b.alloc(nr * 2));
	SGMCHK(e, hipMemcpyAsync(a.p, l2r, nl * 2, hipMemcpyHostToDevice, e->stream)); SGMCHK(e, hipMemcpyAsync(b.p, r2l, nr * 2, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(sgmp_cross_check_kernel, dim3(gridFor(nl)), dim3(256), 0, e->stream, (int16_t*)a.p, (const int16_t*)b.p, wl, wr, h, thCross);
	SGMCHK(e, hipMemcpyAsync(l2r, a.p, nl * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_filter_by_cost(sgmhip_engine* e, int16_t* disparity, const uint16_t* cost, int w, int h, uint16_t th) {
	if (!e || !disparity || !cost || w <= 0 || h <= 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, b; const size_t n = (size_t)w * h;
	SGMCHK(e, a.alloc(n * 2)); SGMCHK(e, b.alloc(n * 2));
	SGMCHK(e, hipMemcpyAsync(a.p, disparity, n * 2, hipMemcpyHostToDevice, e->stream)); SGMCHK(e, hipMemcpyAsync(b.p, cost, n * 2, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(sgmp_filter_by_cost_kernel, dim3(gridFor(n)), dim3(256), 0, e->stream, (int16_t*)a.p, (const uint16_t*)b.p, n, th);
	SGMCHK(e, hipMemcpyAsync(disparity, a.p, n * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_extract_mask(sgmhip_engine* e, const int16_t* disparity, uint8_t* mask, int w, int h, int thValid, int initValid) {
	if (!e || !disparity || !mask || w <= 0 || h <= 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, b; const size_t n = (size_t)w * h;
	SGMCHK(e, a.alloc(n * 2)); SGMCHK(e, b.alloc(n));
	SGMCHK(e, hipMemcpyAsync(a.p, disparity, n * 2, hipMemcpyHostToDevice, e->stream));
	if (initValid) SGMCHK(e, hipMemsetAsync(b.p, 0xFF, n, e->stream));      // maskMap.create(size); setTo(VALID), :1521-1524
	else SGMCHK(e, hipMemcpyAsync(b.p, mask, n, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(sgmp_extract_mask_kernel, dim3((h + 63) / 64), dim3(64), 0, e->stream, (const int16_t*)a.p, (uint8_t*)b.p, w, h, thValid);
	SGMCHK(e, hipMemcpyAsync(mask, b.p, n, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_upscale_mask(sgmhip_engine* e, const uint8_t* mask, int w, int h, uint8_t* mask2x, int w2, int h2) {
	if (!e || !mask || !mask2x || w <= 0 || h <= 0 || w2 <= 0 || h2 <= 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, b; const size_t n = (size_t)w * h, n2 = (size_t)w2 * h2;
	SGMCHK(e, a.alloc(n)); SGMCHK(e, b.alloc(n2));
	SGMCHK(e, hipMemcpyAsync(a.p, mask, n, hipMemcpyHostToDevice, e->stream));
	hipLaunchKernelGGL(sgmp_upscale_mask_kernel, dim3(gridFor(n2)), dim3(256), 0, e->stream, (const uint8_t*)a.p, w, h, (uint8_t*)b.p, w2, h2);
	SGMCHK(e, hipMemcpyAsync(mask2x, b.p, n2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_flip_direction(sgmhip_engine* e, const int16_t* l2r, int w, int h, int16_t* r2l) {
	if (!e || !l2r || !r2l || w <= 0 || h <= 0 || w > 65534) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	DevBuf<int16_t> a, b; DevBuf<uint32_t> k; const size_t n = (size_t)w * h;
	SGMCHK(e, a.alloc(n)); SGMCHK(e, k.alloc(n)); SGMCHK(e, b.alloc(n));
	SGMCHK(e, hipMemcpyAsync(a, l2r, n * 2, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, sgmFlip(e->stream, a, w, h, k, b));
	SGMCHK(e, hipMemcpyAsync(r2l, b, n * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_refine_disparity(sgmhip_engine* e, int subpixelMode, int subpixelSteps) {
	if (!e || e->numCosts == 0 || subpixelMode < 0 || subpixelMode > SGMP_SUBPIXEL_LC_BLEND || subpixelSteps < 0 || subpixelSteps > 64) return SGMHIP_E_ARG;
	if (subpixelSteps <= 1) return 0;                                     // :1696-1697
	SGMCHK(e, hipSetDevice(e->device));
	const long nPix = (long)e->vw * e->vh;
	hipLaunchKernelGGL(sgmp_refine_kernel, dim3(gridFor((size_t)nPix)), dim3(256), 0, e->stream, e->d_pixels, e->d_accums, nPix, e->d_disp, subpixelMode, subpixelSteps);
	SGMCHK(e, hipGetLastError());
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_disparity2range_map(sgmhip_engine* e, const int16_t* disparity, int w, int h, const uint8_t* mask2x, int w2, int h2,
		int minNumDisp, int minNumDispInvalid, SGMHipPixelData* pixels, uint64_t* numCosts, int* maxNumDisp) {
	if (!e || !disparity || !mask2x || !pixels || w <= 0 || h <= 0 || w2 <= SGM_HW + 2 * w || h2 < SGM_HW + 2 * h) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	DevBuf<int16_t> a; DevBuf<uint8_t> m; DevBuf<short2> r; const size_t n = (size_t)w * h, n2 = (size_t)w2 * h2;
	SGMCHK(e, a.alloc(n)); SGMCHK(e, m.alloc(n2)); SGMCHK(e, r.alloc(n));
	SGMCHK(e, hipMemcpyAsync(a, disparity, n * 2, hipMemcpyHostToDevice, e->stream)); SGMCHK(e, hipMemcpyAsync(m, mask2x, n2, hipMemcpyHostToDevice, e->stream));
	sgmRanges(e->stream, a, w, h, m, w2, minNumDisp, minNumDispInvalid, r);
	std::vector<int16_t> rg(n * 2);
	SGMCHK(e, hipMemcpyAsync(rg.data(), r, n * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	// expansion to the 2x pixel table in raster order (:1409-1441): 2x pixel (R, C) takes the range of low-resolution pixel
	// (R < HW+2 ? 0 : min((R-HW)/2, h-1), likewise for C); idx is the running sum of numDisp
	uint64_t total = 0; int mx = 0;
	for (int R = 0; R < h2; ++R) {
		const int rr = R < SGM_HW + 2 ? 0 : std::min((R - SGM_HW) / 2, h - 1);
		for (int Cc = 0; Cc < w2; ++Cc) {
			const int cc = Cc < SGM_HW + 2 ? 0 : std::min((Cc - SGM_HW) / 2, w - 1);
			const int16_t lo = rg[((size_t)rr * w + cc) * 2], hi = rg[((size_t)rr * w + cc) * 2 + 1];
			SGMHipPixelData& px = pixels[(size_t)R * w2 + Cc];
			px.idx = total; px.minDisp = lo; px.maxDisp = hi;
			const int nd = (int16_t)(hi - lo);
			total += (uint64_t)(int64_t)nd;
			if (nd > mx) mx = nd;
		}
	}
	if (numCosts) *numCosts = total;
	if (maxNumDisp) *maxNumDisp = mx;
	return 0;
}

int sgmhip_depth2disparity_map(sgmhip_engine* e, const float* depthMap, int dw, int dh, const double invH[9], const double invQ[16], int subpixelSteps,
		int16_t* disparity, int w, int h) {
	if (!e || !depthMap || !invH || !invQ || !disparity || dw <= 0 || dh <= 0 || w <= 0 || h <= 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, b; const size_t nd = (size_t)dw * dh, n = (size_t)w * h;
	SGMCHK(e, a.alloc(nd * 4)); SGMCHK(e, b.alloc(n * 2));
	SGMCHK(e, hipMemcpyAsync(a.p, depthMap, nd * 4, hipMemcpyHostToDevice, e->stream));
	SGMPMat mh{}, mq{}; memcpy(mh.m, invH, 72); memcpy(mq.m, invQ, 128);
	hipLaunchKernelGGL(sgmp_depth2disparity_kernel, dim3(gridFor(n)), dim3(256), 0, e->stream, (const float*)a.p, dw, dh, mh, mq, subpixelSteps, (int16_t*)b.p, w, h);
	SGMCHK(e, hipMemcpyAsync(disparity, b.p, n * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_disparity2depth_map(sgmhip_engine* e, const int16_t* disparity, const uint16_t* cost, int w, int h, const double H[9], const double Q[16],
		int subpixelSteps, float* depthMap, float* confMap, int dw, int dh) {
	if (!e || !disparity || !H || !Q || !depthMap || (cost && !confMap) || dw <= 0 || dh <= 0 || w <= 0 || h <= 0 || subpixelSteps <= 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	Scoped a, c, d, f; const size_t n = (size_t)w * h, nd = (size_t)dw * dh;
	SGMCHK(e, a.alloc(n * 2)); SGMCHK(e, c.alloc(n * 2)); SGMCHK(e, d.alloc(nd * 4)); SGMCHK(e, f.alloc(nd * 4));
	SGMCHK(e, hipMemcpyAsync(a.p, disparity, n * 2, hipMemcpyHostToDevice, e->stream));
	if (cost) SGMCHK(e, hipMemcpyAsync(c.p, cost, n * 2, hipMemcpyHostToDevice, e->stream));
	SGMPMat mh{}, mq{}; memcpy(mh.m, H, 72); memcpy(mq.m, Q, 128);
	hipLaunchKernelGGL(sgmp_disparity2depth_kernel, dim3(gridFor(nd)), dim3(256), 0, e->stream, (const int16_t*)a.p, cost ? (const uint16_t*)c.p : nullptr, w, h, mh, mq, subpixelSteps, (float*)d.p, (float*)f.p, dw, dh);
	SGMCHK(e, hipMemcpyAsync(depthMap, d.p, nd * 4, hipMemcpyDeviceToHost, e->stream));
	if (cost) SGMCHK(e, hipMemcpyAsync(confMap, f.p, nd * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_project_disparity2depth_map(sgmhip_engine* e, const int16_t* disparity, const uint16_t* cost, int w, int h, const double Q[16], int subpixelSteps,
		float* depthMap, float* depthRangeMap, float* confMap, int dw, int dh, int* anyDepth) {
	if (!e || !disparity || !Q || !depthMap || !depthRangeMap || (cost && !confMap) || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || subpixelSteps <= 0 || (size_t)w * h > 0xFFFFFFFFull) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	DevBuf<int16_t> a; DevBuf<uint16_t> c; DevBuf<unsigned long long> k; DevBuf<float> d, rg, cf; DevBuf<unsigned> cnt; const size_t n = (size_t)w * h, nd = (size_t)dw * dh;
	SGMCHK(e, a.alloc(n)); SGMCHK(e, c.alloc(n)); SGMCHK(e, k.alloc(nd * 4)); SGMCHK(e, d.alloc(nd)); SGMCHK(e, rg.alloc(nd * 2)); SGMCHK(e, cf.alloc(nd)); SGMCHK(e, cnt.alloc(1));
	SGMCHK(e, hipMemcpyAsync(a, disparity, n * 2, hipMemcpyHostToDevice, e->stream));
	if (cost) SGMCHK(e, hipMemcpyAsync(c, cost, n * 2, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipMemsetAsync(cnt, 0, 4, e->stream));
	SGMCHK(e, sgmProject(e->stream, a, cost ? c.p : nullptr, w, h, Q, subpixelSteps, k, dw, dh, d, rg, cost ? cf.p : nullptr, cnt));
	unsigned num = 0;
	SGMCHK(e, hipMemcpyAsync(depthMap, d, nd * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipMemcpyAsync(depthRangeMap, rg, nd * 8, hipMemcpyDeviceToHost, e->stream));
	if (cost) SGMCHK(e, hipMemcpyAsync(confMap, cf, nd * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipMemcpyAsync(&num, cnt, 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	if (anyDepth) *anyDepth = num > 0 ? 1 : 0;
	return 0;
}

int sgmhip_fuse_pairs(sgmhip_engine* e, const float* const* depthMaps, const float* const* depthRangeMaps, const float* const* confMaps, int nPairs, int dw, int dh,
		unsigned minViews, float* depthMap, float* confMap) {
	if (!e || !depthMaps || !depthRangeMaps || !confMaps || nPairs < 0 || nPairs > SGMP_MAX_PAIRS || dw <= 0 || dh <= 0 || !depthMap || !confMap) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	const size_t nd = (size_t)dw * dh;
	std::vector<Scoped> bufs((size_t)nPairs * 3);
	SGMPPairs pr{};
	for (int p = 0; p < nPairs; ++p) {
		if (!depthMaps[p] || !depthRangeMaps[p] || !confMaps[p]) return SGMHIP_E_ARG;
		SGMCHK(e, bufs[p * 3].alloc(nd * 4)); SGMCHK(e, bufs[p * 3 + 1].alloc(nd * 8)); SGMCHK(e, bufs[p * 3 + 2].alloc(nd * 4));
		SGMCHK(e, hipMemcpyAsync(bufs[p * 3].p, depthMaps[p], nd * 4, hipMemcpyHostToDevice, e->stream));
		SGMCHK(e, hipMemcpyAsync(bufs[p * 3 + 1].p, depthRangeMaps[p], nd * 8, hipMemcpyHostToDevice, e->stream));
		SGMCHK(e, hipMemcpyAsync(bufs[p * 3 + 2].p, confMaps[p], nd * 4, hipMemcpyHostToDevice, e->stream));
		pr.depth[p] = (const float*)bufs[p * 3].p; pr.range[p] = (const float*)bufs[p * 3 + 1].p; pr.conf[p] = (const float*)bufs[p * 3 + 2].p;
	}
	Scoped d, c; SGMCHK(e, d.alloc(nd * 4)); SGMCHK(e, c.alloc(nd * 4));
	hipLaunchKernelGGL(sgmp_fuse_pairs_kernel, dim3(gridFor(nd)), dim3(256), 0, e->stream, pr, nPairs, nd, minViews, (float*)d.p, (float*)c.p);
	SGMCHK(e, hipMemcpyAsync(depthMap, d.p, nd * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipMemcpyAsync(confMap, c.p, nd * 4, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

// SemiGlobalMatcher::Fuse (:738-859) for pairs that have the reference image on the left, resident: ProjectDisparity2DepthMap of every pair, pairs that
// produce no depth are dropped (:779-782), then the per-pixel cluster fusion -- the per-pair maps never leave the device.
int sgmhip_fuse_disparities(sgmhip_engine* e, int nPairs, const int16_t* const* disparities, const uint16_t* const* costs, const int* widths, const int* heights,
		const double* Qs, const int* subpixelSteps, int dw, int dh, unsigned minViews, float* depthMap, float* confMap, int* nUsed) {
	if (!e || nPairs < 0 || nPairs > SGMP_MAX_PAIRS || (nPairs && (!disparities || !costs || !widths || !heights || !Qs || !subpixelSteps)) || dw <= 0 || dh <= 0 || !depthMap || !confMap) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	hipStream_t st = e->stream;
	const size_t nd = (size_t)dw * dh;
	std::vector<DevBuf<float>> maps((size_t)nPairs * 3);                     // depth, range (two floats per pixel) and confidence of every pair
	DevBuf<unsigned long long> k; DevBuf<unsigned> cnt; DevBuf<float> d, c;
	SGMCHK(e, k.alloc(nd * 4)); SGMCHK(e, cnt.alloc((size_t)std::max(nPairs, 1))); SGMCHK(e, d.alloc(nd)); SGMCHK(e, c.alloc(nd));
	SGMCHK(e, hipMemsetAsync(cnt, 0, 4 * (size_t)std::max(nPairs, 1), st));
	std::vector<DevBuf<int16_t>> disp((size_t)nPairs); std::vector<DevBuf<uint16_t>> cst((size_t)nPairs);
	for (int p = 0; p < nPairs; ++p) {
		const int w = widths[p], h = heights[p];
		if (!disparities[p] || !costs[p] || w <= 0 || h <= 0 || subpixelSteps[p] <= 0 || (size_t)w * h > 0xFFFFFFFFull) return SGMHIP_E_ARG;
		const size_t n = (size_t)w * h;
		SGMCHK(e, disp[p].alloc(n)); SGMCHK(e, cst[p].alloc(n));
		SGMCHK(e, maps[p * 3].alloc(nd)); SGMCHK(e, maps[p * 3 + 1].alloc(nd * 2)); SGMCHK(e, maps[p * 3 + 2].alloc(nd));
		SGMCHK(e, hipMemcpyAsync(disp[p], disparities[p], n * 2, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(cst[p], costs[p], n * 2, hipMemcpyHostToDevice, st));
		SGMCHK(e, sgmProject(st, disp[p], cst[p], w, h, Qs + 16 * p, subpixelSteps[p], k, dw, dh, maps[p * 3], maps[p * 3 + 1], maps[p * 3 + 2], cnt.p + p));
	}
	std::vector<unsigned> num((size_t)std::max(nPairs, 1), 0u);
	if (nPairs) SGMCHK(e, hipMemcpyAsync(num.data(), cnt, 4 * (size_t)nPairs, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipStreamSynchronize(st));
	SGMPPairs pr{}; int used = 0;
	for (int p = 0; p < nPairs; ++p) if (num[p] > 0) { pr.depth[used] = maps[p * 3]; pr.range[used] = maps[p * 3 + 1]; pr.conf[used] = maps[p * 3 + 2]; ++used; }
	if (nUsed) *nUsed = used;
	if (used == 0) { memset(depthMap, 0, nd * 4); memset(confMap, 0, nd * 4); return 0; }
	hipLaunchKernelGGL(sgmp_fuse_pairs_kernel, dim3(gridFor(nd)), dim3(256), 0, st, pr, used, nd, minViews, d, c);
	SGMCHK(e, hipGetLastError());
	SGMCHK(e, hipMemcpyAsync(depthMap, d, nd * 4, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipMemcpyAsync(confMap, c, nd * 4, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipStreamSynchronize(st));
	return 0;
}

int sgmhip_filter_speckles(sgmhip_engine* e, int16_t* disparity, int w, int h, int maxSpeckleSize, int maxDiff) {
	if (!e || !disparity || w <= 0 || h <= 0 || maxSpeckleSize < 0 || maxDiff < 0 || (size_t)w * h > 0x7fffffffull) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	DevBuf<int16_t> a; DevBuf<int> p, z; const size_t n = (size_t)w * h;
	SGMCHK(e, a.alloc(n)); SGMCHK(e, p.alloc(n)); SGMCHK(e, z.alloc(n));
	SGMCHK(e, hipMemcpyAsync(a, disparity, n * 2, hipMemcpyHostToDevice, e->stream));
	sgmSpeckles(e->stream, a, w, h, maxSpeckleSize, maxDiff, p, z);
	SGMCHK(e, hipMemcpyAsync(disparity, a, n * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_set_disparity(sgmhip_engine* e, const int16_t* disparity) {
	if (!e || !disparity || e->numCosts == 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	SGMCHK(e, hipMemcpyAsync(e->d_disp, disparity, (size_t)e->vw * e->vh * 2, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

// ---- the whole coarse-to-fine loop for one rectified pair, resident (SemiGlobalMatcher.cpp:577-706; kernels in sgm_tsgm.hip) -----------------
namespace {
// computeMaxResolution(w, h, level = 8, minResolution) (libs/Common/Types.inl:2459-2477) -> k with scale = 1 / max(2, 2^k); 0 = plain SGM
int tsgmLevels(int w, int h, unsigned minResolution) {
	if (!minResolution) return 0;
	const unsigned size0 = (unsigned)std::max(w, h);
	unsigned level = 8;
	if ((size0 >> level) < minResolution) { level = 0; while ((size0 >> (level + 1)) >= minResolution) ++level; }
	return (int)std::max(1u, level);
}
inline int cvRound(double v) { return (int)nearbyint(v); }      // cv::saturate_cast<int>(double): round half to even
}

// the size rules of the coarse-to-fine loop (minResolution > 0; 0 is tsgmPlainRun): -> levels k (>= 1), or 0 with the engine's error text set
static int tsgmCheckSize(sgmhip_engine* e, int w, int h, unsigned minResolution) {
	const int k = tsgmLevels(w, h, minResolution);
	if ((w % (1 << k)) || (h % (1 << k)) || (w >> k) <= 2 * SGM_HW + 2 || (h >> k) <= 2 * SGM_HW + 2) { e->err = "image size must be a multiple of 2^levels and its coarsest level larger than the window"; return 0; }
	return k;
}

// the loop on a rectified pair that is on the device already (full-resolution BGR, gray and masks of both sides): what sgmhip_tsgm_match runs after its uploads
// and sgmhip_tsgm_match_rectified runs on the outputs of sgmhip_rectify_pair
static int tsgmRun(sgmhip_engine* e, const unsigned char* fLB, const unsigned char* fRB, const float* fLG, const float* fRG, const unsigned char* fLM, const unsigned char* fRM,
		int w, int h, int k, const int16_t* initLeftDisparity, int nSpeckleSize, int subpixelMode, int subpixelSteps, uint16_t P1, const uint16_t P2s[256],
		int16_t* disparity, uint16_t* cost, int* numLevels, bool initOnDevice = false) {
	hipStream_t st = e->stream;
	const size_t nFull = (size_t)w * h, nValid = (size_t)(w - 2 * SGM_HW) * (h - 2 * SGM_HW);
	// the per-level working set (sized for the finest level)
	DevBuf<unsigned char> lB, rB; DevBuf<float> lG, rG; DevBuf<uint8_t> lM, rM, lM2, rM2; DevBuf<int16_t> lD, rD, lDn, rDn;
	DevBuf<uint32_t> keys; DevBuf<short2> ranges; DevBuf<unsigned long long> tiles, scal; DevBuf<int> par, siz;
	SGMCHK(e, lB.alloc(nFull * 3)); SGMCHK(e, rB.alloc(nFull * 3)); SGMCHK(e, lG.alloc(nFull)); SGMCHK(e, rG.alloc(nFull));
	SGMCHK(e, lM.alloc(nValid)); SGMCHK(e, rM.alloc(nValid)); SGMCHK(e, lM2.alloc(nValid)); SGMCHK(e, rM2.alloc(nValid));
	SGMCHK(e, lD.alloc(nValid)); SGMCHK(e, rD.alloc(nValid)); SGMCHK(e, lDn.alloc(nValid)); SGMCHK(e, rDn.alloc(nValid));
	SGMCHK(e, keys.alloc(nValid)); SGMCHK(e, ranges.alloc(nValid)); SGMCHK(e, par.alloc(nValid)); SGMCHK(e, siz.alloc(nValid));
	const int maxTiles = (int)((nValid + SGMT_TILE - 1) / SGMT_TILE);
	SGMCHK(e, tiles.alloc((size_t)maxTiles)); SGMCHK(e, scal.alloc(2));     // scal: {numCosts, maxNumDisp} of a level's range table
	{ const int rc = sgmSetP2s(e, P1, P2s); if (rc) return rc; }

	int16_t *leftDisp = lD, *rightDisp = rD, *leftNew = lDn, *rightNew = rDn;
	uint8_t *lm = lM, *rm = rM, *lmNext = lM2, *rmNext = rM2;
	int dW = 0, dH = 0;            // size of leftDisp (the previous level's valid grid)
	int mW = 0, mH = 0;            // size of the masks
	int levels = 0;
	bool first = true;
	// Disparity2RangeMap on the device + Match of (bgr, grayA -> grayB) with those ranges; the result is copied to `out`
	auto rangeAndMatch = [&](const int16_t* disp, const uint8_t* mask2x, int vw, int vh, int lw, int lh, const unsigned char* bgr, const float* gA, const float* gB, int a, int b, int16_t* out) -> int {
		const size_t n2 = (size_t)vw * vh;
		sgmRanges(st, disp, dW, dH, mask2x, vw, a, b, ranges);
		const int nT = (int)((n2 + SGMT_TILE - 1) / SGMT_TILE);
		SGMCHK(e, hipMemsetAsync(scal, 0, 16, st));
		hipLaunchKernelGGL(sgmt_tile_sums_kernel, dim3(nT), dim3(256), 0, st, (const short2*)ranges.p, dW, dH, vw, n2, tiles.p, (int*)(scal.p + 1));
		hipLaunchKernelGGL(sgmt_scan_tiles_kernel, dim3(1), dim3(256), 0, st, tiles.p, nT, scal.p);
		unsigned long long hs[2] = {0, 0};
		SGMCHK(e, hipMemcpyAsync(hs, scal, 16, hipMemcpyDeviceToHost, st));
		SGMCHK(e, hipStreamSynchronize(st));
		const uint64_t numCosts = hs[0]; const int mx = (int)(hs[1] & 0xffffffffull);
		if (numCosts == 0 || mx <= 0 || mx > 256) { e->err = "tsgm: empty or too wide disparity ranges at a level"; return SGMHIP_E_ARG; }
		{ const int rc = sgmReserve(e, lw, lh, numCosts, mx); if (rc) return rc; }
		hipLaunchKernelGGL(sgmt_expand_kernel, dim3(nT), dim3(256), 0, st, (const short2*)ranges.p, dW, dH, vw, n2, (const unsigned long long*)tiles.p, e->d_pixels);
		const size_t nImg = (size_t)lw * lh;
		SGMCHK(e, hipMemcpyAsync(e->d_color, bgr, nImg * 3, hipMemcpyDeviceToDevice, st));
		SGMCHK(e, hipMemcpyAsync(e->d_grayL, gA, nImg * 4, hipMemcpyDeviceToDevice, st));
		SGMCHK(e, hipMemcpyAsync(e->d_grayR, gB, nImg * 4, hipMemcpyDeviceToDevice, st));
		// narrow ranges (every level but the first): 16-lane sub-groups; wide ranges: one wavefront per pixel / line
		const int saved = e->subGroups;
		if (!saved && numCosts <= (uint64_t)n2 * 24) e->subGroups = 16;
		const int rcm = sgmMatch(e, P1);
		e->subGroups = saved;
		if (rcm) return rcm;
		SGMCHK(e, hipMemcpyAsync(out, e->d_disp, n2 * 2, hipMemcpyDeviceToDevice, st));
		return 0;
	};
	for (int lvl = k; lvl >= 0; --lvl) {
		const int f = 1 << lvl, lw = w / f, lh = h / f, vw = lw - 2 * SGM_HW, vh = lh - 2 * SGM_HW;
		const size_t nImg = (size_t)lw * lh, nV = (size_t)vw * vh;
		const unsigned char *pLB = fLB, *pRB = fRB; const float *pLG = fLG, *pRG = fRG;
		if (f != 1) {
			hipLaunchKernelGGL(sgmt_area_u8x3_kernel, dim3(gridFor(nImg * 3)), dim3(256), 0, st, fLB, w, lB.p, lw, lh, f);
			hipLaunchKernelGGL(sgmt_area_u8x3_kernel, dim3(gridFor(nImg * 3)), dim3(256), 0, st, fRB, w, rB.p, lw, lh, f);
			hipLaunchKernelGGL(sgmt_area_f32_kernel, dim3(gridFor(nImg)), dim3(256), 0, st, fLG, w, lG.p, lw, lh, f);
			hipLaunchKernelGGL(sgmt_area_f32_kernel, dim3(gridFor(nImg)), dim3(256), 0, st, fRG, w, rG.p, lw, lh, f);
			pLB = lB; pRB = rB; pLG = lG; pRG = rG;
		}
		if (first) {
			const int hw2 = cvRound(lw * 0.5), hh2 = cvRound(lh * 0.5);                 // Image8U::computeResize(size, 0.5), :622
			dW = hw2 - 2 * SGM_HW; dH = hh2 - 2 * SGM_HW;
			if (dW <= 0 || dH <= 0) { e->err = "tsgm: coarsest level too small"; return SGMHIP_E_ARG; }
			if (initLeftDisparity) SGMCHK(e, hipMemcpyAsync(leftDisp, initLeftDisparity, (size_t)dW * dH * 2, initOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
			else hipLaunchKernelGGL(sgmt_fill_i16_kernel, dim3(gridFor((size_t)dW * dH)), dim3(256), 0, st, leftDisp, (size_t)dW * dH, (short)SGMP_NO_DISP);
			hipLaunchKernelGGL(sgmt_mask_first_kernel, dim3(gridFor(nV)), dim3(256), 0, st, fLM, w, lm, vw, vh, f);   // :627-631
			hipLaunchKernelGGL(sgmt_mask_first_kernel, dim3(gridFor(nV)), dim3(256), 0, st, fRM, w, rm, vw, vh, f);
		} else {
			hipLaunchKernelGGL(sgmp_upscale_mask_kernel, dim3(gridFor(nV)), dim3(256), 0, st, (const uint8_t*)lm, mW, mH, lmNext, vw, vh);   // :634-635
			hipLaunchKernelGGL(sgmp_upscale_mask_kernel, dim3(gridFor(nV)), dim3(256), 0, st, (const uint8_t*)rm, mW, mH, rmNext, vw, vh);
			std::swap(lm, lmNext); std::swap(rm, rmNext);
		}
		mW = vw; mH = vh;
		const int a = first ? 11 : 5, b = first ? 33 : 7;
		// right -> left with ranges from the flipped previous disparities (:641-654)
		SGMCHK(e, sgmFlip(st, leftDisp, dW, dH, keys, rightDisp));
		{ const int rc = rangeAndMatch(rightDisp, rm, vw, vh, lw, lh, pRB, pRG, pLG, a, b, rightNew); if (rc) return rc; }
		// left -> right (:657-667)
		{ const int rc = rangeAndMatch(leftDisp, lm, vw, vh, lw, lh, pLB, pLG, pRG, a, b, leftNew); if (rc) return rc; }
		std::swap(leftDisp, leftNew); std::swap(rightDisp, rightNew);
		dW = vw; dH = vh;
		hipLaunchKernelGGL(sgmp_cross_check_kernel, dim3(gridFor(nV)), dim3(256), 0, st, leftDisp, (const int16_t*)rightDisp, vw, vw, vh, 1);
		if (first) {                                                                   // :680-690
			hipLaunchKernelGGL(sgmp_cross_check_kernel, dim3(gridFor(nV)), dim3(256), 0, st, rightDisp, (const int16_t*)leftDisp, vw, vw, vh, 1);
			sgmSpeckles(st, leftDisp, vw, vh, nSpeckleSize, 5, par, siz); sgmSpeckles(st, rightDisp, vw, vh, nSpeckleSize, 5, par, siz);
			hipLaunchKernelGGL(sgmp_extract_mask_kernel, dim3((vh + 63) / 64), dim3(64), 0, st, (const int16_t*)leftDisp, lm, vw, vh, 3);
			hipLaunchKernelGGL(sgmp_extract_mask_kernel, dim3((vh + 63) / 64), dim3(64), 0, st, (const int16_t*)rightDisp, rm, vw, vh, 3);
		}
		first = false; ++levels;
	}
	// sub-pixel refinement on the resident sums of the last (left) Match with the cross-checked map (:699)
	const size_t nV = (size_t)dW * dH;
	SGMCHK(e, hipMemcpyAsync(e->d_disp, leftDisp, nV * 2, hipMemcpyDeviceToDevice, st));
	if (subpixelSteps > 1)
		hipLaunchKernelGGL(sgmp_refine_kernel, dim3(gridFor(nV)), dim3(256), 0, st, e->d_pixels, e->d_accums, (long)nV, e->d_disp, subpixelMode, subpixelSteps);
	SGMCHK(e, hipGetLastError());
	SGMCHK(e, hipMemcpyAsync(disparity, e->d_disp, nV * 2, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipMemcpyAsync(cost, e->d_cost, nV * 2, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipStreamSynchronize(st));
	if (numLevels) *numLevels = levels;
	return 0;
}

// plain SGM (minResolution == 0, :585-590, 643-706) on a rectified pair that is on the device: one level at full resolution.  The seed only gives the global range
// (sgmhip_plain_range); Match(right, left) runs with it as it is and Match(left, right) with its negation -- the reference's assignment, the opposite of the
// tSGM branch (SetStereoRectificationROI centres the shared points' disparities around zero).  Then the first-level filtering and the refinement on the sums of the
// left Match.  The masks are only cropped and re-extracted by the reference (:612-617, 705-706) and never read again: they are not computed.
static int tsgmPlainRun(sgmhip_engine* e, const unsigned char* fLB, const unsigned char* fRB, const float* fLG, const float* fRG, int w, int h,
		const int16_t* initLeftDisparity, int nSpeckleSize, int subpixelMode, int subpixelSteps, uint16_t P1, const uint16_t P2s[256],
		int16_t* disparity, uint16_t* cost, int* numLevels) {
	const int dW = cvRound(w * 0.5) - 2 * SGM_HW, dH = cvRound(h * 0.5) - 2 * SGM_HW;   // the seed: Image8U::computeResize(size, 0.5), :611-625
	if (w <= 2 * SGM_HW || h <= 2 * SGM_HW || dW <= 0 || dH <= 0) { e->err = "plain SGM: the half-resolution seed grid of a " + std::to_string(w) + " x " + std::to_string(h) + " image is empty"; return SGMHIP_E_ARG; }
	int16_t sMin = SGMP_NO_DISP, sMax = SGMP_NO_DISP, mn = 0, mx = 0;
	if (initLeftDisparity) { const auto mm = std::minmax_element(initLeftDisparity, initLeftDisparity + (size_t)dW * dH); sMin = *mm.first; sMax = *mm.second; }
	{ const int16_t two[2] = {sMin, sMax}; sgmhip_plain_range(two, 2, &mn, &mx); }
	{ const std::string why = sgmUniformRefusal(mn, mx); if (!why.empty()) { e->err = "plain SGM: the seed's disparities span " + std::to_string(sMin) + " .. " + std::to_string(sMax) + " (min, max), which gives D = " + std::to_string((int)mx - (int)mn) + ": " + why; return SGMHIP_E_ARG; } }
	hipStream_t st = e->stream;
	const int vw = w - 2 * SGM_HW, vh = h - 2 * SGM_HW;
	const size_t nImg = (size_t)w * h, nV = (size_t)vw * vh;
	DevBuf<int16_t> lD, rD; DevBuf<int> par, siz;
	SGMCHK(e, lD.alloc(nV)); SGMCHK(e, rD.alloc(nV)); SGMCHK(e, par.alloc(nV)); SGMCHK(e, siz.alloc(nV));
	{ const int rc = sgmSetP2s(e, P1, P2s); if (rc) return rc; }
	auto match = [&](const unsigned char* bgr, const float* gA, const float* gB, int a, int b, int16_t* out) -> int {
		{ const int rc = sgmReserveUniform(e, w, h, a, b); if (rc) return rc; }
		SGMCHK(e, hipMemcpyAsync(e->d_color, bgr, nImg * 3, hipMemcpyDeviceToDevice, st));
		SGMCHK(e, hipMemcpyAsync(e->d_grayL, gA, nImg * 4, hipMemcpyDeviceToDevice, st));
		SGMCHK(e, hipMemcpyAsync(e->d_grayR, gB, nImg * 4, hipMemcpyDeviceToDevice, st));
		{ const int rc = sgmMatch(e, P1); if (rc) return rc; }
		SGMCHK(e, hipMemcpyAsync(out, e->d_disp, nV * 2, hipMemcpyDeviceToDevice, st));
		return 0;
	};
	{ const int rc = match(fRB, fRG, fLG, mn, mx, rD); if (rc) return rc; }          // :667-676
	{ const int rc = match(fLB, fLG, fRG, -mx, -mn, lD); if (rc) return rc; }        // :678-685
	hipLaunchKernelGGL(sgmp_cross_check_kernel, dim3(gridFor(nV)), dim3(256), 0, st, lD.p, (const int16_t*)rD.p, vw, vw, vh, 1);   // :698-706
	hipLaunchKernelGGL(sgmp_cross_check_kernel, dim3(gridFor(nV)), dim3(256), 0, st, rD.p, (const int16_t*)lD.p, vw, vw, vh, 1);
	sgmSpeckles(st, lD, vw, vh, nSpeckleSize, 5, par, siz); sgmSpeckles(st, rD, vw, vh, nSpeckleSize, 5, par, siz);
	SGMCHK(e, hipMemcpyAsync(e->d_disp, lD, nV * 2, hipMemcpyDeviceToDevice, st));
	if (subpixelSteps > 1)
		hipLaunchKernelGGL(sgmp_refine_kernel, dim3(gridFor(nV)), dim3(256), 0, st, e->d_pixels, e->d_accums, (long)nV, e->d_disp, subpixelMode, subpixelSteps);
	SGMCHK(e, hipGetLastError());
	SGMCHK(e, hipMemcpyAsync(disparity, e->d_disp, nV * 2, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipMemcpyAsync(cost, e->d_cost, nV * 2, hipMemcpyDeviceToHost, st));
	SGMCHK(e, hipStreamSynchronize(st));
	if (numLevels) *numLevels = 1;
	return 0;
}

int sgmhip_tsgm_match(sgmhip_engine* e, const uint8_t* leftBGR, const uint8_t* rightBGR, const float* leftGray, const float* rightGray,
		const uint8_t* leftMask, const uint8_t* rightMask, int w, int h, unsigned minResolution, const int16_t* initLeftDisparity,
		int nSpeckleSize, int subpixelMode, int subpixelSteps, uint16_t P1, const uint16_t P2s[256], int16_t* disparity, uint16_t* cost, int* numLevels) {
	if (!e || !leftBGR || !rightBGR || !leftGray || !rightGray || !leftMask || !rightMask || !P2s || !disparity || !cost || w <= 0 || h <= 0 || nSpeckleSize < 0 ||
	    subpixelMode < 0 || subpixelMode > SGMP_SUBPIXEL_LC_BLEND || subpixelSteps < 0 || subpixelSteps > 64) return SGMHIP_E_ARG;
	const int k = minResolution ? tsgmCheckSize(e, w, h, minResolution) : 0;
	if (minResolution && k == 0) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	hipStream_t st = e->stream;
	const size_t nFull = (size_t)w * h;
	DevBuf<unsigned char> fLB, fRB, fLM, fRM; DevBuf<float> fLG, fRG;          // the full-resolution inputs
	if (!minResolution) {                                                      // plain SGM reads no mask
		SGMCHK(e, fLB.alloc(nFull * 3)); SGMCHK(e, fRB.alloc(nFull * 3)); SGMCHK(e, fLG.alloc(nFull)); SGMCHK(e, fRG.alloc(nFull));
		SGMCHK(e, hipMemcpyAsync(fLB, leftBGR, nFull * 3, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(fRB, rightBGR, nFull * 3, hipMemcpyHostToDevice, st));
		SGMCHK(e, hipMemcpyAsync(fLG, leftGray, nFull * 4, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(fRG, rightGray, nFull * 4, hipMemcpyHostToDevice, st));
		return tsgmPlainRun(e, fLB, fRB, fLG, fRG, w, h, initLeftDisparity, nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels);
	}
	SGMCHK(e, fLB.alloc(nFull * 3)); SGMCHK(e, fRB.alloc(nFull * 3)); SGMCHK(e, fLG.alloc(nFull)); SGMCHK(e, fRG.alloc(nFull)); SGMCHK(e, fLM.alloc(nFull)); SGMCHK(e, fRM.alloc(nFull));
	SGMCHK(e, hipMemcpyAsync(fLB, leftBGR, nFull * 3, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(fRB, rightBGR, nFull * 3, hipMemcpyHostToDevice, st));
	SGMCHK(e, hipMemcpyAsync(fLG, leftGray, nFull * 4, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(fRG, rightGray, nFull * 4, hipMemcpyHostToDevice, st));
	SGMCHK(e, hipMemcpyAsync(fLM, leftMask, nFull, hipMemcpyHostToDevice, st)); SGMCHK(e, hipMemcpyAsync(fRM, rightMask, nFull, hipMemcpyHostToDevice, st));
	return tsgmRun(e, fLB, fRB, fLG, fRG, fLM, fRM, w, h, k, initLeftDisparity, nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels);
}

// ---- the resident SGM scene: every image uploaded once, pairs rectified on the device (kernel in sgm_rectify.hip) ---------------------------------------------
int sgmhip_scene_create(sgmhip_engine* e, int nImages) {
	if (!e) return SGMHIP_E_ARG;
	if (nImages <= 0) { e->err = "scene_create: the number of images must be positive"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	e->scene.clear(); e->scene.resize((size_t)nImages);
	return 0;
}

int sgmhip_scene_set_image(sgmhip_engine* e, int idx, const uint8_t* bgr, int w, int h) {
	if (!e) return SGMHIP_E_ARG;
	if (idx < 0 || (size_t)idx >= e->scene.size()) { e->err = "scene_set_image: image index " + std::to_string(idx) + " is outside the scene table of " + std::to_string(e->scene.size()); return SGMHIP_E_ARG; }
	if (!bgr || w <= 0 || h <= 0) { e->err = "scene_set_image: no pixels, or a width or height <= 0"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	sgmhip_engine::SceneImage& im = e->scene[(size_t)idx];
	SGMCHK(e, hipStreamSynchronize(e->stream));
	im.w = im.h = 0;
	SGMCHK(e, im.bgr.alloc((size_t)w * h * 3));
	SGMCHK(e, hipMemcpyAsync(im.bgr, bgr, (size_t)w * h * 3, hipMemcpyHostToDevice, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	im.w = w; im.h = h;
	return 0;
}

int sgmhip_scene_clear(sgmhip_engine* e) {
	if (!e) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	e->scene.clear();
	sgmFreeSeed(e);
	return 0;
}

int sgmhip_rectify_pair(sgmhip_engine* e, int idxLeft, int idxRight, const double invH1[9], const double invH2[9], int w, int h, const float srgb2lin[256]) {
	if (!e) return SGMHIP_E_ARG;
	if (!invH1 || !invH2 || !srgb2lin) { e->err = "rectify_pair: null homography or table"; return SGMHIP_E_ARG; }
	const int idx[2] = {idxLeft, idxRight};
	for (int s = 0; s < 2; ++s) {
		if (idx[s] < 0 || (size_t)idx[s] >= e->scene.size()) { e->err = "rectify_pair: image index " + std::to_string(idx[s]) + " is outside the scene table of " + std::to_string(e->scene.size()); return SGMHIP_E_ARG; }
		if (!e->scene[(size_t)idx[s]].w) { e->err = "rectify_pair: image " + std::to_string(idx[s]) + " was never set"; return SGMHIP_E_ARG; }
	}
	if (w <= 0 || h <= 0) { e->err = "rectify_pair: the rectified width and height must be positive"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	hipStream_t st = e->stream;
	const size_t n = (size_t)w * h;
	e->rectW = e->rectH = 0;
	if (n > e->capRect) {
		SGMCHK(e, hipStreamSynchronize(st));
		for (int s = 0; s < 2; ++s) { SGMCHK(e, e->d_rectBGR[s].alloc(n * 3)); SGMCHK(e, e->d_rectGray[s].alloc(n)); SGMCHK(e, e->d_rectMask[s].alloc(n)); }
		e->capRect = n;
	}
	if (!e->d_srgb) SGMCHK(e, e->d_srgb.alloc(256));
	SGMCHK(e, hipMemcpyAsync(e->d_srgb, srgb2lin, 256 * sizeof(float), hipMemcpyHostToDevice, st));
	SGMRectPair pair;
	for (int s = 0; s < 2; ++s) {
		const sgmhip_engine::SceneImage& im = e->scene[(size_t)idx[s]];
		SGMRectSide& o = pair.s[s];
		o.src = im.bgr; o.W0 = im.w; o.H0 = im.h;
		memcpy(o.Hi, s ? invH2 : invH1, sizeof(o.Hi));
		o.bgr = e->d_rectBGR[s]; o.gray = e->d_rectGray[s]; o.mask = e->d_rectMask[s];
	}
	evB(e, 3);
	hipLaunchKernelGGL(sgm_rectify_pair_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), 2), dim3(64, 4), 0, st, pair, w, h, (const float*)e->d_srgb);
	evE(e);
	SGMCHK(e, hipGetLastError());
	SGMCHK(e, hipStreamSynchronize(st));          // srgb2lin is the caller's memory
	e->rectW = w; e->rectH = h;
	return 0;
}

int sgmhip_rectified_get(sgmhip_engine* e, int side, uint8_t* bgr, float* gray, uint8_t* mask) {
	if (!e) return SGMHIP_E_ARG;
	if (side < 0 || side > 1) { e->err = "rectified_get: side must be 0 (left) or 1 (right)"; return SGMHIP_E_ARG; }
	if (!e->rectW) { e->err = "no rectified pair is resident: call sgmhip_rectify_pair first"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	const size_t n = (size_t)e->rectW * e->rectH;
	if (bgr) SGMCHK(e, hipMemcpyAsync(bgr, e->d_rectBGR[side], n * 3, hipMemcpyDeviceToHost, e->stream));
	if (gray) SGMCHK(e, hipMemcpyAsync(gray, e->d_rectGray[side], n * 4, hipMemcpyDeviceToHost, e->stream));
	if (mask) SGMCHK(e, hipMemcpyAsync(mask, e->d_rectMask[side], n, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int sgmhip_tsgm_match_rectified(sgmhip_engine* e, unsigned minResolution, const int16_t* initLeftDisparity, int nSpeckleSize, int subpixelMode, int subpixelSteps,
		uint16_t P1, const uint16_t P2s[256], int16_t* disparity, uint16_t* cost, int* numLevels) {
	if (!e) return SGMHIP_E_ARG;
	if (!P2s || !disparity || !cost || nSpeckleSize < 0 || subpixelMode < 0 || subpixelMode > SGMP_SUBPIXEL_LC_BLEND || subpixelSteps < 0 || subpixelSteps > 64) { e->err = "tsgm_match_rectified: null pointer or option out of range"; return SGMHIP_E_ARG; }
	if (!e->rectW) { e->err = "no rectified pair is resident: call sgmhip_rectify_pair first"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	if (!minResolution) return tsgmPlainRun(e, e->d_rectBGR[0], e->d_rectBGR[1], e->d_rectGray[0], e->d_rectGray[1], e->rectW, e->rectH,
	                                        initLeftDisparity, nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels);
	const int k = tsgmCheckSize(e, e->rectW, e->rectH, minResolution);
	if (k == 0) return SGMHIP_E_ARG;
	return tsgmRun(e, e->d_rectBGR[0], e->d_rectBGR[1], e->d_rectGray[0], e->d_rectGray[1], e->d_rectMask[0], e->d_rectMask[1], e->rectW, e->rectH, k,
	               initLeftDisparity, nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels);
}

// ---- the seed made and kept on the device (include/sgmhip_seed.h; kernels and launch sequence: seed_raster.hip) ------------------------------------------------
int sgmhip_seed_raster(sgmhip_engine* e, int w, int h, const float* proj, const float* z, uint32_t nVerts, const uint32_t* faces, uint32_t nFaces, float* depthOut) {
	if (!e) return SGMHIP_E_ARG;
	const std::string why = seedCheck("seed_raster", SEED_MODE_FACES, w, h, proj, z, nVerts, faces, nFaces);
	if (!why.empty()) { e->err = why; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	const size_t P = (size_t)w * h;
	e->seedW = e->seedH = 0;
	SGMCHK(e, e->d_seedDepth.reserve(P));
	SGMCHK(e, seedRun(e->seed, e->stream, SEED_MODE_FACES, w, h, proj, z, nullptr, nVerts, faces, nFaces, e->d_seedDepth, nullptr));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	SGMCHK(e, seedCollect(e->seed, SEED_MODE_FACES, nVerts == 0 || nFaces == 0));
	if (depthOut) SGMCHK(e, hipMemcpy(depthOut, e->d_seedDepth, sizeof(float) * P, hipMemcpyDeviceToHost));
	e->seedW = w; e->seedH = h;
	return 0;
}

int sgmhip_seed_disparity(sgmhip_engine* e, const double invH[9], const double invQ[16], int subpixelSteps, int w, int h, int16_t* disparityOut) {
	if (!e) return SGMHIP_E_ARG;
	if (!invH || !invQ || w <= 0 || h <= 0) { e->err = "seed_disparity: null matrix, or a width or height <= 0"; return SGMHIP_E_ARG; }
	if (!e->seedW) { e->err = "no seed is resident: call sgmhip_seed_raster first"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	const size_t n = (size_t)w * h;
	e->seedDispW = e->seedDispH = 0;
	SGMCHK(e, e->d_seedDisp.reserve(n));
	SGMPMat mh{}, mq{}; memcpy(mh.m, invH, 72); memcpy(mq.m, invQ, 128);
	hipLaunchKernelGGL(sgmp_depth2disparity_kernel, dim3(gridFor(n)), dim3(256), 0, e->stream, (const float*)e->d_seedDepth.p, e->seedW, e->seedH, mh, mq, subpixelSteps,
	                   e->d_seedDisp.p, w, h);
	SGMCHK(e, hipGetLastError());
	if (disparityOut) SGMCHK(e, hipMemcpyAsync(disparityOut, e->d_seedDisp, n * 2, hipMemcpyDeviceToHost, e->stream));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	e->seedDispW = w; e->seedDispH = h;
	return 0;
}

int sgmhip_tsgm_match_rectified_seeded(sgmhip_engine* e, unsigned minResolution, int nSpeckleSize, int subpixelMode, int subpixelSteps,
		uint16_t P1, const uint16_t P2s[256], int16_t* disparity, uint16_t* cost, int* numLevels) {
	if (!e) return SGMHIP_E_ARG;
	if (!P2s || !disparity || !cost || nSpeckleSize < 0 || subpixelMode < 0 || subpixelMode > SGMP_SUBPIXEL_LC_BLEND || subpixelSteps < 0 || subpixelSteps > 64) { e->err = "tsgm_match_rectified: null pointer or option out of range"; return SGMHIP_E_ARG; }
	if (!e->rectW) { e->err = "no rectified pair is resident: call sgmhip_rectify_pair first"; return SGMHIP_E_ARG; }
	if (!e->seedDispW) { e->err = "no seed disparity is resident: call sgmhip_seed_raster and sgmhip_seed_disparity first"; return SGMHIP_E_ARG; }
	SGMCHK(e, hipSetDevice(e->device));
	const int k = minResolution ? tsgmCheckSize(e, e->rectW, e->rectH, minResolution) : 0;
	if (minResolution && k == 0) return SGMHIP_E_ARG;
	// the first level's seed grid: Image8U::computeResize(level size, 0.5) less the window's border (tsgmRun, tsgmPlainRun)
	const int dW = cvRound((e->rectW >> k) * 0.5) - 2 * SGM_HW, dH = cvRound((e->rectH >> k) * 0.5) - 2 * SGM_HW;
	if (e->seedDispW != dW || e->seedDispH != dH) {
		e->err = "tsgm_match_rectified_seeded: the resident seed disparity is " + std::to_string(e->seedDispW) + " x " + std::to_string(e->seedDispH) + ", the first level's seed grid " +
		         std::to_string(dW) + " x " + std::to_string(dH);
		return SGMHIP_E_ARG;
	}
	if (!minResolution) {   // the seed only gives the global range: its values come back for sgmhip_plain_range
		std::vector<int16_t> host((size_t)dW * dH);
		SGMCHK(e, hipMemcpyAsync(host.data(), e->d_seedDisp, host.size() * 2, hipMemcpyDeviceToHost, e->stream));
		SGMCHK(e, hipStreamSynchronize(e->stream));
		return tsgmPlainRun(e, e->d_rectBGR[0], e->d_rectBGR[1], e->d_rectGray[0], e->d_rectGray[1], e->rectW, e->rectH,
		                    host.data(), nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels);
	}
	return tsgmRun(e, e->d_rectBGR[0], e->d_rectBGR[1], e->d_rectGray[0], e->d_rectGray[1], e->d_rectMask[0], e->d_rectMask[1], e->rectW, e->rectH, k,
	               e->d_seedDisp, nSpeckleSize, subpixelMode, subpixelSteps, P1, P2s, disparity, cost, numLevels, true);
}

int sgmhip_seed_clear(sgmhip_engine* e) {
	if (!e) return SGMHIP_E_ARG;
	SGMCHK(e, hipSetDevice(e->device));
	SGMCHK(e, hipStreamSynchronize(e->stream));
	sgmFreeSeed(e);
	return 0;
}

int sgmhip_rectify_stats_get(sgmhip_engine* e, double* kernelMs, uint64_t* calls) {
	if (!e) return SGMHIP_E_ARG;
	hipSetDevice(e->device);
	const int rc = sgmCollect(e); if (rc) return rc;
	if (kernelMs) *kernelMs = e->rectMs;
	if (calls) *calls = e->rectCalls;
	return 0;
}

} // extern "C"
