// pm_host_image.hip -- the engine's image store (include/pmhip.h: pmhip_image_*, pmhip_scene_set_view_stored, pmhip_working_size, pmhip_scaled_size): part of
// pm_engine.hip's translation unit.  A decoded 8-bit image goes to the device once; the working-resolution BGR image, the gray float image and the resampled
// neighbour copies are made there (pm_image.hip) and adopted by scene views through device-to-device copies.
#include <float.h>

namespace {

#define IMGERR(e, msg) do { (e)->err = (msg); return PMHIP_E_ARG; } while (0)

int imgBlocks(size_t items) { return (int)std::min<size_t>((items + 255) / 256, 8192); }

// uploads one axis table next to the others of its kind (grow-only buffers of the store)
int imgUploadTab(pmhip_engine* e, const PMImgHostTab& t, ImageStore::AreaTab& d, PMImgTab& out) {
	HIPCHK(e, d.ofs.reserve(t.ofs.size())); HIPCHK(e, d.si.reserve(std::max<size_t>(t.si.size(), 1))); HIPCHK(e, d.al.reserve(std::max<size_t>(t.al.size(), 1)));
	HIPCHK(e, hipMemcpyAsync(d.ofs, t.ofs.data(), sizeof(int) * t.ofs.size(), hipMemcpyHostToDevice, e->stream));
	if (!t.si.empty()) {
		HIPCHK(e, hipMemcpyAsync(d.si, t.si.data(), sizeof(int) * t.si.size(), hipMemcpyHostToDevice, e->stream));
		HIPCHK(e, hipMemcpyAsync(d.al, t.al.data(), sizeof(float) * t.al.size(), hipMemcpyHostToDevice, e->stream));
	}
	out = PMImgTab{d.ofs, d.si, d.al};
	return 0;
}
int imgUploadCubic(pmhip_engine* e, const PMImgHostCubic& t, ImageStore::CubicTab& d, PMImgCubicTab& out) {
	HIPCHK(e, d.idx.reserve(t.idx.size())); HIPCHK(e, d.c.reserve(t.c.size()));
	HIPCHK(e, hipMemcpyAsync(d.idx, t.idx.data(), sizeof(int) * t.idx.size(), hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipMemcpyAsync(d.c, t.c.data(), sizeof(float) * t.c.size(), hipMemcpyHostToDevice, e->stream));
	out = PMImgCubicTab{d.idx, d.c};
	return 0;
}

int imgEvents(pmhip_engine* e) {
	for (hipEvent_t& ev : e->imgEv) if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, 0));
	return 0;
}
// the kernel between the two events has been enqueued: wait for it and add its time
int imgTimed(pmhip_engine* e) {
	HIPCHK(e, hipEventRecord(e->imgEv[1], e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	float ms = 0; HIPCHK(e, hipEventElapsedTime(&ms, e->imgEv[0], e->imgEv[1]));
	e->img.stats.kernelMs += ms;
	return 0;
}

template <int MODE> void imgLaunchU8(pmhip_engine* e, const PMImgU8& a) {
	const size_t groups = ((size_t)a.w * a.h + PMIMG_PPL - 1) / PMIMG_PPL;
	hipLaunchKernelGGL((pmimg_area_u8_kernel<MODE, PMIMG_PPL>), dim3(imgBlocks(groups)), dim3(256), 0, e->stream, a);
}

} // namespace

extern "C" {

int pmhip_working_size(int W0, int H0, unsigned nResolutionLevel, unsigned nMinResolution, unsigned nMaxResolution, int* w, int* h) {
	if (W0 < 1 || H0 < 1 || !w || !h) return PMHIP_E_ARG;
	// TImage::computeMaxResolution, libs/Common/Types.inl:2459-2477
	const unsigned size0 = (unsigned)std::max(W0, H0);
	auto shr = [size0](unsigned l) { return l < 32 ? size0 >> l : 0u; };
	unsigned res;
	if (nResolutionLevel == 0) res = std::min(size0, nMaxResolution);
	else {
		unsigned size = shr(nResolutionLevel);
		if (size < nMinResolution) {
			unsigned level = 0;
			while (shr(level + 1) >= nMinResolution && level < 32) ++level;
			size = shr(level);
		}
		res = std::min(size, nMaxResolution);
	}
	// Image::ResizeImage's size rule, libs/MVS/Image.cpp:139-150
	if (res == 0 || size0 <= res) { *w = W0; *h = H0; return 0; }
	const double scale = W0 > H0 ? (double)res / (double)W0 : (double)res / (double)H0;
	*w = (int)nearbyint((double)W0 * scale); *h = (int)nearbyint((double)H0 * scale);
	return 0;
}

int pmhip_scaled_size(int W, int H, float scale, int* w, int* h) {
	if (!(fabsf(scale - 1.f) >= 0.15f)) return 0;      // DepthData::ViewData::NeedScaleImage, in float
	const double s = (double)scale;
	if (w) *w = (int)nearbyint((double)W * s);
	if (h) *h = (int)nearbyint((double)H * s);
	return 1;
}

int pmhip_image_prepare(pmhip_engine* e, int key, const unsigned char* img, int W0, int H0, int channelOrder, int w, int h) {
	if (!e) return PMHIP_E_ARG;
	if (key < 0 || !img || W0 < 1 || H0 < 1 || channelOrder < 0 || channelOrder > 1) IMGERR(e, "pmhip_image_prepare: a key >= 0, an image of at least 1 x 1 and channelOrder 0 (BGR) or 1 (RGB)");
	if (w < 1 || h < 1) IMGERR(e, "pmhip_image_prepare: the working size must be at least 1 x 1");
	if (w > W0 || h > H0) IMGERR(e, "pmhip_image_prepare: INTER_AREA is implemented for shrinking only (the working size exceeds the stored size)");
	if ((uint64_t)W0 * (uint64_t)H0 > (1ull << 30)) IMGERR(e, "pmhip_image_prepare: more than 2^30 pixels");
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));          // a view may still be copying from the entry this one replaces
	int rc = imgEvents(e); if (rc) return rc;
	ImageStore& st = e->img;
	PMImgU8 a{};
	a.W = W0; a.H = H0; a.w = w; a.h = h; a.swapRB = channelOrder == 1;
	int mode;
	if (w == W0 && h == H0) mode = PMIMG_COPY;
	else if (W0 == 2 * w && H0 == 2 * h) mode = PMIMG_HALF;
	else if (W0 % w == 0 && H0 % h == 0) { mode = PMIMG_INT; a.fx = W0 / w; a.fy = H0 / h; a.inv = (float)(1.0 / ((double)a.fx * (double)a.fy)); }
	else {
		mode = PMIMG_TAB;
		if (st.u8Key[0] != W0 || st.u8Key[1] != H0 || st.u8Key[2] != w || st.u8Key[3] != h) {      // (a scene's images mostly share one size: the tables stay)
			PMImgHostTab tx, ty;
			if (!pmimg_area_tab(W0, w, (double)W0 / (double)w, tx) || !pmimg_area_tab(H0, h, (double)H0 / (double)h, ty)) IMGERR(e, "pmhip_image_prepare: area table out of range");
			st.u8Key[0] = 0;
			if ((rc = imgUploadTab(e, tx, st.u8x, st.u8tx)) != 0 || (rc = imgUploadTab(e, ty, st.u8y, st.u8ty)) != 0) return rc;
			HIPCHK(e, hipStreamSynchronize(e->stream));      // tx / ty live on this frame
			st.u8Key[0] = W0; st.u8Key[1] = H0; st.u8Key[2] = w; st.u8Key[3] = h;
		}
		a.tx = st.u8tx; a.ty = st.u8ty;
	}
	const size_t nSrc = (size_t)W0 * H0 * 3, P = (size_t)w * h;
	HIPCHK(e, st.src.reserve(nSrc));
	ImgEntry en;
	HIPCHK(e, en.bgr.alloc(P * 3)); HIPCHK(e, en.gray.alloc(P));
	en.w = w; en.h = h;
	const auto t0 = std::chrono::steady_clock::now();
	HIPCHK(e, hipMemcpyAsync(st.src, img, nSrc, hipMemcpyHostToDevice, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));              // the caller may free the image; and the upload's time is the host's
	st.stats.uploadMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	a.src = st.src; a.bgr = en.bgr; a.gray = en.gray;
	HIPCHK(e, hipEventRecord(e->imgEv[0], e->stream));
	switch (mode) {
	case PMIMG_COPY: imgLaunchU8<PMIMG_COPY>(e, a); break;
	case PMIMG_HALF: imgLaunchU8<PMIMG_HALF>(e, a); break;
	case PMIMG_INT: imgLaunchU8<PMIMG_INT>(e, a); break;
	default: imgLaunchU8<PMIMG_TAB>(e, a); break;
	}
	if ((rc = imgTimed(e)) != 0) return rc;
	st.entries[key] = std::move(en);
	st.stats.nPrepared += 1; st.stats.bytesUploaded += nSrc;
	return 0;
}

int pmhip_image_scale(pmhip_engine* e, int key, int srcKey, float scale, int* wOut, int* hOut) {
	if (!e) return PMHIP_E_ARG;
	if (key < 0) IMGERR(e, "pmhip_image_scale: a key >= 0");
	ImageStore& st = e->img;
	auto it = st.entries.find(srcKey);
	if (it == st.entries.end()) IMGERR(e, "pmhip_image_scale: unknown source key " + std::to_string(srcKey));
	if (!it->second.gray) IMGERR(e, "pmhip_image_scale: the source entry has no gray image");
	const int W = it->second.w, H = it->second.h;
	int w = 0, h = 0;
	if (!pmhip_scaled_size(W, H, scale, &w, &h)) IMGERR(e, "pmhip_image_scale: a scale within 15 % of 1 is not resampled (NeedScaleImage)");
	if (w < 1 || h < 1) IMGERR(e, "pmhip_image_scale: the scale leaves no image");
	if ((uint64_t)w * (uint64_t)h > (1ull << 30)) IMGERR(e, "pmhip_image_scale: more than 2^30 pixels");
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	int rc = imgEvents(e); if (rc) return rc;
	const double s = (double)scale, inv = 1.0 / s;          // OpenCV's scale_x = scale_y of the call
	const float* src = it->second.gray;
	ImgEntry en;
	en.w = w; en.h = h;
	const size_t P = (size_t)w * h;
	HIPCHK(e, en.gray.alloc(P));
	const int blocks = imgBlocks(P);
	if (s > 1) {
		PMImgHostCubic tx, ty; PMImgCubicTab dx, dy;
		pmimg_cubic_tab(w, W, inv, tx); pmimg_cubic_tab(h, H, inv, ty);
		if ((rc = imgUploadCubic(e, tx, st.cx, dx)) != 0 || (rc = imgUploadCubic(e, ty, st.cy, dy)) != 0) return rc;
		HIPCHK(e, hipStreamSynchronize(e->stream));
		HIPCHK(e, hipEventRecord(e->imgEv[0], e->stream));
		hipLaunchKernelGGL(pmimg_cubic_f32, dim3(blocks), dim3(256), 0, e->stream, src, W, (float*)en.gray, w, h, dx, dy);
	} else {
		const double fr = nearbyint(inv);
		if (fabs(inv - fr) < DBL_EPSILON) {
			const int f = (int)fr;
			HIPCHK(e, hipEventRecord(e->imgEv[0], e->stream));
			hipLaunchKernelGGL(pmimg_area_f32_block_kernel, dim3(blocks), dim3(256), 0, e->stream, src, W, H, (float*)en.gray, w, h, f, (float)(1.0 / ((double)f * (double)f)));
		} else {
			PMImgHostTab tx, ty; PMImgTab dx, dy;
			if (!pmimg_area_tab(W, w, inv, tx) || !pmimg_area_tab(H, h, inv, ty)) IMGERR(e, "pmhip_image_scale: area table out of range");
			if ((rc = imgUploadTab(e, tx, st.fx, dx)) != 0 || (rc = imgUploadTab(e, ty, st.fy, dy)) != 0) return rc;
			HIPCHK(e, hipStreamSynchronize(e->stream));
			HIPCHK(e, hipEventRecord(e->imgEv[0], e->stream));
			hipLaunchKernelGGL(pmimg_area_f32_tab_kernel, dim3(blocks), dim3(256), 0, e->stream, src, W, (float*)en.gray, w, h, dx, dy);
		}
	}
	if ((rc = imgTimed(e)) != 0) return rc;
	st.entries[key] = std::move(en);
	st.stats.nScaled += 1;
	if (wOut) *wOut = w;
	if (hOut) *hOut = h;
	return 0;
}

int pmhip_image_get(pmhip_engine* e, int key, int* w, int* h, float* gray, unsigned char* bgr) {
	if (!e) return PMHIP_E_ARG;
	auto it = e->img.entries.find(key);
	if (it == e->img.entries.end()) IMGERR(e, "pmhip_image_get: unknown key " + std::to_string(key));
	const ImgEntry& en = it->second;
	if (bgr && !en.bgr) IMGERR(e, "pmhip_image_get: the entry holds a gray image only");
	if (w) *w = en.w;
	if (h) *h = en.h;
	HIPCHK(e, hipSetDevice(e->device));
	const size_t P = (size_t)en.w * en.h;
	if (gray) HIPCHK(e, hipMemcpyAsync(gray, en.gray, sizeof(float) * P, hipMemcpyDeviceToHost, e->stream));
	if (bgr) HIPCHK(e, hipMemcpyAsync(bgr, en.bgr, 3 * P, hipMemcpyDeviceToHost, e->stream));
	HIPCHK(e, hipStreamSynchronize(e->stream));
	return 0;
}

int pmhip_image_drop(pmhip_engine* e, int key) {
	if (!e) return PMHIP_E_ARG;
	HIPCHK(e, hipSetDevice(e->device));
	HIPCHK(e, hipStreamSynchronize(e->stream));      // views adopt by asynchronous copies
	if (key < 0) { freeImages(e); return 0; }
	auto it = e->img.entries.find(key);
	if (it == e->img.entries.end()) IMGERR(e, "pmhip_image_drop: unknown key " + std::to_string(key));
	e->img.entries.erase(it);
	if (e->img.entries.empty()) freeImages(e);        // the staging and the tables live as long as there are entries
	return 0;
}

uint64_t pmhip_image_bytes(pmhip_engine* e) {
	if (!e) return 0;
	const ImageStore& st = e->img;
	size_t b = st.src.n;
	for (const auto& kv : st.entries) b += kv.second.bgr.n + sizeof(float) * kv.second.gray.n;
	for (const ImageStore::AreaTab* t : {&st.u8x, &st.u8y, &st.fx, &st.fy}) b += sizeof(int) * (t->ofs.n + t->si.n) + sizeof(float) * t->al.n;
	for (const ImageStore::CubicTab* t : {&st.cx, &st.cy}) b += sizeof(int) * t->idx.n + sizeof(float) * t->c.n;
	return (uint64_t)b;
}

int pmhip_image_stats_get(pmhip_engine* e, PMHipImageStats* out, int reset) {
	if (!e || !out) return PMHIP_E_ARG;
	*out = e->img.stats;
	if (reset) e->img.stats = PMHipImageStats{};
	return 0;
}

int pmhip_scene_set_view_stored(pmhip_engine* e, int idx, int key, const double K[9], const double R[9], const double C[3],
		float dMin, float dMax, const int32_t* neighbors, int nNeighbors) {
	if (!e) return PMHIP_E_ARG;
	auto it = e->img.entries.find(key);
	if (it == e->img.entries.end()) IMGERR(e, "pmhip_scene_set_view_stored: unknown key " + std::to_string(key));
	const ImgEntry& en = it->second;
	if (!en.gray) IMGERR(e, "pmhip_scene_set_view_stored: the entry has no gray image");
	if (idx < 0 || idx >= e->nImages) IMGERR(e, "pmhip_scene_set_view_stored: no such view");
	int rc = en.w == e->w && en.h == e->h ? pmhip_scene_set_view(e, idx, en.gray, 1, K, R, C, dMin, dMax, neighbors, nNeighbors)
	                                      : pmhip_scene_set_view_sized(e, idx, en.gray, en.w, en.h, 1, K, R, C, dMin, dMax, neighbors, nNeighbors);
	if (rc) return rc;
	return en.bgr ? sceneSetColor(e, idx, en.bgr, hipMemcpyDeviceToDevice) : 0;
}

} // extern "C"
