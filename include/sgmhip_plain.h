/* sgmhip_plain.h -- plain SGM (minResolution = 0): one disparity range for every pixel, up to 1024 wide (csrc/sgm_kernels_wide.hip), part of the C ABI of libsgmhip.so.
 *
 * A companion of include/sgmhip.h, which includes it at its end: a host that includes sgmhip.h has these functions, and this header may also be included on its own.
 * They are declared here and not in sgmhip.h itself because that header's prototype list is pinned by number (tests/test_abi.py); the Python bindings read both
 * headers (openmvs_amd/sgm.py).  Conventions, error codes and the engine handle are sgmhip.h's. */
#ifndef SGMHIP_PLAIN_H_
#define SGMHIP_PLAIN_H_
#include "sgmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sgmhip_set_problem with ONE disparity range [minDisp, maxDisp) for every pixel of the valid grid and idx = pixel * (maxDisp - minDisp) -- what a plain (non-tSGM) Match
 * is given (SemiGlobalMatcher.cpp:643-684) -- stated as two integers: no pixel table travels, the engine fills its own on the device.  The range may hold
 * 1 .. SGMHIP_MAX_UNIFORM_DISP disparities (a design limit: the path kernel keeps up to 16 entries of the range per lane, csrc/sgm_kernels_wide.hip); anything else,
 * or a bound outside int16, is SGMHIP_E_ARG with the limit in sgmhip_last_error.  sgmhip_match, sgmhip_get_results, sgmhip_set_disparity and
 * sgmhip_refine_disparity work on the problem as on any other.  No memory for the volumes: SGMHIP_E_HIP, no problem is resident, the engine stays usable.
 * sgmhip_set_problem keeps its limit of 256 disparities per pixel. */
#define SGMHIP_MAX_UNIFORM_DISP 1024
int sgmhip_set_problem_uniform(sgmhip_engine* e, const uint8_t* leftBGR, const float* leftGray, const float* rightGray, int w, int h, int minDisp, int maxDisp);
/* The global range of plain SGM from the half-resolution seed disparity map (SemiGlobalMatcher.cpp:644-661), NO_DISP entries included, every intermediate a
 * Disparity (int16) that wraps as one: numDisp = (max - min) + 16, disp = min + max, [disp - numDisp, disp + numDisp).  Host only.  n == 0: SGMHIP_E_ARG. */
int sgmhip_plain_range(const int16_t* seed, size_t n, int16_t* minDisp, int16_t* maxDisp);

#ifdef __cplusplus
}
#endif
#endif /* SGMHIP_PLAIN_H_ */
