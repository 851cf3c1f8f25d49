// Test scaffolding: csrc/vrg_flf_math.hpp compiled for the host (g++, -ffp-contract=off), so that the arithmetic of the First / Last guide
// kernel is held to torch itself without a GPU (tests/test_flf_guide_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in resize_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_flf_math.hpp"

using namespace vrg;

extern "C" {

// g9: h, w, c, last_h, last_w, sx0, sy0, sw, sh
int hm_flf_guide(const float* first, const float* last, const float* weights, float* out, int64_t frames, const int32_t* g9) {
    const int rc = flf_check(frames, g9[0], g9[1], g9[2], g9[3], g9[4], g9[5], g9[6], g9[7], g9[8]);
    if (rc != VRG_OK) return rc;
    flf_guide_host(first, last, weights, out, frames, FlfGeom{g9[0], g9[1], g9[2], g9[3], g9[4], g9[5], g9[6], g9[7], g9[8]});
    return VRG_OK;
}

}  // extern "C"
