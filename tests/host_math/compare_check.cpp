// Test scaffolding: csrc/vrg_compare_math.hpp compiled for the host (g++, -ffp-contract=off), so that the rgb24 rule of the compare kernel is
// held to live numpy without a GPU (tests/test_compare_host.py); anchor_store_byte of csrc/vrg_anchor_math.hpp beside it, for the levels
// at which rounding and truncation part.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in anchor_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_compare_math.hpp"
#include "vrg_anchor_math.hpp"

using namespace vrg;

extern "C" {

void hm_rgb24_frames(const float* src, int64_t pixels, int32_t channels, uint8_t* dst) { rgb24_frames_host(src, pixels, channels, dst); }

void hm_anchor_bytes(const float* values, int64_t n, uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = anchor_store_byte(values[i]);
}

int hm_rgb24_nan_byte(void) { return RGB24_NAN_BYTE; }

}  // extern "C"
