// Test scaffolding: csrc/vrg_anchor_math.hpp compiled for the host (g++, -ffp-contract=off), so that the load and store rules of the anchor
// kernels are held to live Pillow and numpy without a GPU (tests/test_anchor_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in resize_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_anchor_math.hpp"

using namespace vrg;

extern "C" {

int hm_anchor_check(const vrg_anchor_desc* desc, int64_t n, const int32_t* tables, int64_t table_ints, int64_t src_bytes, int32_t out_h,
                    int32_t out_w) {
    return anchor_check(desc, n, tables, table_ints, src_bytes, out_h, out_w);
}

// vrg_anchor_frames_f32 in plain loops, launched in the chunks the kernel is launched in; calls[0] counts the launches
int hm_anchor_frames(const uint8_t* src, int64_t src_bytes, const vrg_anchor_desc* desc, int64_t n, const int32_t* tables, int64_t table_ints,
                     float* out, int32_t out_h, int32_t out_w, int32_t* calls) {
    const int rc = anchor_check(desc, n, tables, table_ints, src_bytes, out_h, out_w);
    if (rc != VRG_OK) return rc;
    const AnchorGeom g{src_bytes, table_ints, out_h, out_w};
    const int64_t frame_values = (int64_t)out_h * out_w * 3;
    return anchor_launches(n, [&](int64_t first, int64_t count) -> int {
        if (calls) ++calls[0];
        for (int64_t i = 0; i < count; ++i) anchor_frame_host(src, desc[first + i], tables, g, out + (first + i) * frame_values);
        return VRG_OK;
    });
}

void hm_anchor_store(const float* in, int64_t pixels, int32_t channels, int32_t order, uint8_t* out) {
    anchor_store_host(in, pixels, channels, order, out);
}

int32_t hm_anchor_constant(int32_t which) {
    return which == 0 ? ANC_TW : which == 1 ? ANC_TH : which == 2 ? ANC_SLOTS : which == 3 ? (int32_t)LAUNCH_RECORDS : (int32_t)ANCHOR_NAN_BYTE;
}

}  // extern "C"
