// Test scaffolding: csrc/vrg_refbatch_math.hpp compiled for the host (g++, -ffp-contract=off), so that the arithmetic of the reference-batch
// kernels is held to torch, numpy and Pillow without a GPU (tests/test_refbatch_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in resize_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_refbatch_math.hpp"

using namespace vrg;

extern "C" {

int hm_refbatch_check(const vrg_refbatch_desc* desc, int64_t n, int64_t src_floats, int64_t src_bytes, int64_t out_elems) {
    return rb_check(desc, n, src_floats, src_bytes, out_elems);
}

int hm_refbatch(const float* src_f32, int64_t src_floats, const uint8_t* src_u8, int64_t src_bytes, const vrg_refbatch_desc* desc, int64_t n,
                float* out, int64_t out_floats) {
    const int rc = rb_check(desc, n, src_floats, src_bytes, out_floats);
    if (rc != VRG_OK) return rc;
    rb_records_host(src_f32, src_u8, desc, n, out);
    return VRG_OK;
}

int hm_refbatch_quantise(const float* src_f32, int64_t src_floats, const vrg_refbatch_desc* desc, int64_t n, uint8_t* dst, int64_t dst_bytes) {
    const int rc = rb_check(desc, n, src_floats, 0, dst_bytes);
    if (rc != VRG_OK) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (!rb_quantise_ok(desc[i])) return VRG_ERR_BAD_ARG;
    rb_quantise_host(src_f32, desc, n, dst);
    return VRG_OK;
}

// the search of the kernels of csrc/vrg_refbatch.hip, as they call it: over the records' first_tile
int64_t hm_rb_find(const vrg_refbatch_desc* desc, int64_t n, int32_t tile) { return rb_find(desc, n, tile); }

}  // extern "C"
