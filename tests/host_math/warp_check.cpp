// Test scaffolding: the byte Lanczos-4 affine warp of csrc/vrg_warp_math.hpp on the host -- the header compiled with g++
// (-ffp-contract=off): wp_phase_table makes the weights, wp_record the record, wp_source / wp_pixel evaluate every result pixel.  Checked
// byte for byte against the independent numpy restatement of tests/warp_support.py (tests/test_warp_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_warp_math.hpp"

using namespace vrg;

extern "C" {

int64_t hm_warp_desc_bytes() { return (int64_t)sizeof(vrg_warp_desc); }

// table: 1024 x 64 int16
void hm_warp_phase_table(int16_t* table) { wp_phase_table(table); }

// 1 = the record was made, 0 = refused
int hm_warp_record(const float* transform, int32_t out_w, int32_t out_h, int32_t src_w, int32_t src_h, int64_t src_offset, void* rec) {
    return wp_record(transform, out_w, out_h, src_w, src_h, src_offset, reinterpret_cast<vrg_warp_desc*>(rec)) ? 1 : 0;
}

// in: [in_h][in_w][3] bytes, out: [out_h][out_w][3] bytes; returns 0 when the transform is refused (out untouched)
int hm_warp_affine(const uint8_t* in, uint8_t* out, const float* transform, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
    static std::vector<int16_t> table;
    if (table.empty()) {
        table.resize((size_t)WP_PHASES * WP_KERNEL);
        wp_phase_table(table.data());
    }
    vrg_warp_desc r;
    if (!wp_record(transform, out_w, out_h, in_w, in_h, 0, &r)) return 0;
    auto load = [&](int32_t y, int32_t x, int c) { return in[((int64_t)y * in_w + x) * 3 + c]; };
    for (int32_t y = 0; y < out_h; ++y) {
        for (int32_t x = 0; x < out_w; ++x) {
            int32_t sx, sy, phase;
            wp_source(r.m, x, y, sx, sy, phase);
            wp_pixel(table.data() + (size_t)phase * WP_KERNEL, sx, sy, in_w, in_h, load, out + ((int64_t)y * out_w + x) * 3);
        }
    }
    return 1;
}

// uint8(clip(rint(v * 255), 0, 255)) of n floats
void hm_warp_quantise(const float* v, uint8_t* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = wp_quantise(v[i]);
}

}  // extern "C"
