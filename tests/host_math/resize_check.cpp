// Test scaffolding: csrc/vrg_resize_math.hpp compiled for the host (g++, -ffp-contract=off), so that the resampling arithmetic of the
// resize / restore kernels is checked against the recorded reference results without a GPU (tests/test_resize_host.py), and serves
// as the expected value of the GPU tests on shapes too large for a fixture.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in host_math_check.cpp); the resize arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_resize_math.hpp"

using namespace vrg;

static ResizeGeom geom(const int32_t* g) {
    return ResizeGeom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12]};
}

extern "C" {

// g: in_h, in_w, in_c, sx0, sy0, sw, sh, out_h, out_w, dx0, dy0, dw, dh
void hm_resize(const float* in, float* out, int64_t frames, const int32_t* g13, int32_t method) {
    const ResizeGeom g = geom(g13);
    for (int64_t f = 0; f < frames; ++f) {
        const float* fr = in + f * (int64_t)g.in_h * g.in_w * g.in_c;
        float* dst = out + f * (int64_t)g.out_h * g.out_w * 3;
        auto load = [&](int32_t y, int32_t x, int c) { return fr[((int64_t)y * g.in_w + x) * g.in_c + c]; };
        for (int32_t y = 0; y < g.out_h; ++y)
            for (int32_t x = 0; x < g.out_w; ++x) rs_pixel(g, method, x, y, load, dst + ((int64_t)y * g.out_w + x) * 3);
    }
}

void hm_restore(const float* work, const float* originals, float* out, int64_t work_frames, int64_t frames, const int32_t* g13,
                int32_t channels, int32_t method, float s, float oms) {
    const ResizeGeom g = geom(g13);
    const int64_t usable = work_frames < frames ? work_frames : frames;
    const int64_t fe = (int64_t)g.out_h * g.out_w * channels;
    for (int64_t f = 0; f < frames; ++f) {
        const float* fr = work + f * (int64_t)g.in_h * g.in_w * g.in_c;
        auto load = [&](int32_t y, int32_t x, int c) { return fr[((int64_t)y * g.in_w + x) * g.in_c + c]; };
        for (int32_t y = 0; y < g.out_h; ++y)
            for (int32_t x = 0; x < g.out_w; ++x) {
                const int64_t e = f * fe + ((int64_t)y * g.out_w + x) * channels;
                for (int c = 0; c < channels; ++c) out[e + c] = clamp01(originals[e + c]);
                if (f < usable) {
                    float r[3];
                    rs_pixel(g, method, x, y, load, r);
                    for (int c = 0; c < 3; ++c) out[e + c] = rs_blend(originals[e + c], r[c], s, oms);
                }
            }
    }
}

}  // extern "C"
