// Test scaffolding: the detector-input arithmetic of csrc/vrg_detect_math.hpp on the host -- the header compiled with g++
// (-ffp-contract=off): the bilinear byte warp and the bilinear byte resize as whole-image loops over dt_warp_pixel / dt_resize_pixel, the
// fused blob exactly as the kernel composes it (no rotated frame in between), the tap tables and the matrices.  Checked byte for byte
// against the independent numpy restatement of tests/detect_support.py (tests/test_detect_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_detect_math.hpp"

using namespace vrg;

namespace {

struct Source {
    const void* base;
    int32_t W, C;
    bool f32;
    void operator()(int32_t y, int32_t x, uint8_t b[3]) const {
        const int64_t at = ((int64_t)y * W + x) * C;
        if (f32) {
            const float* p = reinterpret_cast<const float*>(base) + at;
            b[0] = wp_quantise(p[2]); b[1] = wp_quantise(p[1]); b[2] = wp_quantise(p[0]);
        } else {
            const uint8_t* p = reinterpret_cast<const uint8_t*>(base) + at;
            b[0] = p[0]; b[1] = p[1]; b[2] = p[2];
        }
    }
};

}  // namespace

extern "C" {

void hm_detect_taps(int32_t n_in, int32_t n_out, int32_t* ofs, int16_t* coef) { dt_fill_taps(n_in, n_out, ofs, coef); }

// forward and inverse 2 x 3 of one rotation from its cosine and sine
void hm_detect_rotation(double cos_a, double sin_a, int32_t W, int32_t H, double* forward, double* inverse) {
    dt_rotation(cos_a, sin_a, W, H, forward);
    dt_invert(forward, inverse);
}

// frame: [H][W][C] fp32 R,G,B -> [H][W][3] B,G,R bytes
void hm_detect_quantise(const float* frame, uint8_t* out, int32_t H, int32_t W, int32_t C) {
    const Source src{frame, W, C, true};
    for (int32_t y = 0; y < H; ++y)
        for (int32_t x = 0; x < W; ++x) src(y, x, out + ((int64_t)y * W + x) * 3);
}

// in, out: [H][W][3] bytes; m: the INVERTED matrix
void hm_detect_warp(const uint8_t* in, uint8_t* out, const double* m, int32_t H, int32_t W) {
    const Source src{in, W, 3, false};
    for (int32_t y = 0; y < H; ++y)
        for (int32_t x = 0; x < W; ++x) dt_warp_pixel(m, x, y, W, H, src, out + ((int64_t)y * W + x) * 3);
}

// in: [rh][rw][3] bytes, out: [n_out][n_out][3] bytes
void hm_detect_resize(const uint8_t* in, uint8_t* out, int32_t rh, int32_t rw, int32_t n_out) {
    const Source src{in, rw, 3, false};
    for (int32_t y = 0; y < n_out; ++y)
        for (int32_t x = 0; x < n_out; ++x) dt_resize_pixel(x, y, rw, rh, n_out, src, out + ((int64_t)y * n_out + x) * 3);
}

// The blob of one descriptor as the kernel composes it.  frames: [n][H][W][C] fp32 R,G,B (f32 != 0) or [n][H][W][3] bytes; transforms: [.][6];
// desc: six int32; out: fp32 [3][300][300].  Returns 0 when the descriptor is refused (out zeroed).
int hm_detect_blob(const void* frames, int32_t f32, int64_t n_frames, int32_t H, int32_t W, int32_t C, const double* transforms, int64_t n_transforms,
                   const int32_t* desc, float* out) {
    const vrg_detect_desc d{desc[0], desc[1], desc[2], desc[3], desc[4], desc[5]};
    if (!dt_desc_ok(d, n_frames, n_transforms, H, W)) {
        for (int i = 0; i < 3 * DT_BLOB_PIXELS; ++i) out[i] = 0.0f;
        return 0;
    }
    const int64_t elems = (int64_t)H * W * C;
    const Source src{f32 ? (const void*)(reinterpret_cast<const float*>(frames) + d.frame * elems)
                         : (const void*)(reinterpret_cast<const uint8_t*>(frames) + d.frame * elems), W, C, f32 != 0};
    const double* m = d.transform >= 0 ? transforms + 6 * (int64_t)d.transform : nullptr;
    for (int32_t dy = 0; dy < DT_BLOB; ++dy)
        for (int32_t dx = 0; dx < DT_BLOB; ++dx) {
            uint8_t b[3];
            if (m)
                dt_resize_pixel(dx, dy, d.right - d.left, d.bottom - d.top, DT_BLOB,
                                [&](int32_t y, int32_t x, uint8_t v[3]) { dt_warp_pixel(m, d.left + x, d.top + y, W, H, src, v); }, b);
            else
                dt_resize_pixel(dx, dy, d.right - d.left, d.bottom - d.top, DT_BLOB,
                                [&](int32_t y, int32_t x, uint8_t v[3]) { src(d.top + y, d.left + x, v); }, b);
            for (int c = 0; c < 3; ++c) out[c * DT_BLOB_PIXELS + dy * DT_BLOB + dx] = (float)b[c] - dt_mean(c);
        }
    return 1;
}

}  // extern "C"
