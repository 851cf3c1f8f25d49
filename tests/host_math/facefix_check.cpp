// Test scaffolding: csrc/vrg_facefix_math.hpp on the host -- the header compiled with g++ (-ffp-contract=off): the span table, the
// Gaussian coefficients, the two blur passes through an fp32 plane, and the mean shift + blend of one box.  Checked against the
// independent numpy restatement of tests/facefix_builder_support.py (tests/test_facefix_builder_host.py): masks bit for bit, bytes value
// for value.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_facefix_math.hpp"

using namespace vrg;

extern "C" {

// spans: [height][2] int32
void hm_ff_spans(int32_t width, int32_t height, int32_t* spans) { ff_ellipse_spans(width, height, reinterpret_cast<FfSpan*>(spans)); }

// coeffs: max(3, 4 * feather + 1) floats
void hm_ff_coeffs(int32_t feather, float* coeffs) { ff_gauss_coeffs(feather, coeffs); }

// mask: [height][width] fp32 = _soft_ellipse_mask(width, height, feather)
void hm_ff_mask(int32_t width, int32_t height, int32_t feather, float* mask) {
    std::vector<FfSpan> spans((size_t)height);
    ff_ellipse_spans(width, height, spans.data());
    if (feather <= 0) {
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) mask[(size_t)y * width + x] = (x >= spans[y].x0 && x <= spans[y].x1) ? 1.0f : 0.0f;
        return;
    }
    const int32_t n = ff_gauss_taps(feather);
    std::vector<float> c((size_t)n), plane((size_t)width * height);
    ff_gauss_coeffs(feather, c.data());
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) plane[(size_t)y * width + x] = ff_blur_h(c.data(), n, spans[y], width, x);
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x)
            mask[(size_t)y * width + x] = ff_blur_v(c.data(), n, height, y, [&](int32_t row) { return plane[(size_t)row * width + x]; });
}

// target, face, out: [h][w][3] bytes; mask [h][w]; sums: count, face B G R, target B G R
void hm_ff_composite(const uint8_t* target, const uint8_t* face, const float* mask, int32_t h, int32_t w, float color_match, float strength,
                     uint8_t* out, int64_t* sums_out) {
    uint64_t sums[FF_STAT_SUMS] = {0, 0, 0, 0, 0, 0, 0};
    const size_t n = (size_t)h * w;
    for (size_t p = 0; p < n; ++p) {
        if (!ff_selected(mask[p])) continue;
        sums[0] += 1;
        for (int c = 0; c < 3; ++c) {
            sums[1 + c] += face[p * 3 + c];
            sums[4 + c] += target[p * 3 + c];
        }
    }
    for (int i = 0; i < FF_STAT_SUMS; ++i) sums_out[i] = (int64_t)sums[i];
    float shift[3];
    const bool matched = ff_shifts(sums, color_match, shift);
    for (size_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c) {
            uint8_t f = face[p * 3 + c];
            if (matched) f = ff_shift_byte(f, shift[c]);
            out[p * 3 + c] = ff_blend_byte(target[p * 3 + c], f, mask[p], strength);
        }
}

}  // extern "C"
