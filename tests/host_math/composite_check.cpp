// Test scaffolding: csrc/vrg_composite_math.hpp compiled for the host (g++, -ffp-contract=off), so that the arithmetic of the feathered
// crop composite is checked against the recorded reference results without a GPU (tests/test_composite_host.py), and serves as the
// expected value of the GPU tests on shapes too large for a fixture.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in host_math_check.cpp); the composite uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_composite_math.hpp"

using namespace vrg;

namespace {

// g: crop_h, crop_w, crop_c, height, width, channels, mask_h, mask_w, mask_stride, match_channels
struct Geom {
    int32_t crop_h, crop_w, crop_c, H, W, C, mask_h, mask_w, mask_stride, nc;
};

Geom geom(const int32_t* g) { return Geom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9]}; }

float eval(const vrg_composite_desc& d, const Geom& g, const float* crops, const float* user_mask, int32_t dx, int32_t dy, float v[4]) {
    const float* um = (d.flags & VRG_COMPOSITE_USER_MASK) ? user_mask + (int64_t)d.mask_index * g.mask_h * g.mask_w * g.mask_stride : nullptr;
    auto load_mask = [&](int32_t y, int32_t x) { return um[((int64_t)y * g.mask_w + x) * g.mask_stride]; };
    const float alpha = cp_alpha_masked(d, g.mask_h, g.mask_w, dx, dy, load_mask);
    const float* cf = crops + (int64_t)d.crop_index * g.crop_h * g.crop_w * g.crop_c;
    auto load = [&](int32_t y, int32_t x, int c) { return cf[((int64_t)y * g.crop_w + x) * g.crop_c + c]; };
    cp_crop(d, g.crop_h, g.crop_w, g.nc, dx, dy, load, v);
    return alpha;
}

}  // namespace

extern "C" {

// out[i] = cp_linspace(i, n, step): torch.linspace(-1, 1, n) as the radial rules evaluate it
void hm_composite_linspace(int32_t n, float step, float* out) {
    for (int32_t i = 0; i < n; ++i) out[i] = cp_linspace(i, n, step);
}

// alpha [paste_h][paste_w] and the resampled crop [paste_h][paste_w][4] of ONE record
void hm_composite_box(const float* crops, const float* user_mask, const vrg_composite_desc* d, const int32_t* g10, float* alpha, float* crop) {
    const Geom g = geom(g10);
    for (int32_t dy = 0; dy < d->paste_h; ++dy)
        for (int32_t dx = 0; dx < d->paste_w; ++dx) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int64_t e = (int64_t)dy * d->paste_w + dx;
            alpha[e] = eval(*d, g, crops, user_mask, dx, dy, v);
            for (int c = 0; c < 4; ++c) crop[e * 4 + c] = v[c];
        }
}

// the stats records (16 words each) of the frames that ask for a colour match: fp64 sums in raster order
void hm_composite_stats(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc, int64_t frames,
                        const int32_t* g10, uint32_t* stats) {
    const Geom g = geom(g10);
    for (int64_t f = 0; f < frames; ++f) {
        const vrg_composite_desc& d = desc[f];
        for (int i = 0; i < CP_STATS_WORDS; ++i) stats[f * CP_STATS_WORDS + i] = 0u;
        if (d.rule == VRG_COMPOSITE_NONE || !(d.flags & VRG_COMPOSITE_MATCH)) continue;
        double sums[CP_PART_DOUBLES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const float* of = originals + (int64_t)d.original_index * g.H * g.W * g.C;
        for (int32_t dy = 0; dy < d.paste_h; ++dy)
            for (int32_t dx = 0; dx < d.paste_w; ++dx) {
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                const float alpha = eval(d, g, crops, user_mask, dx, dy, v);
                if (!cp_selected(d, alpha)) continue;
                const float* t = of + ((int64_t)(d.top + dy) * g.W + d.left + dx) * g.C;
                sums[0] += 1.0;
                for (int c = 0; c < g.nc; ++c) {
                    sums[1 + c] += (double)v[c];
                    sums[5 + c] += (double)t[c];
                }
            }
        cp_finalize(d, sums, g.nc, stats + f * CP_STATS_WORDS);
    }
}

// out [frames][H][W][C] and mask [frames][H][W] given the stats records
void hm_composite_apply(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc, const uint32_t* stats,
                        int64_t frames, const int32_t* g10, float* out, float* mask) {
    const Geom g = geom(g10);
    for (int64_t f = 0; f < frames; ++f) {
        const vrg_composite_desc& d = desc[f];
        const float* of = originals + (int64_t)d.original_index * g.H * g.W * g.C;
        const uint32_t* rec = stats + f * CP_STATS_WORDS;
        const bool matched = (d.flags & VRG_COMPOSITE_MATCH) && rec[1] != 0u;
        for (int32_t y = 0; y < g.H; ++y)
            for (int32_t x = 0; x < g.W; ++x) {
                const int64_t px = (int64_t)y * g.W + x;
                const float* in = of + px * g.C;
                float* o = out + (f * (int64_t)g.H * g.W + px) * g.C;
                float& m = mask[f * (int64_t)g.H * g.W + px];
                const bool raw = d.rule == VRG_COMPOSITE_NONE && (d.flags & VRG_COMPOSITE_RAW_COPY);
                for (int c = 0; c < g.C; ++c) o[c] = raw ? in[c] : clamp01(in[c]);
                m = 0.0f;
                const int32_t dx = x - d.left, dy = y - d.top;
                if (d.rule == VRG_COMPOSITE_NONE || dx < 0 || dx >= d.paste_w || dy < 0 || dy >= d.paste_h) continue;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                const float alpha = eval(d, g, crops, user_mask, dx, dy, v);
                for (int c = 0; c < g.nc; ++c) o[c] = cp_blend(in[c], v[c], alpha, matched, matched ? f32_from_bits(rec[10 + c]) : 0.0f);
                m = alpha;
            }
    }
}

}  // extern "C"
