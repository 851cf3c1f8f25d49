// vrg_flf_math.hpp -- arithmetic of the LTX First / Last temporal guide (csrc/vrg_flf.hip), host and device.
//
// What is restated: VRGDG_LTXFirstLastGuide.add_first_last_guide of the reference (VRGDG_LTXFirstLastGuide.py:52-69).  `last` is brought to
// the size of `first` by comfy.utils.common_upscale(last.movedim(-1, 1), w, h, "bilinear", "center"): a centre-crop rectangle (planned on
// the host, ops.center_crop_rect) narrowed out of the channels-last view and F.interpolate(mode="bilinear") over it -- the bilinear rule of
// vrg_resize_math.hpp, taps clamped to the rectangle, NOT clamped to [0, 1].  When `last` already has the size the reference skips the
// call: its values are taken as they are and no filter is evaluated.  Every frame is then first * (1.0 - amount) + last * amount on fp32
// tensors with Python doubles: torch rounds each scalar to fp32 and computes fl(fl(first * w0) + fl(last' * w1)); a weight of 0 still
// multiplies (0 * Inf = NaN).  The caller passes w0 = (float)(1.0 - amount), w1 = (float)amount.
//
// Which of torch's two bilinear kernels runs (rs_bilinear_value): the channels-last kernel when the narrowed view is channels-last
// contiguous and has more than 3 channels, or when the output height + width is at most 128; the generic separable kernel otherwise
// (ATen/native/cpu/UpSampleKernel.cpp: _use_vectorized_kernel_cond_2d, torch with at least two threads).  A one-picture NHWC view narrowed
// in rows only stays contiguous, one narrowed in columns does not unless a single row is left.
// tests/test_flf_guide_host.py holds this header, compiled for the host, to torch itself run live.
#pragma once
#include "vrg_common.hpp"
#include "vrg_resize_math.hpp"

namespace vrg {

constexpr int FLF_CHUNK = 32;                       // frames one workgroup writes (blockIdx.y = chunk)
constexpr int64_t FLF_MAX_FRAMES = 65535ll * FLF_CHUNK;

struct FlfGeom {
    int32_t h, w, c;                                // `first` and every output frame: [h][w][c]
    int32_t last_h, last_w;                         // `last`: [last_h][last_w][c]
    int32_t sx0, sy0, sw, sh;                       // the centre-crop rectangle of `last`
};

// no resample: `last` has the size of `first` (the rectangle is then the whole picture)
VRG_HD bool flf_plain(const FlfGeom& g) {
    return g.last_h == g.h && g.last_w == g.w && g.sx0 == 0 && g.sy0 == 0 && g.sw == g.w && g.sh == g.h;
}

// torch's kernel choice for the narrowed view (see above)
VRG_HD bool flf_paired(const FlfGeom& g) {
    return rs_bilinear_paired(rs_view_contiguous(1, g.last_h, g.last_w, g.sw, g.sh), g.c, g.h, g.w);
}

inline int flf_check(int64_t frames, int32_t h, int32_t w, int32_t channels, int32_t last_h, int32_t last_w, int32_t sx0, int32_t sy0,
                     int32_t sw, int32_t sh) {
    if (frames < 0 || h < 1 || w < 1 || last_h < 1 || last_w < 1 || (channels != 3 && channels != 4)) return VRG_ERR_BAD_ARG;
    if (sx0 < 0 || sy0 < 0 || sw < 1 || sh < 1 || (int64_t)sx0 + sw > last_w || (int64_t)sy0 + sh > last_h) return VRG_ERR_BAD_ARG;
    // in-frame offsets are 32-bit, frames are addressed with 64 bits
    if ((int64_t)h * w * channels > 0x7fffffff || (int64_t)last_h * last_w * channels > 0x7fffffff || frames > FLF_MAX_FRAMES)
        return VRG_ERR_UNSUPPORTED;
    return VRG_OK;
}

// last' at element e of the flattened [h][w][c] picture; `load(i)` = element i of the flattened `last`
template <typename LOAD>
VRG_HD float flf_last_value(const FlfGeom& g, bool plain, bool paired, uint32_t e, LOAD load) {
    if (plain) return load((int64_t)e);
    const uint32_t px = e / (uint32_t)g.c, ch = e - px * (uint32_t)g.c;
    const int32_t y = (int32_t)(px / (uint32_t)g.w), x = (int32_t)(px - (uint32_t)y * (uint32_t)g.w);
    int32_t ix[2], iy[2];
    float wx[2], wy[2];
    rs_linear_taps(x, rs_scale(g.sw, g.w), g.sw, ix, wx);
    rs_linear_taps(y, rs_scale(g.sh, g.h), g.sh, iy, wy);
    const int64_t r0 = (int64_t)(g.sy0 + iy[0]) * g.last_w, r1 = (int64_t)(g.sy0 + iy[1]) * g.last_w;
    const int64_t c0 = g.sx0 + ix[0], c1 = g.sx0 + ix[1];
    return rs_bilinear_value(paired, wx, wy, load((r0 + c0) * g.c + ch), load((r0 + c1) * g.c + ch), load((r1 + c0) * g.c + ch),
                             load((r1 + c1) * g.c + ch));
}

// one value of one frame
VRG_HD float flf_blend(float first, float last, float w0, float w1) { return first * w0 + last * w1; }

// vrg_flf_guide_f32 in plain loops (tests/host_math/flf_check.cpp)
inline void flf_guide_host(const float* first, const float* last, const float* weights, float* out, int64_t frames, const FlfGeom& g) {
    const int64_t n = (int64_t)g.h * g.w * g.c;
    const bool plain = flf_plain(g), paired = flf_paired(g);
    for (int64_t e = 0; e < n; ++e) {
        const float a = first[e], b = flf_last_value(g, plain, paired, (uint32_t)e, [&](int64_t i) { return last[i]; });
        for (int64_t f = 0; f < frames; ++f) out[f * n + e] = flf_blend(a, b, weights[2 * f], weights[2 * f + 1]);
    }
}

}  // namespace vrg
