// vrg_composite_math.hpp -- arithmetic of the feathered crop composite (csrc/vrg_composite.hip), host and device.
//
// What is restated, in the reference's rounding order (fp32, one rounding per operation, -ffp-contract=off; a Python double that meets
// a tensor is cast to fp32 first, as torch does; tensor / scalar is the IEEE quotient and ** 2 is x * x on torch's CPU):
//   VRGDG_ImagePasteBack.py:11-30   _soft_blend_mask (ellipse / rectangle, inset, feather), :33-41 _match_color, :238-259 paste_back
//   VRGDG_StandaloneFaceFixNodes.py:835-847 VRGDGFaceFixComposite (radial alpha from torch.linspace, colour match, blend)
//   VRGDG_StandaloneFaceFixNodes.py:900-914 VRGDGFaceFixCompositeOpaque (alpha from an edge width)
// torch.linspace(-1, 1, n) in fp32 is restated element by element: step = 2 / (n - 1); the first n / 2 elements are -1 + step * i, the
// others 1 - step * (n - 1 - i); n = 1 gives -1.  The square root is the correctly rounded one (the GPU's, libm's and torch's own
// loop); torch's CPU build hands contiguous tensors to a vendor vector library whose sqrt is off by one ulp in under 1 % of the
// elements on some processors -- tools/make_golden_composite.py records the reference with the correctly rounded root.
// The kernels and the host check (tests/host_math/composite_check.cpp) call the SAME functions.
#pragma once
#include "../../include/vrgdg_hip.h"
#include "vrg_resize_math.hpp"

namespace vrg {

constexpr int CP_STATS_WORDS = 16;      // the per-frame stats record, 32-bit words (include/vrgdg_hip.h)
constexpr int CP_PART_DOUBLES = 9;      // one partial: selected count, 4 source sums, 4 target sums

// element i of torch.linspace(-1, 1, n, dtype=float32); step = 2.0f / (float)(n - 1), formed by the caller
VRG_HD float cp_linspace(int32_t i, int32_t n, float step) {
    if (n == 1) return -1.0f;
    return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - i - 1);
}

// The analytic alpha of box pixel (dx, dy), before the user mask.  d.p[] holds the rule's fp32 constants (include/vrgdg_hip.h).
VRG_HD float cp_alpha(const vrg_composite_desc& d, int32_t dx, int32_t dy) {
    const float* p = d.p;
    const bool step = (d.flags & VRG_COMPOSITE_STEP) != 0;
    if (d.rule == VRG_COMPOSITE_ELLIPSE || d.rule == VRG_COMPOSITE_RECTANGLE) {
        const float xx = (float)dx, yy = (float)dy;
        float distance;
        if (d.rule == VRG_COMPOSITE_ELLIPSE) {
            const float ax = (xx - p[0]) / p[2], ay = (yy - p[1]) / p[3];
            distance = (1.0f - __builtin_sqrtf(ax * ax + ay * ay)) * p[4];
        } else {
            const float mx = __builtin_fminf(xx - p[0], p[1] - xx), my = __builtin_fminf(yy - p[0], p[2] - yy);
            distance = __builtin_fminf(mx, my);
        }
        if (step) return distance >= 0.0f ? 1.0f : 0.0f;
        return clamp01(distance / p[5]);
    }
    const float xx = cp_linspace(dx, d.box_w, p[0]), yy = cp_linspace(dy, d.box_h, p[1]);
    const float radius = __builtin_sqrtf(xx * xx + yy * yy);
    if (d.rule == VRG_COMPOSITE_RADIAL) return clamp01((1.0f - radius) / p[2]) * p[3];
    if (step) return radius <= 1.0f ? 1.0f : 0.0f;                          // VRG_COMPOSITE_OPAQUE
    return clamp01((1.0f - radius) / p[2]);
}

// The user mask of Paste Back at box pixel (dx, dy): the [mask_h][mask_w] mask resized to the box with F.interpolate(bilinear,
// align_corners=False), clamped.  torch picks the four-products kernel while box_h + box_w <= 128 and the separable one above, as for
// frames (vrg_resize_math.hpp).  load(y, x) reads the mask.
template <typename LOAD>
VRG_HD float cp_user_mask(const vrg_composite_desc& d, int32_t mask_h, int32_t mask_w, int32_t dx, int32_t dy, LOAD load) {
    int32_t ix[2], iy[2];
    float wx[2], wy[2];
    rs_linear_taps(dx, rs_scale(mask_w, d.box_w), mask_w, ix, wx);
    rs_linear_taps(dy, rs_scale(mask_h, d.box_h), mask_h, iy, wy);
    const float i00 = load(iy[0], ix[0]), i01 = load(iy[0], ix[1]), i10 = load(iy[1], ix[0]), i11 = load(iy[1], ix[1]);
    const float v = d.box_h + d.box_w <= 128
                        ? (wy[0] * wx[0]) * i00 + (wy[0] * wx[1]) * i01 + (wy[1] * wx[0]) * i10 + (wy[1] * wx[1]) * i11
                        : (i00 * wx[0] + i01 * wx[1]) * wy[0] + (i10 * wx[0] + i11 * wx[1]) * wy[1];
    return clamp01(v);
}

// alpha of a box pixel with the user mask multiplied in
template <typename LOAD>
VRG_HD float cp_alpha_masked(const vrg_composite_desc& d, int32_t mask_h, int32_t mask_w, int32_t dx, int32_t dy, LOAD load_mask) {
    const float a = cp_alpha(d, dx, dy);
    return (d.flags & VRG_COMPOSITE_USER_MASK) ? a * cp_user_mask(d, mask_h, mask_w, dx, dy, load_mask) : a;
}

// The crop / work frame resampled to the box (bicubic, align_corners=False: rs_taps) at box pixel (dx, dy), `nc` channels.  Paste Back
// uses the value as it is (bicubic overshoot reaches the colour statistic), the Face Fix nodes clamp it (VRG_COMPOSITE_CLAMP_CROP).
// load(y, x, c) reads the [crop_h][crop_w][.] frame.
template <typename LOAD>
VRG_HD void cp_crop(const vrg_composite_desc& d, int32_t crop_h, int32_t crop_w, int nc, int32_t dx, int32_t dy, LOAD load, float o[4]) {
    int32_t ix[4], iy[4];
    float wx[4], wy[4];
    rs_taps(dx, rs_scale(crop_w, d.box_w), crop_w, ix, wx);
    rs_taps(dy, rs_scale(crop_h, d.box_h), crop_h, iy, wy);
    const bool clamp = (d.flags & VRG_COMPOSITE_CLAMP_CROP) != 0;
    for (int c = 0; c < nc; ++c) {
        float rows[4];
        for (int j = 0; j < 4; ++j) {
            float v[4];
            for (int i = 0; i < 4; ++i) v[i] = load(iy[j], ix[i], c);
            rows[j] = rs_dot<4>(wx, v);
        }
        const float r = rs_dot<4>(wy, rows);
        o[c] = clamp ? clamp01(r) : r;
    }
}

VRG_HD bool cp_selected(const vrg_composite_desc& d, float alpha) { return alpha > d.threshold; }

// (dst_mean - src_mean) * strength, both means fp32
VRG_HD float cp_shift(float src_mean, float dst_mean, float strength) { return (dst_mean - src_mean) * strength; }

// The per-frame record from the fp64 sums over the selected pixels: count, matched, source means, target means, shifts.
// matched = at least 16 selected pixels (the strength > 0 test is the caller's: such frames are not measured at all).
VRG_HD void cp_finalize(const vrg_composite_desc& d, const double sums[CP_PART_DOUBLES], int nc, uint32_t rec[CP_STATS_WORDS]) {
    const int64_t count = (int64_t)sums[0];
    const bool matched = count >= 16;
    for (int i = 0; i < CP_STATS_WORDS; ++i) rec[i] = 0u;
    rec[0] = (uint32_t)count;
    rec[1] = matched ? 1u : 0u;
    if (count <= 0) return;
    for (int c = 0; c < nc; ++c) {
        const float sm = (float)(sums[1 + c] / (double)count), dm = (float)(sums[5 + c] / (double)count);
        rec[2 + c] = f32_bits(sm);
        rec[6 + c] = f32_bits(dm);
        rec[10 + c] = matched ? f32_bits(cp_shift(sm, dm, d.match_strength)) : 0u;
    }
}

// One blended value: clamp(fl(fl(target * fl(1 - alpha)) + fl(crop * alpha)), 0, 1); with a match the crop is clamp(crop + shift, 0, 1) first
VRG_HD float cp_blend(float target, float crop, float alpha, bool matched, float shift) {
    const float c = matched ? clamp01(crop + shift) : crop;
    return clamp01(target * (1.0f - alpha) + c * alpha);
}

}  // namespace vrg
