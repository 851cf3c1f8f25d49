// vrg_resize_math.hpp -- resampling arithmetic of the frame resize / restore kernels (csrc/vrg_resize.hip), host and device.
//
// What is restated: torch's CPU kernels behind F.interpolate(mode = bicubic | bilinear (align_corners=False) | area | nearest) in
// their plain one-rounding-per-operation form -- what ATEN_CPU_CAPABILITY=default executes (ATen/native/UpSample.h:
// area_pixel_compute_scale / area_pixel_compute_source_index / guard_index_and_lambda / get_cubic_upsample_coefficients,
// ATen/native/cpu/UpSampleKernel.cpp: Interpolate<n>::eval, ATen/native/AdaptiveAveragePooling.cpp: start_index / end_index).
// torch's AVX2 / AVX-512 builds evaluate the source coordinate differently (a few ulp); the plain form is the reproducible one.
// Reference lines: VRGDG_VideoEnhanceNodes.py:54-106 (_resize_batch, _restore_batch), :394-419 (restore).
//
// Which of torch's kernels: the reference resamples a permuted NHWC view (channels-last memory), so bicubic and nearest run torch's
// generic separable kernel (value = sum_y wy * (sum_x wx * src), x sum innermost), bilinear its channels-last kernel
// (value = (wy0*wx0)*i00 + (wy0*wx1)*i01 + (wy1*wx0)*i10 + (wy1*wx1)*i11) while the resampled height + width is at most 128 and the
// generic kernel above that (torch's _use_vectorized_kernel_cond_2d; a torch limited to ONE thread always takes the former and is
// then 1-2 ulp(1.0) away on large frames), and area the channels-last adaptive average pooling.
// Each was checked bit for bit against torch 2.10 (tests/golden/resize.npz, tests/test_resize_host.py).
// Everything is fp32, one rounding per operation (-ffp-contract=off), sums left to right starting from the first product.  The kernels and the host check (tests/host_math/resize_check.cpp) call the SAME functions.
#pragma once
#include "vrg_pixel_math.hpp"

namespace vrg {

enum { RS_BICUBIC = 0, RS_BILINEAR = 1, RS_AREA = 2, RS_NEAREST = 3 };

// (float)in / (float)out: area_pixel_compute_scale without a user scale factor, align_corners = False
VRG_HD float rs_scale(int32_t in, int32_t out) { return (float)in / (float)out; }
// scale * (d + 0.5) - 0.5
VRG_HD float rs_source(float scale, int32_t d) { return scale * ((float)d + 0.5f) - 0.5f; }
VRG_HD int32_t rs_clampi(int32_t v, int32_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// guard_index_and_lambda: index = min(floor(real), in - 1), lambda = min(max(real - index, 0), 1)
VRG_HD void rs_index_lambda(float real, int32_t in, int32_t& index, float& lambda) {
    const int32_t fl = (int32_t)__builtin_floorf(real);
    index = fl < in - 1 ? fl : in - 1;
    const float t = real - (float)index;
    lambda = __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f);
}

// Keys' cubic convolution, A = -0.75, torch's Horner order
VRG_HD float rs_cubic1(float x) { return ((-0.75f + 2.0f) * x - (-0.75f + 3.0f)) * x * x + 1.0f; }
VRG_HD float rs_cubic2(float x) { return ((-0.75f * x - 5.0f * -0.75f) * x + 8.0f * -0.75f) * x - 4.0f * -0.75f; }

// bicubic: taps floor(real) - 1 .. + 2, each clamped to [0, in - 1]; `real` is NOT clamped at 0
VRG_HD void rs_taps(int32_t d, float scale, int32_t in, int32_t (&idx)[4], float (&w)[4]) {
    int32_t i;
    float t;
    rs_index_lambda(rs_source(scale, d), in, i, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = rs_clampi(i - 1 + j, in - 1);
    w[0] = rs_cubic2(t + 1.0f);
    w[1] = rs_cubic1(t);
    const float u = 1.0f - t;
    w[2] = rs_cubic1(u);
    w[3] = rs_cubic2(u + 1.0f);
}
// bilinear: real clamped below at 0; i1 = min(i0 + 1, in - 1); w1 = real - i0, w0 = 1 - w1.  (torch short-cuts in == out to
// i0 = i1 = d, w = (1, 0): the same value for every finite input, real being exactly d there.)
VRG_HD void rs_linear_taps(int32_t d, float scale, int32_t in, int32_t (&idx)[2], float (&w)[2]) {
    float real = rs_source(scale, d);
    real = real < 0.0f ? 0.0f : real;
    int32_t i;
    float t;
    rs_index_lambda(real, in, i, t);
    idx[0] = i;
    idx[1] = i < in - 1 ? i + 1 : i;
    w[1] = t;
    w[0] = 1.0f - t;
}

// nearest: min((int)floor(d * scale), in - 1)
VRG_HD int32_t rs_nearest(int32_t d, float scale, int32_t in) {
    const int32_t i = (int32_t)__builtin_floorf((float)d * scale);
    return i < in - 1 ? i : in - 1;
}
// area = adaptive_avg_pool2d: window [floor(d * in / out), ceil((d + 1) * in / out)) in integers; the value is the raster-order sum of
// the window divided by its height, then by its width (two divisions, as torch's channels-last kernel does: one division by the
// count differs in the last bit wherever neither side is a power of two).  A 1 x 1 TARGET is torch's mean() reduction instead
// (pairwise, vectorised): not restated, such a call is a few ulp away.
VRG_HD void rs_area_window(int32_t d, int32_t in, int32_t out, int32_t& lo, int32_t& hi) {
    lo = (int32_t)(((int64_t)d * in) / out);
    hi = (int32_t)((((int64_t)d + 1) * in + out - 1) / out);
}

// sum_j w[j] * v[j], left to right from the first product
template <int N>
VRG_HD float rs_dot(const float (&w)[N], const float (&v)[N]) {
    float acc = v[0] * w[0];
#pragma unroll
    for (int j = 1; j < N; ++j) acc = acc + v[j] * w[j];
    return acc;
}

// One bilinear value from its four taps.  torch picks its channels-last kernel (four products of weight pairs: `paired`) or its generic
// separable kernel (rows first, as bicubic); which one runs is the caller's to say (rs_pixel, csrc/vrg_flf_math.hpp).  Not clamped.
VRG_HD float rs_bilinear_value(bool paired, const float (&wx)[2], const float (&wy)[2], float i00, float i01, float i10, float i11) {
    return paired ? (wy[0] * wx[0]) * i00 + (wy[0] * wx[1]) * i01 + (wy[1] * wx[0]) * i10 + (wy[1] * wx[1]) * i11
                  : (i00 * wx[0] + i01 * wx[1]) * wy[0] + (i10 * wx[0] + i11 * wx[1]) * wy[1];
}

// Which of the two torch runs (ATen/native/cpu/UpSampleKernel.cpp: _use_vectorized_kernel_cond_2d, torch with at least two threads): the
// channels-last kernel when the resampled view is channels-last contiguous and has more than 3 channels, or when the output height +
// width is at most 128; the generic kernel otherwise.
VRG_HD bool rs_bilinear_paired(bool contiguous, int32_t channels, int32_t out_h, int32_t out_w) {
    return (contiguous && channels > 3) || out_h + out_w <= 128;
}
// Is the rectangle sw x sh narrowed out of `frames` channels-last pictures [h][w][c] still channels-last contiguous?  Dimensions of
// size 1 do not count: rows narrowed only in y stay contiguous within a picture, several pictures only when nothing is narrowed.
VRG_HD bool rs_view_contiguous(int64_t frames, int32_t h, int32_t w, int32_t sw, int32_t sh) {
    return (sh == 1 || sw == w) && (frames == 1 || (int64_t)sh * sw == (int64_t)h * w);
}

// The blend of VRGDGVideoEnhanceRestoreOriginal.restore on one value: clamp(o * (1 - s) + clamp01(resampled) * s, 0, 1)
VRG_HD float rs_blend(float original, float restored, float s, float oms) { return clamp01(original * oms + restored * s); }

// Geometry of one call: the source rectangle of the input frames, the rectangle of the output frames it is resampled into (which may
// hang over the output frame: crop to fill), everything else of the output is zero.
struct ResizeGeom {
    int32_t in_h, in_w, in_c;
    int32_t sx0, sy0, sw, sh;
    int32_t out_h, out_w;
    int32_t dx0, dy0, dw, dh;
};

// The argument rules of a geometry, shared by every entry point that takes one (vrg_resize_f32, vrg_restore_f32, vrg_prepare_frames_f32)
inline bool rs_geom_ok(const ResizeGeom& g) {
    if (g.in_h <= 0 || g.in_w <= 0 || g.in_c < 3 || g.out_h <= 0 || g.out_w <= 0) return false;
    if (g.sx0 < 0 || g.sy0 < 0 || g.sw <= 0 || g.sh <= 0 || (int64_t)g.sx0 + g.sw > g.in_w || (int64_t)g.sy0 + g.sh > g.in_h) return false;
    // the destination rectangle may hang over the output frame (crop to fill) but must meet it
    if (g.dw <= 0 || g.dh <= 0 || g.dx0 >= g.out_w || g.dy0 >= g.out_h || (int64_t)g.dx0 + g.dw <= 0 || (int64_t)g.dy0 + g.dh <= 0) return false;
    return true;
}
// in-frame offsets of the source are 32-bit; frames are addressed with 64 bits
inline bool rs_sizes_ok(const ResizeGeom& g) {
    return (int64_t)g.in_w * g.in_c <= 0x7fffffff && (int64_t)g.out_h * g.out_w <= 0x7fffffff / 4;
}

// One RGB output pixel (ox, oy) of one frame, straight from the definitions above (no reuse between pixels): the form the host check
// runs, and the nearest / area kernels.  `frame`: the [in_h][in_w][in_c] input frame.  Result clamped to [0, 1].
template <typename LOAD>
VRG_HD void rs_pixel(const ResizeGeom& g, int32_t method, int32_t ox, int32_t oy, LOAD load, float o[3]) {
    const int32_t dx = ox - g.dx0, dy = oy - g.dy0;
    o[0] = o[1] = o[2] = 0.0f;
    if (dx < 0 || dx >= g.dw || dy < 0 || dy >= g.dh) return;
    const float sx = rs_scale(g.sw, g.dw), sy = rs_scale(g.sh, g.dh);
    if (method == RS_NEAREST) {
        const int32_t x = g.sx0 + rs_nearest(dx, sx, g.sw), y = g.sy0 + rs_nearest(dy, sy, g.sh);
        for (int c = 0; c < 3; ++c) o[c] = clamp01(load(y, x, c));
    } else if (method == RS_AREA) {
        int32_t x0, x1, y0, y1;
        rs_area_window(dx, g.sw, g.dw, x0, x1);
        rs_area_window(dy, g.sh, g.dh, y0, y1);
        const float kh = (float)(y1 - y0), kw = (float)(x1 - x0);
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int32_t y = y0; y < y1; ++y)
            for (int32_t x = x0; x < x1; ++x)
                for (int c = 0; c < 3; ++c) sum[c] = sum[c] + load(g.sy0 + y, g.sx0 + x, c);
        for (int c = 0; c < 3; ++c) o[c] = clamp01(sum[c] / kh / kw);
    } else if (method == RS_BICUBIC) {
        int32_t ix[4], iy[4];
        float wx[4], wy[4];
        rs_taps(dx, sx, g.sw, ix, wx);
        rs_taps(dy, sy, g.sh, iy, wy);
        for (int c = 0; c < 3; ++c) {
            float rows[4];
            for (int j = 0; j < 4; ++j) {
                float v[4];
                for (int i = 0; i < 4; ++i) v[i] = load(g.sy0 + iy[j], g.sx0 + ix[i], c);
                rows[j] = rs_dot<4>(wx, v);
            }
            o[c] = clamp01(rs_dot<4>(wy, rows));
        }
    } else {
        int32_t ix[2], iy[2];
        float wx[2], wy[2];
        rs_linear_taps(dx, sx, g.sw, ix, wx);
        rs_linear_taps(dy, sy, g.sh, iy, wy);
        const bool small = g.dh + g.dw <= 128;
        for (int c = 0; c < 3; ++c) {
            const float i00 = load(g.sy0 + iy[0], g.sx0 + ix[0], c), i01 = load(g.sy0 + iy[0], g.sx0 + ix[1], c);
            const float i10 = load(g.sy0 + iy[1], g.sx0 + ix[0], c), i11 = load(g.sy0 + iy[1], g.sx0 + ix[1], c);
            // torch picks its channels-last kernel (four products of weight pairs) for RGB frames whose resampled height + width is at
            // most 128 and its generic separable kernel (rows first, as bicubic) for everything larger
            o[c] = clamp01(rs_bilinear_value(small, wx, wy, i00, i01, i10, i11));
        }
    }
}

// A box crop (csrc/vrg_crop.hip: the Face Fix work frames) is rs_pixel on a view: the box [box_h][box_w] is the whole input frame AND the
// source rectangle -- so the taps are clamped to the box, not to the frame it was cut from, as F.interpolate sees the sliced view -- and
// the size_h x size_w output frame is the whole destination.  `load(y, x, c)` then takes box coordinates.
VRG_HD ResizeGeom rs_box_geom(int32_t box_w, int32_t box_h, int32_t channels, int32_t size_w, int32_t size_h) {
    return ResizeGeom{box_h, box_w, channels, 0, 0, box_w, box_h, size_h, size_w, 0, 0, size_w, size_h};
}

}  // namespace vrg
