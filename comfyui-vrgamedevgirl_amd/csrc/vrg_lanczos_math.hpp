// vrg_lanczos_math.hpp -- arithmetic of the enhancer's upscale (csrc/vrg_lanczos.hip), host and device.
//
// What is restated: the uint8 path of OpenCV 4.x's resize(..., INTER_LANCZOS4) as the stand-alone enhancer calls it
// (VRGDG_StandaloneVideoEnhancerNodes.py:213-230): an 8 x 8-tap separable filter in fixed point.  Per output index d of an axis with
// n_in source and n_out output samples:
//   scale = n_in / n_out                                 (double)
//   fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), t = fx - s            (fp32)
//   taps s - 3 .. s + 4, each clamped to [0, n_in - 1]
//   t < FLT_EPSILON: w = (0, 0, 0, 1, 0, 0, 0, 0); otherwise w_i = (float)((cs[i][0] * sin(y0) + cs[i][1] * cos(y0)) / (y_i * y_i)) with
//   y_i = -(t + 3 - i) * pi / 4 (t + 3 - i in fp32 as the C expression evaluates it, the product in double), y0 = y_0, cs = (cos, sin)
//   of the multiples of 45 degrees; the eight are summed in fp32 in tap order and each multiplied by 1.f / sum
//   integer weights short(rint(w_i * 2048)); their sum is NOT fixed up
//   horizontal pass: int32 sum of byte * weight; vertical pass: int32 sum of horizontal result * weight
//   output = clamp((v + (1 << 21)) >> 22, 0, 255)
// No cv2 is at hand where this was written: the restatement is pinned by an independent numpy restatement (tests/lanczos_support.py),
// by the float64 Lanczos filter (at most one level away) and -- wherever cv2 can be imported -- by tests/golden/lanczos4_cv2.npz.
//
// The weights (the only transcendental work) are made on the HOST, once per geometry: lz_tap below is host-only, the kernels read the
// table of LzTap records (offset + eight int16) it fills.  The integer passes are shared by the kernels and the host check
// (tests/host_math/lanczos_check.cpp).  Integer sums wrap like int32 hardware arithmetic does (the horizontal sums stay below 2^20 in
// magnitude; a vertical sum can only leave int32 on inputs built for it).
#pragma once
#include <stdint.h>

#include "vrg_pixel_math.hpp"

#include <float.h>
#include <math.h>

namespace vrg {

constexpr int LZ_TAPS = 8;
constexpr int LZ_COEF_BITS = 11;                  // INTER_RESIZE_COEF_BITS

// One output column or row: s = floor(fx) (NOT clamped: the taps are s - 3 + k, each clamped on use) and the eight integer weights.
struct LzTap {
    int32_t s;
    int16_t w[LZ_TAPS];
};
static_assert(sizeof(LzTap) == 20, "LzTap is 20 bytes: the table layout of vrg_lanczos4_taps");

VRG_HD int32_t lz_clampi(int32_t v, int32_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
VRG_HD int32_t lz_mac(int32_t acc, int32_t a, int32_t b) { return (int32_t)((uint32_t)acc + (uint32_t)a * (uint32_t)b); }
// FixedPtCast<int, uchar, 22>
VRG_HD uint8_t lz_cast(int32_t v) {
    const int32_t r = (int32_t)((uint32_t)v + (1u << (2 * LZ_COEF_BITS - 1))) >> (2 * LZ_COEF_BITS);
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// The table, HOST functions (plain inline: never called from a kernel).  lz_source alone is what the entry points need to size a tile's
// source rows.
inline void lz_source(int32_t d, int32_t n_in, int32_t n_out, int32_t& s, float& t) {
    const double scale = (double)n_in / (double)n_out;
    const float fx = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int32_t)floorf(fx);
    t = fx - (float)s;
}

inline void lz_weights(float t, float (&w)[LZ_TAPS]) {
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[LZ_TAPS][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    static const double quarter_pi = 3.1415926535897932384626433832795 * 0.25;
    if (t < FLT_EPSILON) {
        for (int i = 0; i < LZ_TAPS; ++i) w[i] = 0.0f;
        w[3] = 1.0f;
        return;
    }
    const double y0 = -(double)(t + 3.0f) * quarter_pi, s0 = sin(y0), c0 = cos(y0);
    float sum = 0.0f;
    for (int i = 0; i < LZ_TAPS; ++i) {
        const float a = t + 3.0f - (float)i;
        const double y = -(double)a * quarter_pi;
        w[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        sum = sum + w[i];
    }
    const float inv = 1.0f / sum;
    for (int i = 0; i < LZ_TAPS; ++i) w[i] = w[i] * inv;
}

inline LzTap lz_tap(int32_t d, int32_t n_in, int32_t n_out) {
    LzTap e;
    float t, w[LZ_TAPS];
    lz_source(d, n_in, n_out, e.s, t);
    lz_weights(t, w);
    for (int i = 0; i < LZ_TAPS; ++i) {
        const float v = rintf(w[i] * (float)(1 << LZ_COEF_BITS));          // saturate_cast<short>(float): round half to even, then saturate
        e.w[i] = (int16_t)(v < -32768.0f ? -32768.0f : (v > 32767.0f ? 32767.0f : v));
    }
    return e;
}

// columns first, then rows: out_w + out_h records
inline void lz_fill_taps(int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h, LzTap* taps) {
    for (int32_t x = 0; x < out_w; ++x) taps[x] = lz_tap(x, in_w, out_w);
    for (int32_t y = 0; y < out_h; ++y) taps[out_w + y] = lz_tap(y, in_h, out_h);
}

// One source row's horizontal sum for one channel: load(x) = the byte of column x (already clamped by this function)
template <typename LOAD>
VRG_HD int32_t lz_hsum(const LzTap& cx, int32_t in_w, LOAD load) {
    int32_t acc = 0;
#pragma unroll
    for (int k = 0; k < LZ_TAPS; ++k) acc = lz_mac(acc, (int32_t)load(lz_clampi(cx.s - 3 + k, in_w - 1)), (int32_t)cx.w[k]);
    return acc;
}

// One output pixel straight from the definition (no reuse between pixels): the host check and the plain per-pixel kernel.
// load(y, x, c) = byte c of source pixel (y, x).
template <typename LOAD>
VRG_HD void lz_pixel(const LzTap& cx, const LzTap& ry, int32_t in_w, int32_t in_h, LOAD load, uint8_t o[3]) {
    int32_t v[3] = {0, 0, 0};
#pragma unroll 1
    for (int j = 0; j < LZ_TAPS; ++j) {
        const int32_t y = lz_clampi(ry.s - 3 + j, in_h - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int32_t h = lz_hsum(cx, in_w, [&](int32_t x) { return load(y, x, c); });
            v[c] = lz_mac(v[c], h, (int32_t)ry.w[j]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = lz_cast(v[c]);
}

}  // namespace vrg
