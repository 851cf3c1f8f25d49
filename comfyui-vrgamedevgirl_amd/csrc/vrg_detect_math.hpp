// vrg_detect_math.hpp -- arithmetic of the face detector's input (csrc/vrg_detect.hip), host and device.
//
// What is restated: the per-frame pixel work of `_detect_with_rotation` / `_detect` (VRGDG_StandaloneFaceFixNodes.py:95-185 and
// VRGDG_FaceFix.py:67-157 of the reference) in front of the network, as OpenCV 4.x's classic fixed-point paths evaluate it, in integers and
// IEEE double / float only:
//   bytes      wp_quantise of vrg_warp_math.hpp: rint(fl(x * 255)), half to even, clipped to 0 .. 255, NaN gives 0 (:291); blob channel c
//              reads source channel 2 - c of an fp32 R,G,B frame (:292, COLOR_RGB2BGR), channel c of a decoded B,G,R byte frame
//   rotation   warpAffine(bgr, getRotationMatrix2D((W / 2.0, H / 2.0), angle, 1.0), (W, H), INTER_LINEAR, BORDER_REPLICATE).  The host
//              makes the matrix and inverts it in double (dt_rotation, dt_invert: cv2's order of operations) and hands the kernels the
//              six INVERSE doubles.  Per pixel (AB_SCALE = 1024, every rounding half to even and saturated to int32):
//                adelta = rint(m0 * x * 1024), bdelta = rint(m3 * x * 1024)
//                X0 = rint((m1 * y + m2) * 1024) + 16, Y0 = rint((m4 * y + m5) * 1024) + 16
//                X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5; position (X >> 5, Y >> 5), each saturated to int16; phases fx = X & 31,
//                fy = Y & 31
//                weights (32 - fx)(32 - fy) * 32, fx (32 - fy) * 32, (32 - fx) fy * 32, fx fy * 32 (they sum to 32768) on the taps (sx, sy),
//                (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1), each column clamped to [0, W - 1] and each row to [0, H - 1] on its own;
//                byte = (sum + 16384) >> 15.  cv2's int16 table cannot hold 32768 at phase (0, 0) and moves one unit elsewhere; either
//                split returns the top-left byte (tests/test_warp_host.py::test_phase_table), so the products are evaluated directly.
//              OpenCV >= 4.11 also ships a float-based linear warpAffine, and IPP / OpenCL builds may differ: the fixed-point path is pinned.
//   resize     cv2.resize(region, (300, 300)) (INTER_LINEAR, 8U).  Per axis scale = 1.0 / (300.0 / n_in) in double (not n_in / 300.0),
//              f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s.  Horizontally s < 0 gives f = 0, s = 0 and s >= n_in - 1 gives
//              f = 0, s = n_in - 1; vertically f stays and the two rows are clamped to [0, n_in - 1].  Coefficients rint((1.f - f) * 2048)
//              and rint(f * 2048) (float products, half to even, int16).  Horizontal pass S[s] * c0 + S[s + 1] * c1 in int32, vertical pass
//              (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.  When both scales are exactly 2 (a 600 x 600 region) cv2
//              switches to its area rule, (p00 + p01 + p10 + p11 + 2) >> 2.
//   blob       blobFromImage(., 1.0, (300, 300), (104, 177, 123), swapRB=False, crop=False): fp32 [3][300][300], (float)byte - mean[c],
//              exact in fp32.
// No cv2 is at hand where this was written: the restatement is pinned by an independent numpy restatement (tests/detect_support.py), by
// properties that rest on nobody's memory of cv2 (identity, integer translations against np.pad(mode="edge"), 300 x 300 and 600 x 600
// regions, constants), by float64 yardsticks and -- wherever cv2 can be imported or tests/golden/detect_cv2.npz exists -- by cv2 itself.
#pragma once
#include <stdint.h>

#include "vrg_warp_math.hpp"

namespace vrg {

constexpr int DT_BLOB = 300;                        // the network's input is 300 x 300
constexpr int DT_BLOB_PIXELS = DT_BLOB * DT_BLOB;
constexpr int DT_MIN_SIDE = 8;                      // the Builder skips smaller regions (VRGDG_FaceFix.py:74)
constexpr int DT_MAX_SIDE = 32767;                  // positions are int16
constexpr int DT_COEF_ONE = 2048;                   // INTER_RESIZE_COEF_SCALE

VRG_HD float dt_mean(int c) { return c == 0 ? 104.0f : (c == 1 ? 177.0f : 123.0f); }

// cvRound of a double, saturated to int32 (NaN gives INT32_MIN)
VRG_HD int32_t dt_round(double v) {
    const double r = __builtin_rint(v);
    if (!(r > -2147483648.0)) return (int32_t)(-2147483647 - 1);
    if (!(r < 2147483647.0)) return 2147483647;
    return (int32_t)r;
}

VRG_HD int32_t dt_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
VRG_HD int32_t dt_clamp(int32_t v, int32_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// source position and phases of destination pixel (x, y): m = the inverted matrix
VRG_HD void dt_source(const double m[6], int32_t x, int32_t y, int32_t& sx, int32_t& sy, int32_t& fx, int32_t& fy) {
    const double ab_scale = (double)(1 << WP_AB_BITS);
    const int32_t adelta = dt_round(m[0] * (double)x * ab_scale), bdelta = dt_round(m[3] * (double)x * ab_scale);
    const int32_t X0 = dt_add(dt_round((m[1] * (double)y + m[2]) * ab_scale), WP_ROUND_DELTA);
    const int32_t Y0 = dt_add(dt_round((m[4] * (double)y + m[5]) * ab_scale), WP_ROUND_DELTA);
    const int32_t X = dt_add(X0, adelta) >> (WP_AB_BITS - WP_INTER_BITS), Y = dt_add(Y0, bdelta) >> (WP_AB_BITS - WP_INTER_BITS);
    sx = wp_sat16(X >> WP_INTER_BITS);
    sy = wp_sat16(Y >> WP_INTER_BITS);
    fx = X & (WP_TAB - 1);
    fy = Y & (WP_TAB - 1);
}

// One pixel of the rotated W x H frame: pixel(y, x, b) gives the three B,G,R bytes of the source frame.
template <typename PIXEL>
VRG_HD void dt_warp_pixel(const double m[6], int32_t x, int32_t y, int32_t W, int32_t H, PIXEL pixel, uint8_t o[3]) {
    int32_t sx, sy, fx, fy;
    dt_source(m, x, y, sx, sy, fx, fy);
    const int32_t x0 = dt_clamp(sx, W - 1), x1 = dt_clamp(sx + 1, W - 1), y0 = dt_clamp(sy, H - 1), y1 = dt_clamp(sy + 1, H - 1);
    const int32_t w00 = (WP_TAB - fx) * (WP_TAB - fy) * 32, w01 = fx * (WP_TAB - fy) * 32, w10 = (WP_TAB - fx) * fy * 32, w11 = fx * fy * 32;
    uint8_t p00[3], p01[3], p10[3], p11[3];
    pixel(y0, x0, p00);
    pixel(y0, x1, p01);
    pixel(y1, x0, p10);
    pixel(y1, x1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[c] = (uint8_t)((w00 * (int32_t)p00[c] + w01 * (int32_t)p01[c] + w10 * (int32_t)p10[c] + w11 * (int32_t)p11[c] + (1 << (WP_COEF_BITS - 1))) >> WP_COEF_BITS);
}

// The two taps of output index d of one axis of the resize: samples s0, s1 (inside the axis) and their int16 coefficients.
struct DtTap {
    int32_t s0, s1, c0, c1;
};

VRG_HD double dt_scale(int32_t n_in, int32_t n_out) { return 1.0 / ((double)n_out / (double)n_in); }

// s as cv2 leaves it (horizontally 0 .. n_in - 1, vertically floor(f), which may lie one outside) and the coefficients
VRG_HD void dt_tap_raw(int32_t d, int32_t n_in, double scale, bool horizontal, int32_t& s, int32_t& c0, int32_t& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int32_t)__builtin_floorf(f);
    f -= (float)s;
    if (horizontal) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= n_in - 1) { f = 0.0f; s = n_in - 1; }
    }
    c0 = (int32_t)__builtin_rintf((1.0f - f) * (float)DT_COEF_ONE);
    c1 = (int32_t)__builtin_rintf(f * (float)DT_COEF_ONE);
}

VRG_HD DtTap dt_tap(int32_t d, int32_t n_in, double scale, bool horizontal) {
    DtTap t;
    int32_t s;
    dt_tap_raw(d, n_in, scale, horizontal, s, t.c0, t.c1);
    t.s0 = dt_clamp(s, n_in - 1);
    t.s1 = dt_clamp(s + 1, n_in - 1);          // horizontally at s = n_in - 1 the second term is absent: c1 = 0 there
    return t;
}

VRG_HD uint8_t dt_byte(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// the two passes of the byte resize: the horizontal one of a row (int32), the vertical one of two such rows
VRG_HD int32_t dt_hpass(int32_t p0, int32_t p1, int32_t c0, int32_t c1) { return p0 * c0 + p1 * c1; }
VRG_HD uint8_t dt_vpass(int32_t r0, int32_t r1, int32_t b0, int32_t b1) { return dt_byte((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2); }

// One pixel (dx, dy) of the n_out x n_out resize of an rw x rh region: pixel(y, x, b) gives the three bytes of the region.
template <typename PIXEL>
VRG_HD void dt_resize_pixel(int32_t dx, int32_t dy, int32_t rw, int32_t rh, int32_t n_out, PIXEL pixel, uint8_t o[3]) {
    const double scale_x = dt_scale(rw, n_out), scale_y = dt_scale(rh, n_out);
    uint8_t p00[3], p01[3], p10[3], p11[3];
    if (scale_x == 2.0 && scale_y == 2.0) {
        pixel(2 * dy, 2 * dx, p00);
        pixel(2 * dy, 2 * dx + 1, p01);
        pixel(2 * dy + 1, 2 * dx, p10);
        pixel(2 * dy + 1, 2 * dx + 1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(((int32_t)p00[c] + (int32_t)p01[c] + (int32_t)p10[c] + (int32_t)p11[c] + 2) >> 2);
        return;
    }
    const DtTap tx = dt_tap(dx, rw, scale_x, true), ty = dt_tap(dy, rh, scale_y, false);
    pixel(ty.s0, tx.s0, p00);
    pixel(ty.s0, tx.s1, p01);
    pixel(ty.s1, tx.s0, p10);
    pixel(ty.s1, tx.s1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t r0 = dt_hpass(p00[c], p01[c], tx.c0, tx.c1), r1 = dt_hpass(p10[c], p11[c], tx.c0, tx.c1);
        o[c] = dt_vpass(r0, r1, ty.c0, ty.c1);
    }
}

// A descriptor the kernels may follow: the frame exists, the transform exists or is -1 (none), the region lies inside the frame and
// neither side is below DT_MIN_SIDE.
VRG_HD bool dt_desc_ok(const vrg_detect_desc& d, int64_t frames, int64_t transforms, int32_t H, int32_t W) {
    return d.frame >= 0 && (int64_t)d.frame < frames && d.transform >= -1 && (int64_t)d.transform < transforms && d.left >= 0 && d.top >= 0 &&
           d.right <= W && d.bottom <= H && d.right - d.left >= DT_MIN_SIDE && d.bottom - d.top >= DT_MIN_SIDE;
}

VRG_HD bool dt_frame_desc_ok(const vrg_detect_frame_desc& d, int64_t frames, int64_t transforms) {
    return d.frame >= 0 && (int64_t)d.frame < frames && d.transform >= -1 && (int64_t)d.transform < transforms;
}

// ------------------------------------------------------------------------------------------------ HOST: the tables and the matrices
// ofs: 2 * n_out int32, coef: 4 * n_out int16 -- the horizontal table (s, then the pairs c0, c1), then the vertical one (s as floor(f))
inline void dt_fill_taps(int32_t n_in, int32_t n_out, int32_t* ofs, int16_t* coef) {
    const double scale = dt_scale(n_in, n_out);
    for (int axis = 0; axis < 2; ++axis)
        for (int32_t d = 0; d < n_out; ++d) {
            int32_t s, c0, c1;
            dt_tap_raw(d, n_in, scale, axis == 0, s, c0, c1);
            ofs[axis * n_out + d] = s;
            coef[2 * (axis * n_out + d)] = (int16_t)c0;
            coef[2 * (axis * n_out + d) + 1] = (int16_t)c1;
        }
}

// getRotationMatrix2D((W / 2.0, H / 2.0), angle, 1.0); cos and sin come from the caller's libm
inline void dt_rotation(double cos_a, double sin_a, int32_t W, int32_t H, double M[6]) {
    const double cx = (double)W / 2.0, cy = (double)H / 2.0, a = cos_a, b = sin_a;
    M[0] = a; M[1] = b; M[2] = (1.0 - a) * cx - b * cy;
    M[3] = -b; M[4] = a; M[5] = b * cx + (1.0 - a) * cy;
}

// the inversion of warpAffine without WARP_INVERSE_MAP (and of invertAffineTransform), in double
inline void dt_invert(const double M[6], double m[6]) {
    for (int i = 0; i < 6; ++i) m[i] = M[i];
    double D = m[0] * m[4] - m[1] * m[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = m[4] * D, A22 = m[0] * D;
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
    const double b1 = -m[0] * m[2] - m[1] * m[5], b2 = -m[3] * m[2] - m[4] * m[5];
    m[2] = b1; m[5] = b2;
}

}  // namespace vrg
