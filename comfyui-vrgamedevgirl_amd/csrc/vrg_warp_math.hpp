// vrg_warp_math.hpp -- arithmetic of the landmark-aligned Face Fix composite's warp (csrc/vrg_composite.hip), host and device.
//
// What is restated: the uint8 path of OpenCV 4.x's warpAffine(src, M, (w, h), INTER_LANCZOS4, BORDER_REFLECT101) as
// VRGDGFaceFixCompositeLandmarkAligned calls it (VRGDG_StandaloneFaceFixNodes.py:1046): the affine remap in fixed point.
//   the 2 x 3 matrix goes to double and is inverted in double (wp_invert: D = M0*M4 - M1*M3, D = D ? 1/D : 0, ...)
//   per column x: adelta = cvRound(M0 * x * 1024), bdelta = cvRound(M3 * x * 1024)            (cvRound: half to even)
//   per row y:    X0 = cvRound((M1 * y + M2) * 1024) + 16, Y0 = cvRound((M4 * y + M5) * 1024) + 16
//   per pixel:    X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5; position (X >> 5, Y >> 5), each saturated to int16; phase
//                 (Y & 31) * 32 + (X & 31)
//   the pixel:    64 taps at (sx - 3 + k2, sy - 3 + k1), each coordinate folded by BORDER_REFLECT101; int32 sum of byte * weight;
//                 output clamp((sum + (1 << 14)) >> 15, 0, 255)
//   the weights:  1024 phases x 8 x 8 int16: saturate_cast<short>(wy[k1] * wx[k2] * 32768) of the 1-D float weights of phase k / 32
//                 (lz_weights of vrg_lanczos_math.hpp), then the fix-up that makes every phase sum to exactly 32768 (wp_phase_table)
// No cv2 is at hand where this was written: the restatement is pinned by an independent numpy restatement (tests/warp_support.py), by
// properties that do not rest on anyone's memory of cv2 (identity, integer translations against np.pad(mode="reflect")), by a float64
// yardstick and -- wherever cv2 can be imported -- by tests/golden/warp_lanczos4_cv2.npz.
//
// The record of one warped frame carries the six doubles of the INVERTED matrix; the four roundings per pixel are made where the pixel is
// (v_mul_f64, v_rndne_f64: IEEE double, the same integers on the host and on the device).  Whether every rounding and every sum stays
// inside int32 is decided once per frame on the host (wp_record): a record that is `set` never overflows in the kernel.
// The table and the records are made on the HOST (plain inline functions, never called from a kernel); the coordinate walk, the fold
// and the 64-tap sum are shared by the kernels and the host check (tests/host_math/warp_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/vrgdg_hip.h"
#include "vrg_lanczos_math.hpp"

namespace vrg {

constexpr int WP_AB_BITS = 10;                    // AB_BITS = max(10, INTER_BITS)
constexpr int WP_INTER_BITS = 5;                  // INTER_BITS
constexpr int WP_TAB = 1 << WP_INTER_BITS;        // 32 phases per axis
constexpr int WP_PHASES = WP_TAB * WP_TAB;
constexpr int WP_KERNEL = LZ_TAPS * LZ_TAPS;      // 64 int16 per phase
constexpr int WP_COEF_BITS = 15;                  // INTER_REMAP_COEF_BITS
constexpr int WP_ROUND_DELTA = (1 << WP_AB_BITS) / WP_TAB / 2;
constexpr int64_t WP_TABLE_BYTES = (int64_t)WP_PHASES * WP_KERNEL * 2;

// cvRound of a double that is known to fit int32
VRG_HD int32_t wp_round(double v) { return (int32_t)__builtin_rint(v); }

VRG_HD int32_t wp_sat16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// borderInterpolate(p, len, BORDER_REFLECT_101): the reflections p < 0 ? -p : 2 * (len - 1) - p repeated until p is in range, in closed
// form (the walk has period 2 * (len - 1); the restatement of the tests iterates)
VRG_HD int32_t wp_reflect101(int32_t p, int32_t len) {
    if ((uint32_t)p < (uint32_t)len) return p;
    if (len == 1) return 0;
    const int32_t period = 2 * (len - 1);
    int32_t q = p % period;
    if (q < 0) q += period;
    return q < len ? q : period - q;
}

// source position and phase of destination pixel (x, y): m = the inverted matrix
VRG_HD void wp_source(const double m[6], int32_t x, int32_t y, int32_t& sx, int32_t& sy, int32_t& phase) {
    const double ab_scale = (double)(1 << WP_AB_BITS);
    const int32_t adelta = wp_round(m[0] * (double)x * ab_scale), bdelta = wp_round(m[3] * (double)x * ab_scale);
    const int32_t X0 = wp_round((m[1] * (double)y + m[2]) * ab_scale) + WP_ROUND_DELTA;
    const int32_t Y0 = wp_round((m[4] * (double)y + m[5]) * ab_scale) + WP_ROUND_DELTA;
    const int32_t X = (X0 + adelta) >> (WP_AB_BITS - WP_INTER_BITS), Y = (Y0 + bdelta) >> (WP_AB_BITS - WP_INTER_BITS);
    sx = wp_sat16(X >> WP_INTER_BITS);
    sy = wp_sat16(Y >> WP_INTER_BITS);
    phase = (Y & (WP_TAB - 1)) * WP_TAB + (X & (WP_TAB - 1));
}

// FixedPtCast<int, uchar, 15>
VRG_HD uint8_t wp_cast(int32_t v) {
    const int32_t r = (v + (1 << (WP_COEF_BITS - 1))) >> WP_COEF_BITS;
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// One warped pixel of a [src_h][src_w][3] byte image: kernel = the 64 weights of the pixel's phase (16-byte aligned), load(y, x, c) reads
// the image.
template <typename LOAD>
VRG_HD void wp_pixel(const int16_t* kernel, int32_t sx, int32_t sy, int32_t src_w, int32_t src_h, LOAD load, uint8_t o[3]) {
    int32_t xs[LZ_TAPS];
#pragma unroll
    for (int k = 0; k < LZ_TAPS; ++k) xs[k] = wp_reflect101(sx - 3 + k, src_w);
    int32_t acc[3] = {0, 0, 0};
    const int16_t* rows = (const int16_t*)__builtin_assume_aligned(kernel, 16);      // a phase starts on 128 bytes of a 16-byte-aligned table
#pragma unroll 1
    for (int j = 0; j < LZ_TAPS; ++j) {
        const int32_t y = wp_reflect101(sy - 3 + j, src_h);
        int16_t wr[LZ_TAPS];                                                           // this row's eight weights: one 16-byte load
#pragma unroll
        for (int k = 0; k < LZ_TAPS; ++k) wr[k] = rows[j * LZ_TAPS + k];
#pragma unroll
        for (int k = 0; k < LZ_TAPS; ++k) {
            const int32_t w = (int32_t)wr[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (int32_t)load(y, xs[k], c) * w;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = wp_cast(acc[c]);
}

// uint8(clip(rint(v * 255), 0, 255)) as numpy does it in fp32 (round half to even); NaN gives 0
VRG_HD uint8_t wp_quantise(float v) {
    const float r = __builtin_rintf(v * 255.0f);
    return (uint8_t)(r >= 255.0f ? 255.0f : (r > 0.0f ? r : 0.0f));
}

// ------------------------------------------------------------------------------------------------ HOST: the table and the records
// initInterTab2D(INTER_LANCZOS4, fixpt): table[phase][k1][k2], phase = fy * 32 + fx
inline void wp_phase_table(int16_t* table) {
    float w1[WP_TAB][LZ_TAPS];
    for (int k = 0; k < WP_TAB; ++k) lz_weights((float)k * (1.0f / (float)WP_TAB), w1[k]);
    for (int fy = 0; fy < WP_TAB; ++fy) {
        for (int fx = 0; fx < WP_TAB; ++fx) {
            int16_t* t = table + (fy * WP_TAB + fx) * WP_KERNEL;
            int32_t sum = 0;
            for (int k1 = 0; k1 < LZ_TAPS; ++k1) {
                for (int k2 = 0; k2 < LZ_TAPS; ++k2) {
                    const float v = rintf(w1[fy][k1] * w1[fx][k2] * (float)(1 << WP_COEF_BITS));
                    t[k1 * LZ_TAPS + k2] = (int16_t)(v < -32768.0f ? -32768.0f : (v > 32767.0f ? 32767.0f : v));
                    sum += t[k1 * LZ_TAPS + k2];
                }
            }
            if (sum != (1 << WP_COEF_BITS)) {
                const int32_t diff = sum - (1 << WP_COEF_BITS), half = LZ_TAPS / 2;
                int lo = half * LZ_TAPS + half, hi = lo;
                for (int k1 = half; k1 < half + 2; ++k1) {
                    for (int k2 = half; k2 < half + 2; ++k2) {
                        const int i = k1 * LZ_TAPS + k2;
                        if (t[i] < t[lo]) lo = i;
                        else if (t[i] > t[hi]) hi = i;
                    }
                }
                if (diff < 0) t[hi] = (int16_t)(t[hi] - diff);
                else t[lo] = (int16_t)(t[lo] - diff);
            }
        }
    }
}

// the inversion of warpAffine without WARP_INVERSE_MAP, in double
inline void wp_invert(const float t[6], double m[6]) {
    for (int i = 0; i < 6; ++i) m[i] = (double)t[i];
    double D = m[0] * m[4] - m[1] * m[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = m[4] * D, A22 = m[0] * D;
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
    const double b1 = -m[0] * m[2] - m[1] * m[5], b2 = -m[3] * m[2] - m[4] * m[5];
    m[2] = b1; m[5] = b2;
}

// The record of one frame warped to out_w x out_h from a [src_h][src_w][3] image at `src_offset` bytes.  false (record cleared) when the
// transform has a non-finite entry or a scaled term or a sum of two leaves int32 for some pixel: each term is monotonic in its
// coordinate, so the first and last column and row decide.
inline bool wp_record(const float t[6], int32_t out_w, int32_t out_h, int32_t src_w, int32_t src_h, int64_t src_offset, vrg_warp_desc* rec) {
    *rec = vrg_warp_desc{};
    for (int i = 0; i < 6; ++i)
        if (!(fabs((double)t[i]) <= (double)FLT_MAX)) return false;
    if (out_w < 1 || out_h < 1 || src_w < 1 || src_h < 1 || src_offset < 0) return false;
    double m[6];
    wp_invert(t, m);
    const double ab_scale = (double)(1 << WP_AB_BITS), lo = -2147483648.0, hi = 2147483647.0;
    for (int i = 0; i < 6; ++i)
        if (!(fabs(m[i]) <= DBL_MAX)) return false;
    for (int axis = 0; axis < 2; ++axis) {
        const double a = m[3 * axis], b = m[3 * axis + 1], c = m[3 * axis + 2];
        for (int ix = 0; ix < 2; ++ix) {
            const double col = rint(a * (double)(ix ? out_w - 1 : 0) * ab_scale);
            for (int iy = 0; iy < 2; ++iy) {
                const double row = rint((b * (double)(iy ? out_h - 1 : 0) + c) * ab_scale);
                if (!(col >= lo && col <= hi && row >= lo && row + WP_ROUND_DELTA <= hi)) return false;
                const double sum = row + WP_ROUND_DELTA + col;
                if (!(sum >= lo && sum <= hi)) return false;
            }
        }
    }
    for (int i = 0; i < 6; ++i) rec->m[i] = m[i];
    rec->src_offset = src_offset;
    rec->src_w = src_w;
    rec->src_h = src_h;
    rec->set = 1;
    return true;
}

}  // namespace vrg
