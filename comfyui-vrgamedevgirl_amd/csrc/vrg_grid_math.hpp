// vrg_grid_math.hpp -- arithmetic of the Video Folder Grid Plot (csrc/vrg_grid.hip), host and device.
//
// What is restated: the per-frame pixel work of VRGDG_VideoFolderGridPlot (LTXLoraTrain.py:8062-8086 `_fit_frame_to_tile`, :8190-8236
// `_build_grid_frames_from_images` of the reference) as numpy and OpenCV 4.x's hal::resize evaluate it.  No cv2 is at hand where this was
// written: the restatement is pinned by an independent numpy restatement (tests/grid_support.py), by the float64 filters (at most one level
// away) and -- wherever cv2 can be imported or tests/golden/video_grid_cv2.npz exists -- by cv2 itself.
//
//   bytes      np.clip(x * 255.0, 0, 255).astype(np.uint8): one fp32 multiply, a clip, TRUNCATION toward zero (area_quant of the cut score
//              rounds; this does not).  NaN is undefined in numpy; here it gives 0.  Channels 0..2 of an fp32 R,G,B frame; a decoded
//              B,G,R byte frame is its own quantisation and output channel c reads its channel 2 - c.
//   resize     cv2.resize(img, (new_w, new_h), INTER_AREA) on 8UC3.  Per axis inv = (double)n_out / n_in, scale = 1.0 / inv (not
//              n_in / (double)n_out, which vrg_area_math.hpp forms for its 64-pixel case).
//                copy      both sides unchanged: the bytes
//                area      both scales >= 1.  Fast when both lie within DBL_EPSILON of integers sx, sy: the integer sum of the sx x sy
//                          cell, saturate(rint((float)sum * (1.0f / (sx * sy)))); sx == sy == 2 is (a + b + c + d + 2) >> 2.  Otherwise the
//                          tap rule and the fp32 order written at the top of vrg_area_math.hpp with n_out in place of 64.
//                linear    any axis enlarges: the fixed-point byte bilinear resize of vrg_detect_math.hpp (dt_hpass, dt_vpass) with the
//                          coefficients of area mode: s = floor(d * scale), f = (float)((d + 1) - (s + 1) * inv), f = f <= 0 ? 0 :
//                          f - floor(f); s < 0 gives s = 0, f = 0 and s >= n_in - 1 gives s = n_in - 1, f = 0; rint((1.f - f) * 2048) and
//                          rint(f * 2048).
//   grid       (float)byte / 255.0f, correctly rounded, everything outside picture and label 0.
// One table record serves every mode: an AreaCell (first sample, count, three weights).  For the linear rule count is 1 or 2 and w_first,
// w_last hold the two integer coefficients (0 .. 2048, exact as floats).
#pragma once
#include <stdint.h>

#include "vrg_area_math.hpp"
#include "vrg_detect_math.hpp"

#include <float.h>
#include <math.h>

namespace vrg {

enum GridMode { GRID_COPY = 0, GRID_FAST = 1, GRID_FAST_2X2 = 2, GRID_GENERAL = 3, GRID_LINEAR = 4 };

constexpr int GRID_ROW_VALUES = 4096;               // source values one wave stages at a time (csrc/vrg_grid.hip)
constexpr int GRID_LANES = 64;                      // tile columns of one workgroup

// np.clip(x * 255.0, 0, 255).astype(np.uint8)
VRG_HD uint8_t grid_quant(float x) {
    const float c = __builtin_fminf(__builtin_fmaxf(x * 255.0f, 0.0f), 255.0f);             // NaN -> 0
    return (uint8_t)(int32_t)c;
}
VRG_HD uint8_t grid_quant(uint8_t x) { return x; }

// np.float32(k) / np.float32(255.0)
VRG_HD float grid_unit(int32_t k) { return (float)k / 255.0f; }

inline double grid_inv(int32_t n_in, int32_t n_out) { return (double)n_out / (double)n_in; }
inline double grid_scale(int32_t n_in, int32_t n_out) { return 1.0 / grid_inv(n_in, n_out); }

// is the scale within DBL_EPSILON of an integer (cv2: saturate_cast<int>(scale), round half to even)
inline bool grid_integer_scale(double scale, int32_t& i) {
    i = (int32_t)rint(scale);
    return fabs(scale - (double)i) < DBL_EPSILON;
}

inline int grid_mode(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
    if (in_h == out_h && in_w == out_w) return GRID_COPY;
    const double sx = grid_scale(in_w, out_w), sy = grid_scale(in_h, out_h);
    if (!(sx >= 1.0 && sy >= 1.0)) return GRID_LINEAR;
    int32_t ix, iy;
    if (!grid_integer_scale(sx, ix) || !grid_integer_scale(sy, iy)) return GRID_GENERAL;
    return ix == 2 && iy == 2 ? GRID_FAST_2X2 : GRID_FAST;
}

// fast paths: 1.0f / (sx * sy)
inline float grid_fast_inv(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
    int32_t ix = 1, iy = 1;
    grid_integer_scale(grid_scale(in_w, out_w), ix);
    grid_integer_scale(grid_scale(in_h, out_h), iy);
    return 1.0f / (float)(ix * iy);
}

// the two taps of the bilinear rule in area mode: samples s, s + 1 (one sample where clamped), coefficients as floats
inline AreaCell grid_linear_cell(int32_t d, int32_t n_in, int32_t n_out) {
    const double inv = grid_inv(n_in, n_out), scale = 1.0 / inv;
    int32_t s = (int32_t)floor((double)d * scale);
    float f = (float)((double)(d + 1) - (double)(s + 1) * inv);
    f = f <= 0.0f ? 0.0f : f - floorf(f);
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.0f; }
    AreaCell c;
    c.first = s;
    c.count = s + 1 <= n_in - 1 ? 2 : 1;
    c.w_first = (float)(int32_t)rintf((1.0f - f) * (float)DT_COEF_ONE);
    c.w_mid = 0.0f;
    c.w_last = (float)(int32_t)rintf(f * (float)DT_COEF_ONE);
    return c;
}

// the table of one axis in one mode: n_out records
inline void grid_fill_taps(int32_t n_in, int32_t n_out, int32_t mode, AreaCell* cells) {
    const double scale = grid_scale(n_in, n_out);
    int32_t step = 1;
    if (mode == GRID_FAST || mode == GRID_FAST_2X2) grid_integer_scale(scale, step);
    for (int32_t d = 0; d < n_out; ++d) {
        if (mode == GRID_LINEAR) cells[d] = grid_linear_cell(d, n_in, n_out);
        else if (mode == GRID_GENERAL) cells[d] = area_cell_scaled(d, n_in, scale);
        else cells[d] = AreaCell{d * step, step, 1.0f, 1.0f, 1.0f};                      // copy (step 1) and the integer cells
    }
}

// the most tile columns (64, 32, .. 1) whose source samples of any run of that many consecutive records fit one staging buffer; 0: none
inline int32_t grid_cells_per_segment(const AreaCell* cells, int32_t n_out, int32_t channels) {
    for (int32_t cps = GRID_LANES; cps >= 1; cps >>= 1) {
        int64_t longest = 0;
        for (int32_t d = 0; d < n_out; ++d) {
            const int32_t dl = d + cps - 1 < n_out - 1 ? d + cps - 1 : n_out - 1;
            const int64_t n = (int64_t)(cells[dl].first + cells[dl].count - cells[d].first) * channels;
            longest = n > longest ? n : longest;
        }
        if (longest <= GRID_ROW_VALUES) return cps;
    }
    return 0;
}

// The three steps every mode shares, in words (fp32 bits for the general rule, int32 otherwise).
//   term: what one sample adds to the running value of one source row
VRG_HD float grid_term_general(float acc, uint8_t s, float w) { return area_add(acc, s, w); }
VRG_HD int32_t grid_term_fast(int32_t acc, uint8_t s) { return acc + (int32_t)s; }
//   linear: the row value from its one or two samples
VRG_HD int32_t grid_row_linear(uint8_t s0, uint8_t s1, const AreaCell& x) { return dt_hpass(s0, s1, (int32_t)x.w_first, (int32_t)x.w_last); }
//   last: the byte of the linear rule from the values of its one or two rows
VRG_HD uint8_t grid_byte_linear(int32_t r0, int32_t r1, const AreaCell& y) { return dt_vpass(r0, r1, (int32_t)y.w_first, (int32_t)y.w_last); }

// ---- HOST: straight from the definition (tests/host_math/grid_check.cpp; never called from a kernel) ----

// in: one [H][W][C] frame (fp32 R,G,B, or bytes B,G,R with swap), out: [out_h][out_w][3] bytes R,G,B
template <typename T>
inline void grid_resize_tile(const T* in, int32_t H, int32_t W, int32_t C, bool swap, int32_t out_h, int32_t out_w, const AreaCell* xc,
                             const AreaCell* yc, int32_t mode, uint8_t* out) {
    const float inv = mode == GRID_FAST || mode == GRID_FAST_2X2 ? grid_fast_inv(H, W, out_h, out_w) : 1.0f;
    for (int32_t dy = 0; dy < out_h; ++dy)
        for (int32_t dx = 0; dx < out_w; ++dx)
            for (int32_t c = 0; c < 3; ++c) {
                const int32_t sc = swap ? 2 - c : c;
                const AreaCell& x = xc[dx];
                const AreaCell& y = yc[dy];
                float sum = 0.0f;
                int32_t isum = 0, r[2] = {0, 0};
                for (int32_t j = 0; j < y.count; ++j) {
                    const T* row = in + ((int64_t)(y.first + j) * W + x.first) * C + sc;
                    float buf = 0.0f;
                    for (int32_t k = 0; k < x.count; ++k) {
                        const uint8_t s = grid_quant(row[(int64_t)k * C]);
                        buf = grid_term_general(buf, s, area_weight(x, k));
                        isum = grid_term_fast(isum, s);
                    }
                    sum = area_fold(sum, buf, area_weight(y, j), j == 0);
                    if (j < 2) r[j] = grid_row_linear(grid_quant(row[0]), grid_quant(row[(int64_t)(x.count - 1) * C]), x);
                }
                uint8_t o;
                if (mode == GRID_GENERAL) o = area_cast(sum);
                else if (mode == GRID_LINEAR) o = grid_byte_linear(r[0], r[y.count - 1 > 0 ? 1 : 0], y);
                else o = area_fast_cast(isum, inv, mode == GRID_FAST_2X2);
                out[((int64_t)dy * out_w + dx) * 3 + c] = o;
            }
}

}  // namespace vrg
