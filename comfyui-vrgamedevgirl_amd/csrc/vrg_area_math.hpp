// vrg_area_math.hpp -- arithmetic of the shot-aware Face Fix cut score (csrc/vrg_cut.hip), host and device.
//
// What is restated: VRGDGFaceFixPrepareShotAware._cut_score (VRGDG_StandaloneFaceFixNodes.py:421-435) and the quantisation in front of it
// (:456), as OpenCV 4.x evaluates them.  No cv2 is at hand where this was written: the restatement is pinned by an independent numpy
// restatement (tests/cut_support.py), by the exact area average in float64 (at most one level away) and -- wherever cv2 can be imported or
// tests/golden/cut_score_cv2.npz exists -- by cv2 itself.
//
//   bytes      rint(fl(clamp(x, 0, 1) * 255.0f)), round half to even, channels 0..2 of an fp32 frame (NaN is undefined in the reference;
//              here it gives 0)
//   resize     cv2.resize(rgb, (64, 64), INTER_AREA) for sides >= 64.  Per axis (computeResizeAreaTab, double, scale = n_in / 64.0), for
//              the output index d: fs1 = d * scale, fs2 = fs1 + scale, cell = min(scale, n_in - fs1), s1 = ceil(fs1),
//              s2 = min(floor(fs2), n_in - 1), s1 = min(s1, s2); the taps, in this order:
//                (s1 - 1, (float)((s1 - fs1) / cell))                        if s1 - fs1 > 1e-3
//                (s,      (float)(1.0 / cell))                               for s in [s1, s2)
//                (s2,     (float)(min(min(fs2 - s2, 1.0), cell) / cell))     if fs2 - s2 > 1e-3
//              The taps of one d are consecutive source samples, and all but the first and the last carry the same weight: an AreaCell
//              (first sample, count, first / middle / last weight) holds them.
//              general path (resizeArea_<uchar, float>), fp32, two roundings per term, no FMA: per source row buf[d] = 0, then over the x
//              taps in order buf = fl(buf + fl(S * alpha)); per output row over its y taps in order sum = fl(beta * buf) for the first,
//              sum = fl(sum + fl(beta * buf)) for the others; byte = clip(rint(sum), 0, 255).
//              fast path (both n_in / 64 integers): the integer sum of the sx x sy cell, (float)sum * (1.0f / (sx * sy)), rint, clip; a
//              128 x 128 source is (a + b + c + d + 2) >> 2; a 64 x 64 source comes back as it is (the sum of one byte times 1.0f).
//   HSV        cvtColor(COLOR_RGB2HSV) on bytes, 12-bit fixed point: v = max, diff = v - min, s = (diff * sdiv[v] + 2048) >> 12,
//              h = (g - b | b - r + 2 diff | r - g + 4 diff) for v == (r | g | b) in that order of preference,
//              h = (h * hdiv[diff] + 2048) >> 12, + 180 if negative; sdiv[i] = rint((255 << 12) / (double)i), hdiv[i] = rint((180 << 12) /
//              (6.0 * i)), both 0 at i = 0.
//   histogram  calcHist([hsv], [0, 1], None, [32, 32], [0, 180, 0, 256]): bin = (8 * h) / 45 * 32 + (s >> 3).
//   score      the correlation of two histograms does not change when each is divided by its L2 norm, so the device returns exact
//              integers per consecutive pair -- D = sum |a - b| over the 12288 thumbnail bytes, S11, S22, S12 over the two histograms --
//              and the host finishes in double (VRGDG_StandaloneFaceFixNodes.cut_scores_from_sums).
#pragma once
#include <stdint.h>

#include "vrg_pixel_math.hpp"

#include <math.h>

namespace vrg {

constexpr int AREA_OUT = 64;                       // the thumbnail is 64 x 64
constexpr int AREA_THUMB_BYTES = AREA_OUT * AREA_OUT * 3;
constexpr int AREA_HIST_BINS = 32 * 32;

enum AreaMode { AREA_GENERAL = 0, AREA_FAST = 1, AREA_FAST_2X2 = 2 };

// The taps of one output column or row: source samples first .. first + count - 1; tap 0 weighs w_first, tap count - 1 (when count > 1)
// w_last, every tap between them w_mid.
struct AreaCell {
    int32_t first, count;
    float w_first, w_mid, w_last;
};
static_assert(sizeof(AreaCell) == 20, "AreaCell is 20 bytes: the table layout of vrg_area_taps");

VRG_HD float area_weight(const AreaCell& c, int32_t k) { return k == 0 ? c.w_first : (k == c.count - 1 ? c.w_last : c.w_mid); }

inline int area_mode(int32_t in_h, int32_t in_w) {
    if (in_h % AREA_OUT != 0 || in_w % AREA_OUT != 0) return AREA_GENERAL;
    return (in_h == 2 * AREA_OUT && in_w == 2 * AREA_OUT) ? AREA_FAST_2X2 : AREA_FAST;
}

// HOST: the cell of output index d of an axis with n_in samples reduced by `scale` >= 1 (computeResizeAreaTab; the caller forms the scale)
inline AreaCell area_cell_scaled(int32_t d, int32_t n_in, double scale) {
    const double fs1 = (double)d * scale, fs2 = fs1 + scale;
    const double rest = (double)n_in - fs1, cell = scale < rest ? scale : rest;
    int32_t s1 = (int32_t)ceil(fs1), s2 = (int32_t)floor(fs2);
    if (s2 > n_in - 1) s2 = n_in - 1;
    if (s1 > s2) s1 = s2;
    const bool head = (double)s1 - fs1 > 1e-3, tail = fs2 - (double)s2 > 1e-3;
    AreaCell c;
    c.first = head ? s1 - 1 : s1;
    c.count = (head ? 1 : 0) + (s2 - s1) + (tail ? 1 : 0);
    c.w_mid = (float)(1.0 / cell);
    double part = fs2 - (double)s2;
    if (part > 1.0) part = 1.0;
    if (part > cell) part = cell;
    const float w_head = (float)(((double)s1 - fs1) / cell), w_tail = (float)(part / cell);
    c.w_first = head ? w_head : (s2 > s1 ? c.w_mid : w_tail);
    c.w_last = tail ? w_tail : (s2 > s1 ? c.w_mid : w_head);
    return c;
}

// HOST: the cell of output index d of an axis with n_in >= 64 samples
inline AreaCell area_cell(int32_t d, int32_t n_in) { return area_cell_scaled(d, n_in, (double)n_in / (double)AREA_OUT); }

// 64 column cells, then 64 row cells
inline void area_fill_cells(int32_t in_h, int32_t in_w, AreaCell* cells) {
    for (int32_t d = 0; d < AREA_OUT; ++d) cells[d] = area_cell(d, in_w);
    for (int32_t d = 0; d < AREA_OUT; ++d) cells[AREA_OUT + d] = area_cell(d, in_h);
}

// (video_frames[...] .clamp(0, 1) * 255).round().astype(uint8)
VRG_HD uint8_t area_quant(float x) {
    const float c = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);             // NaN -> 0
    return (uint8_t)(int32_t)__builtin_rintf(c * 255.0f);
}

// saturate_cast<uchar>(float)
VRG_HD uint8_t area_cast(float sum) {
    const float r = __builtin_rintf(sum);
    return (uint8_t)(int32_t)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

// the general path's two steps
VRG_HD float area_add(float acc, uint8_t s, float w) { return acc + (float)s * w; }
VRG_HD float area_fold(float sum, float buf, float beta, bool first) { return first ? beta * buf : sum + beta * buf; }

// the fast path's last step: inv = 1.0f / (sx * sy)
VRG_HD uint8_t area_fast_cast(int32_t sum, float inv, bool two_by_two) {
    return two_by_two ? (uint8_t)((sum + 2) >> 2) : area_cast((float)sum * inv);
}

VRG_HD int32_t area_sdiv(int32_t i) { return i ? (int32_t)rint((double)(255 << 12) / (double)i) : 0; }
VRG_HD int32_t area_hdiv(int32_t i) { return i ? (int32_t)rint((double)(180 << 12) / (6.0 * (double)i)) : 0; }

// bin of one R,G,B byte pixel; sdiv_v = area_sdiv(v), hdiv_d = area_hdiv(diff) come from the caller's tables through the two functions
template <typename SDIV, typename HDIV>
VRG_HD int32_t area_hsv_bin(int32_t r, int32_t g, int32_t b, SDIV sdiv, HDIV hdiv, int32_t* h_out = nullptr, int32_t* s_out = nullptr) {
    int32_t v = r > g ? r : g, lo = r < g ? r : g;
    v = v > b ? v : b;
    lo = lo < b ? lo : b;
    const int32_t diff = v - lo;
    const int32_t s = (diff * sdiv(v) + (1 << 11)) >> 12;
    int32_t h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv(diff) + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    if (h_out) *h_out = h;
    if (s_out) *s_out = s;
    return (8 * h) / 45 * 32 + (s >> 3);
}

// ---- HOST: everything straight from the definition (tests/host_math/cut_check.cpp; never called from a kernel) ----

// in: one [H][W][C] fp32 frame, out: [64][64][3] bytes
inline void area_thumbnail(const float* in, int32_t H, int32_t W, int32_t C, const AreaCell* cells, uint8_t* out) {
    const AreaCell* xc = cells;
    const AreaCell* yc = cells + AREA_OUT;
    const int mode = area_mode(H, W);
    const float inv = 1.0f / (float)((W / AREA_OUT) * (H / AREA_OUT));
    for (int32_t dy = 0; dy < AREA_OUT; ++dy)
        for (int32_t dx = 0; dx < AREA_OUT; ++dx)
            for (int32_t c = 0; c < 3; ++c) {
                float sum = 0.0f;
                int32_t isum = 0;
                for (int32_t j = 0; j < yc[dy].count; ++j) {
                    const float* row = in + ((int64_t)(yc[dy].first + j) * W + xc[dx].first) * C + c;
                    float buf = 0.0f;
                    for (int32_t k = 0; k < xc[dx].count; ++k) {
                        const uint8_t s = area_quant(row[(int64_t)k * C]);
                        buf = area_add(buf, s, area_weight(xc[dx], k));
                        isum += s;
                    }
                    sum = area_fold(sum, buf, area_weight(yc[dy], j), j == 0);
                }
                out[(dy * AREA_OUT + dx) * 3 + c] = mode == AREA_GENERAL ? area_cast(sum) : area_fast_cast(isum, inv, mode == AREA_FAST_2X2);
            }
}

inline void area_histogram(const uint8_t* thumb, int32_t* hist) {
    for (int i = 0; i < AREA_HIST_BINS; ++i) hist[i] = 0;
    for (int p = 0; p < AREA_OUT * AREA_OUT; ++p)
        hist[area_hsv_bin(thumb[3 * p], thumb[3 * p + 1], thumb[3 * p + 2], area_sdiv, area_hdiv)] += 1;
}

// sums = (D, S11, S22, S12) of the pair (a = the earlier frame, b = the later one)
inline void area_pair_sums(const uint8_t* a, const uint8_t* b, const int32_t* ha, const int32_t* hb, int64_t sums[4]) {
    int64_t d = 0, s11 = 0, s22 = 0, s12 = 0;
    for (int i = 0; i < AREA_THUMB_BYTES; ++i) d += a[i] > b[i] ? a[i] - b[i] : b[i] - a[i];
    for (int i = 0; i < AREA_HIST_BINS; ++i) {
        s11 += (int64_t)ha[i] * ha[i];
        s22 += (int64_t)hb[i] * hb[i];
        s12 += (int64_t)ha[i] * hb[i];
    }
    sums[0] = d; sums[1] = s11; sums[2] = s22; sums[3] = s12;
}

}  // namespace vrg
