// vrg_pil_math.hpp -- arithmetic of the far-face repair composite (csrc/vrg_farface.hip), host and device.
//
// What is restated: `composite` of the reference's scripts/far_face_repair_backend.py (:339-371) -- which is Pillow and numpy, not cv2, so
// every rule below is pinned against the installed Pillow itself (tests/test_far_face_host.py), byte for byte.
//   resize (:357-358)       Image.resize(size, LANCZOS) on RGB / L bytes (Pillow's Resample.c).  Separable; the horizontal pass writes a
//                           rounded byte image, then the vertical pass runs; a pass whose size does not change is skipped.  Per axis, in
//                           double: scale = in / out, fs = max(scale, 1), support = 3 fs, ksize = 2 ceil(support) + 1;  for output xx:
//                           c = (xx + 0.5) scale, xmin = max(int(c - support + 0.5), 0), xmax = min(int(c + support + 0.5), in),
//                           w_x = L((x + xmin - c + 0.5) / fs), L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3, divided by their sum in index
//                           order, then fixed to 22 bits: int(w 2^22 +- 0.5).  pixel = clip((2^21 + sum byte * k) >> 22, 0, 255).  The
//                           tables are made on the HOST (pil_lanczos_table): no kernel evaluates a sine.
//   blur (:210)             ImageFilter.GaussianBlur(radius = sigma) on L (BoxBlur.c): three box passes along the rows, then three along
//                           the columns, every pass rounded to bytes.  In C `float`: s2 = sigma^2 / 3, L = sqrt(12 s2 + 1),
//                           l = floor((L - 1) / 2), a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), R = l + a, r = int(R),
//                           ww = int(2^24 / (2R + 1)) -- the quotient ROUNDED TO FLOAT first (sigma = 1: 11184811, not ...810) --
//                           fw = (2^24 - (2r + 1) ww) / 2.  pixel = (ww sum_{|i| <= r} in[clamp(x + i)] + fw (in[clamp(x - r - 1)] +
//                           in[clamp(x + r + 1)]) + 2^23) >> 24 in uint32.  All terms are integers, so a prefix sum gives the bytes of
//                           Pillow's running accumulator (pil_box_pixel).
//   ellipse (:208)          ImageDraw.ellipse is NOT restated: its first and last set column per row come from Pillow on the host.
//   colour match (:214-224) selected = mask >= 64 (alpha > 0.25); x[selected].mean(axis = 0) of float32 rows is numpy's SEQUENTIAL fp32 sum
//                           in row-major order divided by the count in fp32 -- not the exact mean once a sum passes 2^24.  Every value
//                           such a sum takes is an integer; within one binade adding a byte is acc -> acc + d[parity of acc / ulp]
//                           (round to nearest even), and such maps compose associatively (NpMap), so a run of pixels reduces in parallel
//                           and applies at once wherever the sum stays below the next power of two; elsewhere it is walked in order
//                           with real fp32 adds (np_walk).  shift = fl(fl(orig_mean - rep_mean) * 0.65f);
//                           byte = trunc(clip(fl((float)rep + shift), 0, 255)); fewer than 16 selected: no shift.
//   paste (:366)            Image.paste(rgb, box, L mask): t = o (255 - m) + r m + 128, out = ((t >> 8) + t) >> 8 -- ONE rounded division.
//
// The contact sheet of the same backend (`contact_sheet`, :374-408; csrc/vrg_thumb.hip) adds Image.thumbnail, which is NOT a plain resize:
//   size (Image.py)         thumbnail((x, y)): x, y floored; nothing is done when x >= w and y >= h.  In double: aspect = w / h; where
//                           x / y >= aspect, x = round_aspect(y aspect) judged by |aspect - n / y|, else y = round_aspect(x / aspect)
//                           judged by |aspect - x / n| (0 for n = 0); round_aspect takes floor or ceil, the floor on a tie, at least 1.
//   factors                 with reducing_gap g (default 2.0): f = int(w / out_w / g) or 1 per axis, in double.
//   reduce (Reduce.c)       Image.reduce((fx, fy)): output (X, Y) averages the cell [X fx, min((X + 1) fx, w)) x [Y fy, min((Y + 1) fy, h)),
//                           the size is rounded up.  Pillow takes one of many routes -- NxN, 1xN, Nx1, the special 2x2 3x3 4x4 5x5 (shifts
//                           for powers of two, a multiplier else) and its corner routine for the partial last column, row and corner --
//                           and ALL of them give, for a cell of n pixels, ((sum + n / 2) * (2^24 / n)) >> 24 in uint32 with both
//                           divisions truncated (pil_reduce_byte): for n a power of two that is the shift (sum + n / 2) >> log2 n, and
//                           for n = 1 the byte itself.  The largest product, (255 n + n / 2)(2^24 / n) <= 255.5 * 2^24, fits uint32.
//                           Established per route against the installed Pillow over EVERY sum of a cell (tests/test_contact_sheet_host.py).
//   box resize (Resample.c) Image.resize(size, filter, box = (0, 0, w / fx, h / fy)) of the reduced picture: precompute_coeffs with a
//                           source box.  The box reaches C as `float`: in0, in1 are fp32, scale = (double)(in1 - in0) / out with the
//                           difference taken in fp32, center = in0 + (xx + 0.5) scale, the rest as for resize above with the filter's
//                           support (pil_filter_table).  BICUBIC: a = -0.5, support 2: ((a + 2) t - (a + 3)) t t + 1 for t < 1,
//                           (((t - 5) t + 8) t - 4) a for t < 2.  A pass is skipped only where out == in and the box is the whole axis.
//                           A reduced picture more than 100 times as tall as wide resizes vertically first in Pillow: not restated, refused.
//   sheet (:398-406)        cols = max(1, columns), rows = ceil(n / cols), the cell is the largest thumbnail, thumbnail i is pasted at
//                           ((i % cols) cell_w, (i / cols) cell_h) on (24, 24, 24).
#pragma once
#include <stdint.h>

#include "vrg_pixel_math.hpp"

#include <math.h>

namespace vrg {

constexpr int PIL_PRECISION_BITS = 22;
constexpr int PIL_STATS_WORDS = 12;       // uint32 per frame: count, 3 original means, 3 repaired means, 3 shifts (fp32 bits), matched, 0
constexpr int PIL_MIN_SELECTED = 16;
constexpr int PIL_SELECT_FROM = 64;       // alpha > 0.25  <=>  mask >= 64
constexpr int PIL_MAX_LINE = 8192;        // the longest row / column of a mask the blur kernel holds in LDS
constexpr int NP_RUN = 8;                 // consecutive pixels one lane folds into a map
constexpr int NP_CHUNK = 256 * NP_RUN;    // pixels a workgroup reduces at once

struct PilSpan {
    int32_t x0, x1;                       // the set columns of a row; x0 > x1 = none
};

// ---------------------------------------------------------------------------------------------------------------------------------
// resize
// ---------------------------------------------------------------------------------------------------------------------------------
inline double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}

inline double pil_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? pil_sinc(x) * pil_sinc(x / 3) : 0.0; }

inline int32_t pil_lanczos_ksize(int32_t n_in, int32_t n_out) {
    const double scale = (double)n_in / n_out;
    return (int32_t)ceil(3.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// HOST.  bounds: [n_out][2] (first source index, tap count); weights: [n_out][ksize], zero beyond the count
inline void pil_lanczos_table(int32_t n_in, int32_t n_out, int32_t* bounds, int32_t* weights) {
    const double scale = (double)n_in / n_out, fs = scale < 1.0 ? 1.0 : scale, support = 3.0 * fs, ss = 1.0 / fs;
    const int32_t ksize = pil_lanczos_ksize(n_in, n_out);
    double* k = new double[(size_t)ksize];
    for (int32_t xx = 0; xx < n_out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int32_t xmin = (int32_t)(center - support + 0.5), xmax = (int32_t)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < xmax; ++x) {
            k[x] = pil_lanczos((x + xmin - center + 0.5) * ss);
            ww += k[x];
        }
        int32_t* w = weights + (size_t)xx * ksize;
        for (int32_t x = 0; x < ksize; ++x) {
            if (x >= xmax) {
                w[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? k[x] / ww : k[x];
            w[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PIL_PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PIL_PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    delete[] k;
}

VRG_HD uint8_t pil_clip8(int32_t ss) {
    const int32_t v = ss >> PIL_PRECISION_BITS;                              // arithmetic
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// one output pixel of one pass: `n` taps with weights w[0 .. n), load(i, c) = channel c of tap i
template <int C, class Load>
VRG_HD void pil_taps(const int32_t* w, int32_t n, Load load, uint8_t* out) {
    int32_t ss[C];
    for (int c = 0; c < C; ++c) ss[c] = 1 << (PIL_PRECISION_BITS - 1);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t k = w[i];
        for (int c = 0; c < C; ++c) ss[c] += (int32_t)load(i, c) * k;
    }
    for (int c = 0; c < C; ++c) out[c] = pil_clip8(ss[c]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// thumbnail: reduce, a filter over a source box, the size rule, the sheet
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int PIL_FILTER_LANCZOS = 1;     // Pillow's own numbers (Image.Resampling)
constexpr int PIL_FILTER_BICUBIC = 3;
constexpr int PIL_TALL_RATIO = 100;       // Image.resize goes vertically first beyond it

// one byte of Image.reduce: the sum of a cell of n pixels (n >= 1, sum <= 255 n)
VRG_HD uint8_t pil_reduce_byte(uint32_t sum, uint32_t n) { return (uint8_t)(((sum + (n >> 1)) * ((1u << 24) / n)) >> 24); }

VRG_HD int32_t pil_reduced_size(int32_t n, int32_t f) { return (n + f - 1) / f; }

// HOST.  Image.reduce((fx, fy)) of src[h][w][C] into dst[ceil(h / fy)][ceil(w / fx)][C]
inline void pil_reduce_image(const uint8_t* src, int32_t h, int32_t w, int32_t C, int32_t fx, int32_t fy, uint8_t* dst) {
    const int32_t rw = pil_reduced_size(w, fx), rh = pil_reduced_size(h, fy);
    for (int32_t Y = 0; Y < rh; ++Y)
        for (int32_t X = 0; X < rw; ++X) {
            const int32_t x0 = X * fx, x1 = x0 + fx < w ? x0 + fx : w, y0 = Y * fy, y1 = y0 + fy < h ? y0 + fy : h;
            for (int32_t c = 0; c < C; ++c) {
                uint32_t sum = 0;
                for (int32_t y = y0; y < y1; ++y)
                    for (int32_t x = x0; x < x1; ++x) sum += src[((int64_t)y * w + x) * C + c];
                dst[((int64_t)Y * rw + X) * C + c] = pil_reduce_byte(sum, (uint32_t)((x1 - x0) * (y1 - y0)));
            }
        }
}

inline double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

inline bool pil_filter_known(int32_t filter) { return filter == PIL_FILTER_BICUBIC || filter == PIL_FILTER_LANCZOS; }
inline double pil_filter_support(int32_t filter) { return filter == PIL_FILTER_BICUBIC ? 2.0 : 3.0; }
inline double pil_filter_value(int32_t filter, double x) { return filter == PIL_FILTER_BICUBIC ? pil_bicubic(x) : pil_lanczos(x); }

inline int32_t pil_filter_ksize(int32_t filter, float in0, float in1, int32_t n_out) {
    const double scale = (double)(in1 - in0) / n_out;
    return (int32_t)ceil(pil_filter_support(filter) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// HOST.  One axis of Image.resize(.., filter, box): n_out outputs from the source interval [in0, in1) of n_in pixels; bounds and weights
// as for pil_lanczos_table, which this equals for LANCZOS with the box (0, n_in)
inline void pil_filter_table(int32_t filter, int32_t n_in, float in0, float in1, int32_t n_out, int32_t* bounds, int32_t* weights) {
    const double scale = (double)(in1 - in0) / n_out, fs = scale < 1.0 ? 1.0 : scale, support = pil_filter_support(filter) * fs, ss = 1.0 / fs;
    const int32_t ksize = pil_filter_ksize(filter, in0, in1, n_out);
    double* k = new double[(size_t)ksize];
    for (int32_t xx = 0; xx < n_out; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        int32_t xmin = (int32_t)(center - support + 0.5), xmax = (int32_t)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < xmax; ++x) {
            k[x] = pil_filter_value(filter, (x + xmin - center + 0.5) * ss);
            ww += k[x];
        }
        int32_t* w = weights + (size_t)xx * ksize;
        for (int32_t x = 0; x < ksize; ++x) {
            if (x >= xmax) {
                w[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? k[x] / ww : k[x];
            w[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PIL_PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PIL_PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    delete[] k;
}

// HOST.  max(min(floor(v), ceil(v), key), 1) of Image.thumbnail: the floor on a tie
template <class Key>
inline double pil_round_aspect(double v, Key key) {
    const double lo = floor(v), hi = ceil(v);
    const double pick = key(hi) < key(lo) ? hi : lo;
    return pick < 1.0 ? 1.0 : pick;
}

// HOST.  the size Image.thumbnail((req_w, req_h)) gives a picture of w x h; false: the picture stays as it is.  req_w, req_h >= 1.
inline bool pil_thumbnail_size(int32_t w, int32_t h, double req_w, double req_h, int32_t* out_w, int32_t* out_h) {
    double x = floor(req_w), y = floor(req_h);
    if (x >= w && y >= h) return false;
    const double aspect = (double)w / h;
    if (x / y >= aspect) x = pil_round_aspect(y * aspect, [&](double n) { return fabs(aspect - n / y); });
    else y = pil_round_aspect(x / aspect, [&](double n) { return n == 0.0 ? 0.0 : fabs(aspect - x / n); });
    *out_w = (int32_t)x;
    *out_h = (int32_t)y;
    return true;
}

// HOST.  int(n_in / n_out / gap) or 1
inline int32_t pil_reduce_factor(int32_t n_in, int32_t n_out, double gap) {
    const double f = (double)n_in / n_out / gap;
    return f >= 2.0 ? (f > 2147483647.0 ? 2147483647 : (int32_t)f) : 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// blur
// ---------------------------------------------------------------------------------------------------------------------------------
struct PilBox {
    int32_t r;
    uint32_t ww, fw;
};

// HOST (C float arithmetic, no contraction)
inline PilBox pil_box_parameters(float sigma) {
    const float sigma2 = sigma * sigma / 3;
    const float L = (float)sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float radius = l + a;
    PilBox b;
    b.r = (int32_t)radius;
    b.ww = (uint32_t)((float)(1u << 24) / (radius * 2 + 1));
    b.fw = ((1u << 24) - (uint32_t)(b.r * 2 + 1) * b.ww) / 2;
    return b;
}

// pixel x of one box pass over a line of n bytes: prefix(i) = in(0) + .. + in(i - 1) for 0 <= i <= n
template <class Prefix, class In>
VRG_HD uint8_t pil_box_pixel(int32_t x, int32_t n, const PilBox& b, Prefix prefix, In in) {
    const int32_t r = b.r;
    const int32_t lo = x - r < 0 ? 0 : x - r, hi = x + r + 1 > n ? n : x + r + 1;
    const int32_t before = r - x > 0 ? r - x : 0, after = x + r - (n - 1) > 0 ? x + r - (n - 1) : 0;
    const int32_t fl = x - r - 1 < 0 ? 0 : x - r - 1, fr = x + r + 1 > n - 1 ? n - 1 : x + r + 1;
    const uint32_t acc = prefix(hi) - prefix(lo) + (uint32_t)in(0) * (uint32_t)before + (uint32_t)in(n - 1) * (uint32_t)after;
    const uint32_t bulk = acc * b.ww + ((uint32_t)in(fl) + (uint32_t)in(fr)) * b.fw;
    return (uint8_t)((bulk + (1u << 23)) >> 24);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// numpy's sequential fp32 sum of bytes
// ---------------------------------------------------------------------------------------------------------------------------------
// The sum is held as the integer it is.  Its binade gives the ulp 2^sh (sh = 0 below 2^24, where every add is exact).
VRG_HD uint32_t np_top_bit(uint64_t v) {
    uint32_t k = 0;
    while (v >>= 1) ++k;
    return k;
}

VRG_HD uint32_t np_ulp_shift(uint64_t acc) { return acc < (1ull << 24) ? 0u : np_top_bit(acc) - 23u; }

// the first value of the next binade: the sum must stay below it for the ulp to hold
VRG_HD uint64_t np_limit(uint64_t acc) { return acc < (1ull << 24) ? (1ull << 24) : (2ull << np_top_bit(acc)); }

// what fl(acc + b) adds to acc, a multiple of 2^sh whose unit has the given parity: round to nearest, ties to even
VRG_HD uint32_t np_inc(uint32_t b, uint32_t sh, uint32_t parity) {
    if (sh == 0) return b;
    if (sh > 9) return 0;                                                    // half an ulp is above 255
    const uint32_t unit = 1u << sh, q = b >> sh, rem = b & (unit - 1u), half = unit >> 1;
    const uint32_t up = (rem > half || (rem == half && ((q ^ parity) & 1u))) ? 1u : 0u;
    return (q + up) << sh;
}

struct NpMap {
    uint32_t d[2];                                                           // acc -> acc + d[(acc >> sh) & 1]
};

VRG_HD void np_map_push(NpMap& m, uint32_t b, uint32_t sh) {
    for (int p = 0; p < 2; ++p) m.d[p] += np_inc(b, sh, (uint32_t)p ^ ((m.d[p] >> sh) & 1u));
}

// first f, then g
VRG_HD NpMap np_map_then(const NpMap& f, const NpMap& g, uint32_t sh) {
    NpMap h;
    for (int p = 0; p < 2; ++p) h.d[p] = f.d[p] + g.d[((uint32_t)p ^ (f.d[p] >> sh)) & 1u];
    return h;
}

// applies a run's map if the sum stays inside its binade (all steps increase it, so the end decides); false: walk the run instead
VRG_HD bool np_apply(uint64_t& acc, const NpMap& m, uint32_t sh) {
    const uint64_t next = acc + m.d[(acc >> sh) & 1u];
    if (next >= np_limit(acc)) return false;
    acc = next;
    return true;
}

// the definition: real fp32 adds in order (`stride` bytes apart)
VRG_HD uint64_t np_walk(uint64_t acc, const uint8_t* b, int32_t n, int32_t stride) {
    float a = (float)acc;
    for (int32_t i = 0; i < n; ++i) a = a + (float)b[(int64_t)i * stride];
    return (uint64_t)a;
}

// stats: the record of one frame; sums: original x3, repaired x3
VRG_HD void np_finish(uint32_t count, const uint64_t* sums, float strength, uint32_t* stats) {
    float m[6];
    const float n = (float)(count ? count : 1u);
    for (int i = 0; i < 6; ++i) m[i] = (float)sums[i] / n;
    stats[0] = count;
    for (int i = 0; i < 6; ++i) stats[1 + i] = f32_bits(m[i]);
    for (int c = 0; c < 3; ++c) {
        const float d = m[c] - m[3 + c];
        stats[7 + c] = f32_bits(d * strength);
    }
    stats[10] = count >= (uint32_t)PIL_MIN_SELECTED ? 1u : 0u;
    stats[11] = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// paste
// ---------------------------------------------------------------------------------------------------------------------------------
VRG_HD uint8_t pil_shift_byte(uint8_t rep, float shift) {
    float v = (float)rep + shift;
    v = v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v;
    return (uint8_t)v;
}

VRG_HD uint8_t pil_paste_byte(uint8_t o, uint8_t r, uint8_t m) {
    const uint32_t t = (uint32_t)o * (255u - m) + (uint32_t)r * m + 128u;
    return (uint8_t)(((t >> 8) + t) >> 8);
}

}  // namespace vrg
