// vrg_pil_math.hpp -- arithmetic of the far-face repair composite (csrc/vrg_farface.hip), host and device.
//
// What is restated: `composite` of the reference's scripts/far_face_repair_backend.py (:339-371) -- which is Pillow and numpy, not cv2, so
// every rule below is pinned against the installed Pillow itself (tests/test_far_face_host.py), byte for byte.
//   resize (:357-358)       Image.resize(size, LANCZOS) on RGB / L bytes: csrc/vrg_pil_resample.hpp, which this header includes and which the
//                           reference sheets and the contact sheet (`contact_sheet` of the same backend, :374-408) share.
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
#pragma once
#include <stdint.h>

#include "vrg_pil_resample.hpp"
#include "vrg_pixel_math.hpp"

#include <math.h>

namespace vrg {

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
