// vrg_prepare_math.hpp -- the band / segment plan of the Video Enhance Prepare kernels (csrc/vrg_prepare.hip), host and device, and the one
// place where a value becomes a PNG byte.  The resampling arithmetic itself is vrg_resize_math.hpp, unchanged: the kernels here call
// rs_taps / rs_dot / rs_pixel / rs_scale and are bit-identical to vrg_resize_f32.
//
// The plan.  An output frame is cut into bands of PREP_BAND rows and segments of `cps` columns; a workgroup owns one band of one segment
// of one output frame.  The bicubic kernel stages the source columns that the segment's x taps touch (prep_source_span) in a buffer of
// PREP_STAGE_FLOATS floats, so `cps` is the largest count, at most PREP_THREADS (one column per thread), at which every segment's span
// fits (prep_plan); the direct kernels take cps = PREP_THREADS.  The host check (tests/host_math/prepare_check.cpp) walks the same
// functions: every row and column covered exactly once, every span inside the buffer.
#pragma once
#include "vrg_resize_math.hpp"

namespace vrg {

constexpr int PREP_THREADS = 256;
constexpr int PREP_BAND = 8;
constexpr int PREP_STAGE_FLOATS = 4096;

// rintf(v * 255.0f) of an already clamped value: numpy's (x * 255).round().astype("uint8") in fp32, ties to even
VRG_HD uint8_t prep_byte(float v) { return (uint8_t)(int32_t)__builtin_rintf(v * 255.0f); }

// columns [c0, c1) of segment s, rows [r0, r1) of band b
VRG_HD void prep_segment(int32_t cps, int32_t out_w, int32_t s, int32_t& c0, int32_t& c1) {
    const int64_t a = (int64_t)s * cps, b = a + cps;
    c0 = (int32_t)(a < out_w ? a : out_w);
    c1 = (int32_t)(b < out_w ? b : out_w);
}
VRG_HD void prep_band(int32_t out_h, int32_t b, int32_t& r0, int32_t& r1) { prep_segment(PREP_BAND, out_h, b, r0, r1); }

// The source columns [lo, hi) of the input frame that the bicubic x taps of output columns [c0, c1) touch; false: none of these columns
// lies in the destination rectangle (nothing to stage, the segment is padding).  rs_source is monotone in the column, floor and the
// clamp of rs_taps keep that, so the first tap of the first column and the last tap of the last column bound every tap in between.
VRG_HD bool prep_source_span(const ResizeGeom& g, int32_t c0, int32_t c1, int32_t& lo, int32_t& hi) {
    const int64_t end = (int64_t)g.dx0 + g.dw;
    const int32_t a = c0 > g.dx0 ? c0 : g.dx0, b = (int32_t)(c1 < end ? c1 : end);
    lo = hi = 0;
    if (a >= b) return false;
    const float sx = rs_scale(g.sw, g.dw);
    int32_t ix[4];
    float w[4];
    rs_taps(a - g.dx0, sx, g.sw, ix, w);
    lo = g.sx0 + ix[0];
    rs_taps(b - 1 - g.dx0, sx, g.sw, ix, w);
    hi = g.sx0 + ix[3] + 1;
    return true;
}

// The ring of four horizontally resampled source rows (`have`, -1 = empty) against the rows `want` of the next output row: the smallest
// s in 0 .. 4 such that have[j + s] == want[j] for every j < 4 - s.  Slots 0 .. 3 - s are kept (moved down by s), the last s are new.
VRG_HD int prep_ring_shift(const int32_t (&have)[4], const int32_t (&want)[4]) {
    for (int s = 0; s < 4; ++s) {
        bool ok = true;
        for (int j = 0; j + s < 4; ++j) ok = ok && have[j + s] == want[j];
        if (ok) return s;
    }
    return 4;
}

struct PrepPlan {
    int32_t cps, segments, bands;
};

// false: a single column's taps do not fit the stage buffer (more than PREP_STAGE_FLOATS / 4 channels), or more bands than a launch takes
inline bool prep_plan(const ResizeGeom& g, bool staged, PrepPlan& p) {
    p.bands = (int32_t)(((int64_t)g.out_h + PREP_BAND - 1) / PREP_BAND);
    p.cps = g.out_w < PREP_THREADS ? g.out_w : PREP_THREADS;
    if (staged) {
        for (;;) {
            bool fits = true;
            const int32_t segments = (int32_t)(((int64_t)g.out_w + p.cps - 1) / p.cps);
            for (int32_t s = 0; s < segments && fits; ++s) {
                int32_t c0, c1, lo, hi;
                prep_segment(p.cps, g.out_w, s, c0, c1);
                if (prep_source_span(g, c0, c1, lo, hi)) fits = (int64_t)(hi - lo) * g.in_c <= PREP_STAGE_FLOATS;
            }
            if (fits) break;
            if (p.cps == 1) return false;
            p.cps -= p.cps > 16 ? p.cps / 16 : 1;
        }
    }
    p.segments = (int32_t)(((int64_t)g.out_w + p.cps - 1) / p.cps);
    return p.bands <= 65535 && p.segments <= 0x7fffffff;
}

}  // namespace vrg
