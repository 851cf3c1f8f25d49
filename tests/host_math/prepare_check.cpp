// Test scaffolding: csrc/vrg_prepare_math.hpp compiled for the host (g++, -ffp-contract=off): the band / segment plan of the Video Enhance
// Prepare kernels, and the walk of k_prepare_bicubic (csrc/vrg_prepare.hip) replayed with the same functions -- a ring of four
// horizontally resampled rows moved by prep_ring_shift, taps taken out of a staged span -- so that its order of products and sums is
// compared with rs_pixel without a GPU (tests/test_prepare_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <string.h>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_prepare_math.hpp"

using namespace vrg;

static ResizeGeom geom(const int32_t* g) {
    return ResizeGeom{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12]};
}

extern "C" {

int32_t hm_prepare_constants(int32_t which) { return which == 0 ? PREP_THREADS : which == 1 ? PREP_BAND : PREP_STAGE_FLOATS; }

// plan: cps, segments, bands; 0 = the plan refuses the geometry
int32_t hm_prepare_plan(const int32_t* g13, int32_t staged, int32_t* plan3) {
    PrepPlan p;
    if (!rs_geom_ok(geom(g13)) || !prep_plan(geom(g13), staged != 0, p)) return 0;
    plan3[0] = p.cps;
    plan3[1] = p.segments;
    plan3[2] = p.bands;
    return 1;
}

// The walk of a whole launch over one output frame.  rows[out_h] and cols[out_w] count how often a row / column is owned by a band /
// segment; worst[0] = the most floats a segment stages, worst[1] = the most often one source row is staged by one workgroup,
// worst[2] = the most source rows two neighbouring bands both stage.  Returns the number of staged taps outside their span (0 wanted).
int64_t hm_prepare_cover(const int32_t* g13, int32_t staged, int32_t* rows, int32_t* cols, int64_t* worst) {
    const ResizeGeom g = geom(g13);
    PrepPlan p;
    if (!prep_plan(g, staged != 0, p)) return -1;
    memset(rows, 0, sizeof(int32_t) * (size_t)g.out_h);
    memset(cols, 0, sizeof(int32_t) * (size_t)g.out_w);
    worst[0] = worst[1] = worst[2] = 0;
    int64_t outside = 0;
    for (int32_t b = 0; b < p.bands; ++b) {
        int32_t r0, r1;
        prep_band(g.out_h, b, r0, r1);
        for (int32_t r = r0; r < r1; ++r) ++rows[r];
    }
    const float sx = rs_scale(g.sw, g.dw), sy = rs_scale(g.sh, g.dh);
    for (int32_t s = 0; s < p.segments; ++s) {
        int32_t c0, c1, lo, hi;
        prep_segment(p.cps, g.out_w, s, c0, c1);
        for (int32_t c = c0; c < c1; ++c) ++cols[c];
        if (!staged || !prep_source_span(g, c0, c1, lo, hi)) continue;
        const int64_t n = (int64_t)(hi - lo) * g.in_c;
        worst[0] = n > worst[0] ? n : worst[0];
        for (int32_t c = c0; c < c1; ++c) {
            const int32_t dx = c - g.dx0;
            if (dx < 0 || dx >= g.dw) continue;
            int32_t ix[4];
            float w[4];
            rs_taps(dx, sx, g.sw, ix, w);
            for (int i = 0; i < 4; ++i) outside += (g.sx0 + ix[i] < lo || g.sx0 + ix[i] >= hi) ? 1 : 0;
        }
    }
    if (!staged) return outside;
    int32_t* staged_rows = new int32_t[(size_t)g.sh];
    int32_t* before = new int32_t[(size_t)g.sh];
    memset(before, 0, sizeof(int32_t) * (size_t)g.sh);
    for (int32_t b = 0; b < p.bands; ++b) {
        int32_t r0, r1;
        prep_band(g.out_h, b, r0, r1);
        memset(staged_rows, 0, sizeof(int32_t) * (size_t)g.sh);
        int32_t hy[4] = {-1, -1, -1, -1};
        for (int32_t oy = r0; oy < r1; ++oy) {
            const int32_t dy = oy - g.dy0;
            if (dy < 0 || dy >= g.dh) continue;
            int32_t iy[4];
            float w[4];
            rs_taps(dy, sy, g.sh, iy, w);
            const int sh = prep_ring_shift(hy, iy);
            for (int j = 4 - sh; j < 4; ++j)
                if (!(j > 0 && iy[j] == iy[j - 1])) ++staged_rows[iy[j]];
            for (int j = 0; j < 4; ++j) hy[j] = iy[j];
        }
        int64_t shared = 0;
        for (int32_t y = 0; y < g.sh; ++y) {
            worst[1] = staged_rows[y] > worst[1] ? staged_rows[y] : worst[1];
            shared += (staged_rows[y] && before[y]) ? 1 : 0;
        }
        worst[2] = shared > worst[2] ? shared : worst[2];
        memcpy(before, staged_rows, sizeof(int32_t) * (size_t)g.sh);
    }
    delete[] staged_rows;
    delete[] before;
    return outside;
}

// k_prepare_bicubic replayed on the host for `frames` frames picked by index (null: in order): out_f32 and out_u8, either may be null
void hm_prepare_bicubic(const float* in, const int32_t* index, int64_t n_out, const int32_t* g13, float* out_f32, uint8_t* out_u8) {
    const ResizeGeom g = geom(g13);
    PrepPlan p;
    if (!prep_plan(g, true, p)) return;
    const float sx = rs_scale(g.sw, g.dw), sy = rs_scale(g.sh, g.dh);
    float* stage = new float[PREP_STAGE_FLOATS];
    for (int64_t z = 0; z < n_out; ++z) {
        const float* fin = in + (index ? index[z] : z) * (int64_t)g.in_h * g.in_w * g.in_c;
        for (int32_t b = 0; b < p.bands; ++b)
            for (int32_t s = 0; s < p.segments; ++s) {
                int32_t c0, c1, r0, r1, lo, hi;
                prep_segment(p.cps, g.out_w, s, c0, c1);
                prep_band(g.out_h, b, r0, r1);
                const bool any = prep_source_span(g, c0, c1, lo, hi);
                const int n = (hi - lo) * g.in_c;
                for (int32_t c = c0; c < c1; ++c) {                            // one "thread"
                    const int32_t dx = c - g.dx0;
                    const bool in_x = dx >= 0 && dx < g.dw;
                    int32_t ix[4], hy[4] = {-1, -1, -1, -1};
                    float wx[4], h[4][3] = {};
                    rs_taps(in_x ? dx : 0, sx, g.sw, ix, wx);
                    for (int i = 0; i < 4; ++i) ix[i] = (g.sx0 + ix[i] - lo) * g.in_c;
                    for (int32_t oy = r0; oy < r1; ++oy) {
                        const int32_t dy = oy - g.dy0;
                        float val[3] = {0.0f, 0.0f, 0.0f};
                        if (any && dy >= 0 && dy < g.dh) {
                            int32_t iy[4];
                            float wy[4];
                            rs_taps(dy, sy, g.sh, iy, wy);
                            const int sh = prep_ring_shift(hy, iy);
                            if (sh > 0 && sh < 4)
                                for (int j = 0; j + sh < 4; ++j) memcpy(h[j], h[j + sh], sizeof(h[j]));
                            for (int j = 4 - sh; j < 4; ++j) {
                                if (j > 0 && iy[j] == iy[j - 1]) {
                                    memcpy(h[j], h[j - 1], sizeof(h[j]));
                                } else if (in_x) {
                                    memcpy(stage, fin + ((int64_t)(g.sy0 + iy[j]) * g.in_w + lo) * g.in_c, sizeof(float) * (size_t)n);
                                    for (int ch = 0; ch < 3; ++ch) {
                                        float v[4];
                                        for (int i = 0; i < 4; ++i) v[i] = stage[ix[i] + ch];
                                        h[j][ch] = rs_dot<4>(wx, v);
                                    }
                                }
                            }
                            for (int j = 0; j < 4; ++j) hy[j] = iy[j];
                            if (in_x)
                                for (int ch = 0; ch < 3; ++ch) {
                                    float col[4];
                                    for (int j = 0; j < 4; ++j) col[j] = h[j][ch];
                                    val[ch] = clamp01(rs_dot<4>(wy, col));
                                }
                        }
                        const int64_t e = (((int64_t)z * g.out_h + oy) * g.out_w + c) * 3;
                        for (int ch = 0; ch < 3; ++ch) {
                            if (out_f32) out_f32[e + ch] = val[ch];
                            if (out_u8) out_u8[e + ch] = prep_byte(val[ch]);
                        }
                    }
                }
            }
    }
    delete[] stage;
}

uint8_t hm_prepare_byte(float v) { return prep_byte(v); }

}  // extern "C"
