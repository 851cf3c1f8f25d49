// vrg_facefix_math.hpp -- arithmetic of the AI Video Builder's Face Fix composite (csrc/vrg_facefix.hip), host and device.
//
// What is restated: the per-pixel work of finalize_face_fix in the reference's VRGDG_FaceFix.py (:937-957) on decoded B,G,R bytes.
//   mask geometry (:884-888)   inset = max(2, int(round(min(w, h) * 0.035)))  -- Python round: half to even, on the double product
//                              axes = (max(1, w // 2 - inset), max(1, h // 2 - inset)), centre (w // 2, h // 2)
//   ellipse fill (:888)        cv2.ellipse(mask, centre, axes, 0, 0, 360, 1.0, -1) as a table of one inclusive span [x0, x1] per row (the
//                              shape is convex).  OpenCV 4.x restated from memory: EllipseEx picks delta (90 / 30 / 18 / 5 degrees) from
//                              the larger axis, ellipse2Poly walks the integer-degree sine table (fp32 entries of seven decimals) in
//                              16.16 fixed point and rounds every vertex half to even, FillConvexPoly draws the outline (Line2, clipped by
//                              clipLine) and fills between two 16.16 edges with rounding offsets of one half; the spans are then closed
//                              under the reflections about the centre column and row (the restated outline alone differs from its
//                              mirror image by single pixels at the ends of some rows).  HOST only: ff_ellipse_spans.
//                              No cv2 is at hand where this was written, so equality with cv2 is NOT pinned; everything downstream only
//                              reads the spans, and replacing this one function changes no kernel.
//   Gaussian (:890-893)        n = max(3, 4 * feather + 1) taps, sigma = max(0.1, feather);  t_i = exp(-(i - (n - 1) / 2)^2 / (2 sigma^2))
//                              in double, c_i = (float)(t_i / sum t) with the sum in double in index order.  HOST only: ff_gauss_coeffs.
//   blur (:893-894)            horizontal pass, then vertical pass, both fp32: taps in increasing index order, each product rounded, then
//                              added (no contraction); BORDER_REFLECT_101 repeated until the index is inside the plane (n may exceed the
//                              box); the horizontal plane is stored as fp32; then clip(0, 1).  The input is 0 / 1 and adding fl(c * 0)
//                              leaves an fp32 sum unchanged, so the horizontal pass adds the coefficients of the taps inside the span.
//                              feather == 0: the mask is the 0 / 1 spans.  cv2's own GaussianBlur arithmetic is NOT pinned either.
//   mean shift (:897-910)      active when strength > 0 and at least 16 pixels have alpha > 0.35 (fp32 compare): exact integer sums S of
//                              the selected bytes of both images, mean = (float)((double)S / (double)N),
//                              shift_c = fl(fl(tmean_c - smean_c) * (float)strength), byte = trunc(clip(fl((float)src + shift_c), 0, 255)).
//                              numpy's fp32 running mean equals the exact mean rounded once while N * 255 < 2^24 (N <= 65,793); beyond
//                              that this is the exact mean (the precedent of the fp32 composite), the reference drifts.
//   blend (:953-957)           a = fl(base_alpha * (float)composite_strength), v = fl(fl((float)target * fl(1.0f - a)) + fl((float)face * a)),
//                              byte = trunc(clip(v, 0, 255)).
// The resize of :949 is cv2's byte Lanczos-4 of vrg_lanczos_math.hpp, unchanged.
#pragma once
#include <stdint.h>

#include "vrg_pixel_math.hpp"

#include <math.h>

namespace vrg {

// one row of a mask: the filled pixels are x0 .. x1; x0 > x1 = none
struct FfSpan {
    int32_t x0, x1;
};
static_assert(sizeof(FfSpan) == 8, "FfSpan is two int32: the table layout of vrg_ff_ellipse_spans");

constexpr int FF_STAT_SUMS = 7;          // selected count, three sums of the face bytes, three of the original's
constexpr int FF_STATS_WORDS = 12;       // uint64 per frame: the seven sums, matched, the three fp32 shifts (+ one zero) in [8..9], two zeros
constexpr int FF_MIN_SELECTED = 16;

inline int32_t ff_gauss_taps(int32_t feather) { return 4 * feather + 1 < 3 ? 3 : 4 * feather + 1; }

inline void ff_mask_geometry(int32_t w, int32_t h, int32_t& cx, int32_t& cy, int32_t& ax, int32_t& ay) {
    int32_t inset = (int32_t)nearbyint((double)(w < h ? w : h) * 0.035);          // default rounding mode: half to even
    inset = inset < 2 ? 2 : inset;
    cx = w / 2;
    cy = h / 2;
    ax = w / 2 - inset < 1 ? 1 : w / 2 - inset;
    ay = h / 2 - inset < 1 ? 1 : h / 2 - inset;
}

inline void ff_gauss_coeffs(int32_t feather, float* c) {
    const int32_t n = ff_gauss_taps(feather);
    const double sigma = feather < 1 ? 0.1 : (double)feather;                      // max(0.1, feather) of an integer feather
    const double half = (double)(n - 1) / 2.0;
    double sum = 0.0;
    for (int32_t i = 0; i < n; ++i) sum += exp(-(((double)i - half) * ((double)i - half)) / (2.0 * sigma * sigma));
    for (int32_t i = 0; i < n; ++i) c[i] = (float)(exp(-(((double)i - half) * ((double)i - half)) / (2.0 * sigma * sigma)) / sum);
}

// ---- the ellipse rasteriser (host) ----------------------------------------------------------------------------------------------------
namespace ffdraw {

constexpr int SHIFT = 16;
constexpr int64_t ONE = (int64_t)1 << SHIFT;

struct Pt {
    int64_t x, y;
};

struct Canvas {
    int32_t w, h;
    FfSpan* rows;
    void put(int64_t x, int64_t y) const {
        if (x < 0 || x >= w || y < 0 || y >= h) return;
        FfSpan& s = rows[y];
        if (s.x0 > s.x1) s.x0 = s.x1 = (int32_t)x;
        else {
            if (x < s.x0) s.x0 = (int32_t)x;
            if (x > s.x1) s.x1 = (int32_t)x;
        }
    }
};

inline float sin_deg(int d) {            // the table entry: sin of an integer degree, seven decimals, as fp32
    return (float)(nearbyint(sin((double)d * (3.1415926535897932384626433832795 / 180.0)) * 1e7) / 1e7);
}

// Cohen-Sutherland in int64 on the 16.16 size
inline bool clip_line(int64_t width, int64_t height, Pt& p1, Pt& p2) {
    const int64_t right = width - 1, bottom = height - 1;
    if (width <= 0 || height <= 0) return false;
    int64_t &x1 = p1.x, &y1 = p1.y, &x2 = p2.x, &y2 = p2.y;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        int64_t a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// the outline of one polygon edge, both ends in 16.16
inline void line2(const Canvas& cv, Pt p1, Pt p2) {
    if (!clip_line((int64_t)cv.w << SHIFT, (int64_t)cv.h << SHIFT, p1, p2)) return;
    int64_t dx = p2.x - p1.x, dy = p2.y - p1.y;
    const int64_t j = dx < 0 ? -1 : 0, i = dy < 0 ? -1 : 0;
    const int64_t ax = (dx ^ j) - j, ay = (dy ^ i) - i;
    int64_t x_step, y_step;
    int64_t count;
    if (ax > ay) {
        dy = (dy ^ j) - j;
        if (j) { const Pt t = p1; p1 = p2; p2 = t; }
        x_step = ONE;
        y_step = (dy * ONE) / (ax | 1);
        count = (p2.x - p1.x) >> SHIFT;
    } else {
        dx = (dx ^ i) - i;
        if (i) { const Pt t = p1; p1 = p2; p2 = t; }
        x_step = (dx * ONE) / (ay | 1);
        y_step = ONE;
        count = (p2.y - p1.y) >> SHIFT;
    }
    p1.x += ONE >> 1;
    p1.y += ONE >> 1;
    cv.put((p2.x + (ONE >> 1)) >> SHIFT, (p2.y + (ONE >> 1)) >> SHIFT);
    if (ax > ay) {
        p1.x >>= SHIFT;
        for (; count >= 0; --count) {
            cv.put(p1.x, p1.y >> SHIFT);
            p1.x += 1;
            p1.y += y_step;
        }
    } else {
        p1.y >>= SHIFT;
        for (; count >= 0; --count) {
            cv.put(p1.x >> SHIFT, p1.y);
            p1.x += x_step;
            p1.y += 1;
        }
    }
}

inline void fill_convex_poly(const Canvas& cv, const Pt* v, int npts) {
    struct Edge {
        int idx, di;
        int64_t x, dx;
        int ye;
    } edge[2];
    const int64_t delta = ONE >> 1;
    int imin = 0, edges = npts;
    int64_t xmin = v[0].x, xmax = v[0].x, ymin = v[0].y, ymax = v[0].y;
    Pt p0 = v[npts - 1];
    for (int i = 0; i < npts; ++i) {
        const Pt p = v[i];
        if (p.y < ymin) {
            ymin = p.y;
            imin = i;
        }
        ymax = ymax > p.y ? ymax : p.y;
        xmax = xmax > p.x ? xmax : p.x;
        xmin = xmin < p.x ? xmin : p.x;
        line2(cv, p0, p);
        p0 = p;
    }
    xmin = (xmin + delta) >> SHIFT;
    xmax = (xmax + delta) >> SHIFT;
    ymin = (ymin + delta) >> SHIFT;
    ymax = (ymax + delta) >> SHIFT;
    if (npts < 3 || xmax < 0 || ymax < 0 || xmin >= cv.w || ymin >= cv.h) return;
    ymax = ymax < cv.h - 1 ? ymax : cv.h - 1;
    int y = (int)ymin;
    edge[0].idx = edge[1].idx = imin;
    edge[0].ye = edge[1].ye = y;
    edge[0].di = 1;
    edge[1].di = npts - 1;
    edge[0].x = edge[1].x = -ONE;
    edge[0].dx = edge[1].dx = 0;
    do {
        for (int i = 0; i < 2; ++i) {
            if (y >= edge[i].ye) {
                int idx0 = edge[i].idx;
                const int di = edge[i].di;
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    const int ty = (int)((v[idx].y + delta) >> SHIFT);
                    if (ty > y) {
                        const int64_t xs = v[idx0].x, xe = v[idx].x;
                        edge[i].ye = ty;
                        edge[i].dx = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                        edge[i].x = xs;
                        edge[i].idx = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            const int left = edge[0].x > edge[1].x ? 1 : 0, right = 1 - left;
            int64_t xx1 = (edge[left].x + delta) >> SHIFT, xx2 = (edge[right].x + delta) >> SHIFT;
            if (xx2 >= 0 && xx1 < cv.w) {
                xx1 = xx1 < 0 ? 0 : xx1;
                xx2 = xx2 >= cv.w ? cv.w - 1 : xx2;
                if (xx1 <= xx2) {
                    cv.put(xx1, y);
                    cv.put(xx2, y);
                }
            }
        }
        edge[0].x += edge[0].dx;
        edge[1].x += edge[1].dx;
    } while (++y <= (int)ymax);
}

}  // namespace ffdraw

// spans[h]: the filled ellipse of a w x h mask
inline void ff_ellipse_spans(int32_t w, int32_t h, FfSpan* spans) {
    using namespace ffdraw;
    for (int32_t y = 0; y < h; ++y) spans[y] = FfSpan{0, -1};
    int32_t cx, cy, ax, ay;
    ff_mask_geometry(w, h, cx, cy, ax, ay);
    const int64_t cx16 = (int64_t)cx << SHIFT, cy16 = (int64_t)cy << SHIFT, aw = (int64_t)ax << SHIFT, ah = (int64_t)ay << SHIFT;
    int delta = (int)(((aw > ah ? aw : ah) + (ONE >> 1)) >> SHIFT);
    delta = delta < 3 ? 90 : delta < 10 ? 30 : delta < 15 ? 18 : 5;
    const float alpha = sin_deg(450), beta = sin_deg(0);                          // cos and sin of the ellipse's rotation, 0 degrees
    Pt v[80];
    int n = 0;
    for (int i = 0; i < 360 + delta; i += delta) {
        const int angle = i > 360 ? 360 : i;
        const double x = (double)aw * sin_deg(450 - angle), y = (double)ah * sin_deg(angle);
        const double px = (double)cx16 + x * alpha - y * beta, py = (double)cy16 + x * beta + y * alpha;
        const Pt pt{(int64_t)nearbyint(px), (int64_t)nearbyint(py)};
        if (n == 0 || pt.x != v[n - 1].x || pt.y != v[n - 1].y) v[n++] = pt;
    }
    if (n == 1) {
        v[0] = v[1] = Pt{cx16, cy16};
        n = 2;
    }
    fill_convex_poly(Canvas{w, h, spans}, v, n);
    // Close the spans under the two reflections the centre allows (columns 2 cx - x, rows 2 cy - y, where they lie inside the plane).  The
    // polygon is symmetric about the centre and so is the fill; the outline as restated is not: Line2 walks an edge from its left (upper)
    // end and samples the minor coordinate at offsets from THAT end, so an edge and its mirror image can differ by one pixel at the end of
    // a row.  Every span holds the centre column, so the union of a span and a mirror image is again one span.
    for (int32_t y = 0; y < h; ++y) {
        FfSpan& s = spans[y];
        if (s.x0 > s.x1) continue;
        const int32_t lo = 2 * cx - s.x1 < 0 ? 0 : 2 * cx - s.x1, hi = 2 * cx - s.x0 > w - 1 ? w - 1 : 2 * cx - s.x0;
        if (lo > hi) continue;
        s.x0 = s.x0 < lo ? s.x0 : lo;
        s.x1 = s.x1 > hi ? s.x1 : hi;
    }
    for (int32_t y = 0; y < h; ++y) {
        const int32_t my = 2 * cy - y;
        if (my <= y || my >= h) continue;
        FfSpan &a = spans[y], &b = spans[my];
        if (a.x0 > a.x1) a = b;
        else if (b.x0 <= b.x1) {
            a.x0 = a.x0 < b.x0 ? a.x0 : b.x0;
            a.x1 = a.x1 > b.x1 ? a.x1 : b.x1;
        }
        b = a;
    }
}

// ---- the passes the kernels and the host check share -----------------------------------------------------------------------------------
VRG_HD int32_t ff_reflect101(int32_t i, int32_t n) {
    if ((uint32_t)i < (uint32_t)n) return i;
    if (n == 1) return 0;
    const int32_t p = 2 * (n - 1);
    int32_t m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - m;
}

// horizontal pass at column x of a row whose filled pixels are `s`
VRG_HD float ff_blur_h(const float* c, int32_t n, FfSpan s, int32_t w, int32_t x) {
    const int32_t r = (n - 1) / 2;
    float acc = 0.0f;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t src = ff_reflect101(x + i - r, w);
        if (src >= s.x0 && src <= s.x1) acc = acc + c[i];
    }
    return acc;
}

// vertical pass at row y: load(row) = the horizontal plane's value in this column
template <typename LOAD>
VRG_HD float ff_blur_v(const float* c, int32_t n, int32_t h, int32_t y, LOAD load) {
    const int32_t r = (n - 1) / 2;
    float acc = 0.0f;
    for (int32_t j = 0; j < n; ++j) {
        const float p = c[j] * load(ff_reflect101(y + j - r, h));
        acc = acc + p;
    }
    return acc < 0.0f ? 0.0f : (acc > 1.0f ? 1.0f : acc);
}

VRG_HD bool ff_selected(float alpha) { return alpha > 0.35f; }

// sums: count, face B G R, original B G R
VRG_HD bool ff_shifts(const uint64_t (&sums)[FF_STAT_SUMS], float strength, float (&shift)[3]) {
    shift[0] = shift[1] = shift[2] = 0.0f;
    if (!(strength > 0.0f) || sums[0] < (uint64_t)FF_MIN_SELECTED) return false;
    const double n = (double)sums[0];
    for (int c = 0; c < 3; ++c) {
        const float smean = (float)((double)sums[1 + c] / n), tmean = (float)((double)sums[4 + c] / n);
        const float d = tmean - smean;
        shift[c] = d * strength;
    }
    return true;
}

// the last five words of a frame's FF_STATS_WORDS record from its seven sums: matched, the three fp32 shifts
VRG_HD void ff_finish_record(unsigned long long* rec, float color_match) {
    uint64_t sums[FF_STAT_SUMS];
    for (int i = 0; i < FF_STAT_SUMS; ++i) sums[i] = rec[i];
    float shift[3];
    const bool matched = ff_shifts(sums, color_match, shift);
    rec[7] = matched ? 1ull : 0ull;
    rec[8] = (unsigned long long)f32_bits(shift[0]) | ((unsigned long long)f32_bits(shift[1]) << 32);
    rec[9] = (unsigned long long)f32_bits(shift[2]);
}

// ... and read back: -> matched
VRG_HD bool ff_read_record(const unsigned long long* rec, float (&shift)[3]) {
    const unsigned long long a = rec[8], b = rec[9];
    shift[0] = f32_from_bits((uint32_t)a);
    shift[1] = f32_from_bits((uint32_t)(a >> 32));
    shift[2] = f32_from_bits((uint32_t)b);
    return rec[7] != 0ull;
}

VRG_HD uint8_t ff_trunc_byte(float v) {
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (uint8_t)(int32_t)v;
}

VRG_HD uint8_t ff_shift_byte(uint8_t face, float shift) { return ff_trunc_byte((float)face + shift); }

VRG_HD uint8_t ff_blend_byte(uint8_t target, uint8_t face, float base_alpha, float strength) {
    const float a = base_alpha * strength;
    const float ia = 1.0f - a;
    const float t = (float)target * ia, f = (float)face * a;
    return ff_trunc_byte(t + f);
}

}  // namespace vrg
