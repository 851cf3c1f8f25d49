// vrg_pil_resample.hpp -- Pillow's byte resampling, stated once for the far-face composite (csrc/vrg_farface.hip), the reference sheets
// (csrc/vrg_sheet.hip) and the contact sheet (csrc/vrg_thumb.hip), host and device.  Every rule is pinned against the installed Pillow,
// byte for byte (tests/test_far_face_host.py, tests/test_sheet_host.py, tests/test_contact_sheet_host.py).
//   resize (Resample.c)     Image.resize(size, filter, box) on RGB / L bytes.  Separable; the horizontal pass writes a rounded byte image,
//                           then the vertical pass runs; a pass is skipped only where out == in and the box is the whole axis.  Per axis,
//                           in double, for the source interval [in0, in1): scale = (in1 - in0) / out, fs = max(scale, 1),
//                           support = S fs (LANCZOS: S = 3, BICUBIC: S = 2), ksize = 2 ceil(support) + 1;  for output xx:
//                           c = in0 + (xx + 0.5) scale, xmin = max(int(c - support + 0.5), 0), xmax = min(int(c + support + 0.5), in),
//                           w_x = F((x + xmin - c + 0.5) / fs), divided by their sum in index order, then fixed to 22 bits:
//                           int(w 2^22 +- 0.5).  pixel = clip((2^21 + sum byte * k) >> 22, 0, 255).  LANCZOS: sinc(t) sinc(t / 3) on
//                           -3 <= t < 3.  BICUBIC: a = -0.5: ((a + 2) t - (a + 3)) t t + 1 for t < 1, (((t - 5) t + 8) t - 4) a for
//                           t < 2.  The tables are made on the HOST (pil_filter_table): no kernel evaluates a sine.
//   box                     A box reaches Pillow's C as `float`: in0, in1 are fp32 and in1 - in0 is taken in fp32 (pil_box_span).  A
//                           resize without a box is the whole axis, start 0 and span n_in, exact for every int32 n_in: the builder takes
//                           start and span as doubles, prepared by the caller.
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
//   shared kernel parts     a row segment staged in LDS at the phase of its address (pil_stage_bytes), and a canvas written as a flat run
//                           of 16-byte pieces (pil_flat_plan, pil_flat_write).
#pragma once
#include <stdint.h>

#include "vrg_pixel_math.hpp"

#include <math.h>

namespace vrg {

constexpr int PIL_PRECISION_BITS = 22;
constexpr int PIL_FILTER_LANCZOS = 1;     // Pillow's own numbers (Image.Resampling)
constexpr int PIL_FILTER_BICUBIC = 3;
constexpr int PIL_TALL_RATIO = 100;       // Image.resize goes vertically first beyond it

inline double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}

inline double pil_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? pil_sinc(x) * pil_sinc(x / 3) : 0.0; }

inline double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

inline bool pil_filter_known(int32_t filter) { return filter == PIL_FILTER_BICUBIC || filter == PIL_FILTER_LANCZOS; }
inline double pil_filter_support(int32_t filter) { return filter == PIL_FILTER_BICUBIC ? 2.0 : 3.0; }

// the length of a box as Pillow's C takes it: the difference of two floats, in float
inline double pil_box_span(float in0, float in1) { return (double)(in1 - in0); }

// HOST.  taps per output index of one axis: `span` source pixels (the whole axis: n_in) onto n_out outputs
inline int32_t pil_filter_ksize(int32_t filter, double span, int32_t n_out) {
    const double scale = span / n_out;
    return (int32_t)ceil(pil_filter_support(filter) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// HOST.  One axis of Image.resize(.., filter, box): n_out outputs from the source interval [start, start + span) of n_in pixels -- a box
// (in0, pil_box_span(in0, in1)), or the whole axis (0, n_in).  bounds: [n_out][2] (first source index, tap count); weights:
// [n_out][ksize], zero beyond the count.  The filter is chosen once, outside the tap loops (pil_filter_table).
template <class Kernel>
inline void pil_axis_table(Kernel kernel, double kernel_support, int32_t ksize, int32_t n_in, double start, double span, int32_t n_out,
                           int32_t* bounds, int32_t* weights) {
    const double scale = span / n_out, fs = scale < 1.0 ? 1.0 : scale, support = kernel_support * fs, ss = 1.0 / fs;
    double* k = new double[(size_t)ksize];
    for (int32_t xx = 0; xx < n_out; ++xx) {
        const double center = start + (xx + 0.5) * scale;
        int32_t xmin = (int32_t)(center - support + 0.5), xmax = (int32_t)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < xmax; ++x) {
            k[x] = kernel((x + xmin - center + 0.5) * ss);
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

inline void pil_filter_table(int32_t filter, int32_t n_in, double start, double span, int32_t n_out, int32_t* bounds, int32_t* weights) {
    const int32_t ksize = pil_filter_ksize(filter, span, n_out);
    if (filter == PIL_FILTER_BICUBIC) pil_axis_table(pil_bicubic, 2.0, ksize, n_in, start, span, n_out, bounds, weights);
    else pil_axis_table(pil_lanczos, 3.0, ksize, n_in, start, span, n_out, bounds, weights);
}

// HOST.  Image.resize(size, LANCZOS) without a box, under its earlier names: the one builder over the whole axis, no float in between
inline int32_t pil_lanczos_ksize(int32_t n_in, int32_t n_out) { return pil_filter_ksize(PIL_FILTER_LANCZOS, n_in, n_out); }
inline void pil_lanczos_table(int32_t n_in, int32_t n_out, int32_t* bounds, int32_t* weights) {
    pil_filter_table(PIL_FILTER_LANCZOS, n_in, 0.0, n_in, n_out, bounds, weights);
}

// record i of an axis table of n_out records (bounds, then weights): its first source index, its tap count, its weights, and whether it
// may be followed -- the count within ksize and every tap inside the sources [lo, hi).  What stands in for a record that may not is the
// caller's: 0 in the sheet and far-face passes, the canvas colour in the contact sheet, a refusal in the host checks.
struct PilRecord {
    int32_t first, n;
    const int32_t* w;
    bool ok;
};

VRG_HD PilRecord pil_record(const int32_t* table, int32_t n_out, int32_t i, int32_t ksize, int32_t lo, int32_t hi) {
    const int32_t first = table[2 * i], n = table[2 * i + 1];
    return PilRecord{first, n, table + 2 * (int64_t)n_out + (int64_t)i * ksize, first >= lo && n >= 0 && n <= ksize && first <= hi - n};
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

// the same over taps `pitch` bytes apart (a column of a byte image): tap i of channel c is at[i * pitch + c]
template <int C>
VRG_HD void pil_walk(const int32_t* w, int32_t n, const uint8_t* at, int64_t pitch, uint8_t* out) {
    pil_taps<C>(w, n, [&](int32_t i, int c) { return at[i * pitch + c]; }, out);
}

VRG_HD uint8_t pil_walk_byte(const int32_t* w, int32_t n, const uint8_t* at, int64_t pitch) {
    uint8_t o;
    pil_walk<1>(w, n, at, pitch, &o);
    return o;
}

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

// a canvas of `total` elements of `elem` bytes from `out`, written as a flat run of 16-byte pieces, one per thread: `lead` elements lie
// in front of the first 16-byte boundary of `out` (all of them, where the canvas ends before it), `pieces` whole pieces follow, and one
// thread more stores the elements off the grid.  false: more workgroups than a launch takes.
struct PilFlat {
    int64_t lead, pieces, blocks;
};

VRG_HD bool pil_flat_plan(const void* out, int64_t elem, int64_t total, int64_t threads, PilFlat& f) {
    f.lead = (int64_t)((16 - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / elem;
    f.lead = f.lead < total ? f.lead : total;
    f.pieces = (total - f.lead) / (16 / elem);
    f.blocks = (f.pieces + 1 + threads - 1) / threads;
    return f.blocks <= 0x7fffffffll;
}

}  // namespace vrg

#if defined(__HIPCC__) || defined(__HIP__)
namespace vrg {

typedef float pil_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t pil_u4 __attribute__((ext_vector_type(4)));

// n bytes from src into rb by the whole workgroup of `threads`: byte i lands at rb[ph + i], ph the returned phase (the address mod 16), so
// that the 16-byte non-temporal loads and the LDS words they fill are both aligned.  rb is 16-byte aligned and holds n + 32 bytes.
__device__ __forceinline__ int pil_stage_bytes(const uint8_t* src, int n, uint8_t* rb, int tid, int threads) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    int head = (16 - ph) & 15;
    head = head < n ? head : n;
    const int nq = (n - head) >> 4;
    if (tid < head) rb[ph + tid] = src[tid];
    const pil_u4* body = reinterpret_cast<const pil_u4*>(src + head);
    pil_u4* dst = reinterpret_cast<pil_u4*>(rb + ph + head);
    for (int q = tid; q < nq; q += threads) dst[q] = __builtin_nontemporal_load(body + q);
    const int t = head + 16 * nq + tid;                                        // at most 15 bytes behind the last 16-byte piece
    if (t < n) rb[ph + t] = src[t];
    return ph;
}

// thread t of the launch of pil_flat_plan: its piece in one non-temporal store (four floats or sixteen bytes), or -- the thread behind the
// last piece -- the elements off the grid one by one.  cur.seek(e) moves the cursor to element e of the canvas, cur.next() gives the byte
// there and steps to e + 1, cur.unit(byte) is the float of a byte (asked only of a float canvas).  Nothing of `out` is read.
template <typename O, class Cursor>
__device__ __forceinline__ void pil_flat_write(O* __restrict__ out, int64_t total, int64_t lead, int64_t pieces, int64_t t, Cursor cur) {
    constexpr int V = 16 / (int)sizeof(O);                                     // elements of a piece
    if (t < pieces) {
        const int64_t e0 = lead + t * V;
        cur.seek(e0);
        if constexpr (sizeof(O) == 4) {
            pil_f4 v;
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = cur.unit(cur.next());
            __builtin_nontemporal_store(v, reinterpret_cast<pil_f4*>(out + e0));
        } else {
            pil_u4 v = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < V; ++i) v[i >> 2] |= (uint32_t)cur.next() << (8 * (i & 3));
            __builtin_nontemporal_store(v, reinterpret_cast<pil_u4*>(out + e0));
        }
    } else if (t == pieces) {                                                  // fewer than 2 V elements
        const int64_t behind = lead + pieces * V;
        for (int64_t k = 0; k < lead + total - behind; ++k) {
            const int64_t e = k < lead ? k : behind + (k - lead);
            cur.seek(e);
            if constexpr (sizeof(O) == 4) out[e] = cur.unit(cur.next());
            else out[e] = cur.next();
        }
    }
}

}  // namespace vrg
#endif
