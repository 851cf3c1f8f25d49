// Test scaffolding: csrc/vrg_pil_math.hpp on the host -- the header compiled with g++ (-ffp-contract=off): the Lanczos tables and the two
// byte passes of the resize, the box parameters and the six box passes of the mask through prefix sums, numpy's sequential fp32 means in
// the plain form (np_walk) and in the parallel form the kernel uses (maps of NP_RUN pixels, reduced pairwise per NP_CHUNK), and the paste.
// Checked against installed Pillow / numpy and the restatement of tests/far_face_support.py (tests/test_far_face_host.py), byte for byte.
// Also the host side of csrc/vrg_byte_mover.hpp and csrc/vrg_common.hpp: the movers' hit test, span_fits and the chunked launcher
// (tests/test_byte_movers_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_byte_mover.hpp"
#include "vrg_pil_math.hpp"

using namespace vrg;

template <int C>
static void resize_c(const uint8_t* in, int32_t in_h, int32_t in_w, uint8_t* out, int32_t out_h, int32_t out_w) {
    std::vector<uint8_t> tmp;
    const uint8_t* src = in;
    if (in_w != out_w) {
        const int32_t k = pil_filter_ksize(PIL_FILTER_LANCZOS, in_w, out_w);
        std::vector<int32_t> b((size_t)out_w * 2), w((size_t)out_w * k);
        pil_filter_table(PIL_FILTER_LANCZOS, in_w, 0.0, in_w, out_w, b.data(), w.data());
        tmp.resize((size_t)in_h * out_w * C);
        for (int32_t y = 0; y < in_h; ++y)
            for (int32_t x = 0; x < out_w; ++x) {
                const uint8_t* row = in + ((size_t)y * in_w + b[2 * x]) * C;
                pil_taps<C>(w.data() + (size_t)x * k, b[2 * x + 1], [&](int32_t i, int c) { return row[(size_t)i * C + c]; },
                            tmp.data() + ((size_t)y * out_w + x) * C);
            }
        src = tmp.data();
    }
    if (in_h == out_h) {
        memcpy(out, src, (size_t)out_h * out_w * C);
        return;
    }
    const int32_t k = pil_filter_ksize(PIL_FILTER_LANCZOS, in_h, out_h);
    std::vector<int32_t> b((size_t)out_h * 2), w((size_t)out_h * k);
    pil_filter_table(PIL_FILTER_LANCZOS, in_h, 0.0, in_h, out_h, b.data(), w.data());
    for (int32_t y = 0; y < out_h; ++y)
        for (int32_t x = 0; x < out_w; ++x) {
            const uint8_t* col = src + ((size_t)b[2 * y] * out_w + x) * C;
            pil_taps<C>(w.data() + (size_t)y * k, b[2 * y + 1], [&](int32_t i, int c) { return col[(size_t)i * out_w * C + c]; },
                        out + ((size_t)y * out_w + x) * C);
        }
}

static void box_line(std::vector<uint8_t>& line, const PilBox& b) {
    const int32_t n = (int32_t)line.size();
    std::vector<uint32_t> pre((size_t)n + 1, 0u);
    for (int32_t i = 0; i < n; ++i) pre[i + 1] = pre[i] + line[i];
    std::vector<uint8_t> out((size_t)n);
    for (int32_t x = 0; x < n; ++x)
        out[x] = pil_box_pixel(x, n, b, [&](int32_t i) { return pre[i]; }, [&](int32_t i) { return line[i]; });
    line.swap(out);
}

// the kernel's order: maps of NP_RUN consecutive values, reduced pairwise over NP_CHUNK, applied or walked
static uint64_t sum_parallel(const std::vector<uint8_t>& v) {
    uint64_t acc = 0;
    const size_t n = v.size();
    for (size_t base = 0; base < n; base += NP_CHUNK) {
        const uint32_t sh = np_ulp_shift(acc);
        const int32_t len = (int32_t)(n - base < (size_t)NP_CHUNK ? n - base : (size_t)NP_CHUNK);
        NpMap maps[256];
        for (int t = 0; t < 256; ++t) {
            maps[t].d[0] = maps[t].d[1] = 0u;
            for (int e = 0; e < NP_RUN; ++e) {
                const int32_t i = t * NP_RUN + e;
                if (i < len) np_map_push(maps[t], v[base + i], sh);
            }
        }
        for (int s = 1; s < 256; s *= 2)
            for (int t = 0; t + s < 256; t += 2 * s) maps[t] = np_map_then(maps[t], maps[t + s], sh);
        if (!np_apply(acc, maps[0], sh)) acc = np_walk(acc, v.data() + base, len, 1);
    }
    return acc;
}

extern "C" {

int32_t hm_pil_ksize(int32_t n_in, int32_t n_out) { return pil_filter_ksize(PIL_FILTER_LANCZOS, n_in, n_out); }

void hm_pil_table(int32_t n_in, int32_t n_out, int32_t* bounds, int32_t* weights) { pil_filter_table(PIL_FILTER_LANCZOS, n_in, 0.0, n_in, n_out, bounds, weights); }

void hm_pil_resize(const uint8_t* in, int32_t in_h, int32_t in_w, int32_t channels, uint8_t* out, int32_t out_h, int32_t out_w) {
    if (channels == 3) resize_c<3>(in, in_h, in_w, out, out_h, out_w);
    else resize_c<1>(in, in_h, in_w, out, out_h, out_w);
}

void hm_pil_box(float sigma, int32_t* out) {
    const PilBox b = pil_box_parameters(sigma);
    out[0] = b.r;
    out[1] = (int32_t)b.ww;
    out[2] = (int32_t)b.fw;
}

// spans [height][2] -> mask [height][width] = soft_face_mask((width, height), feather)
void hm_pil_mask(const int32_t* spans, int32_t width, int32_t height, int32_t feather, uint8_t* mask) {
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) mask[(size_t)y * width + x] = (x >= spans[2 * y] && x <= spans[2 * y + 1]) ? 255 : 0;
    if (feather <= 0) return;
    const PilBox b = pil_box_parameters((float)feather);
    for (int32_t y = 0; y < height; ++y) {
        std::vector<uint8_t> line(mask + (size_t)y * width, mask + (size_t)(y + 1) * width);
        for (int pass = 0; pass < 3; ++pass) box_line(line, b);
        memcpy(mask + (size_t)y * width, line.data(), (size_t)width);
    }
    for (int32_t x = 0; x < width; ++x) {
        std::vector<uint8_t> line((size_t)height);
        for (int32_t y = 0; y < height; ++y) line[y] = mask[(size_t)y * width + x];
        for (int pass = 0; pass < 3; ++pass) box_line(line, b);
        for (int32_t y = 0; y < height; ++y) mask[(size_t)y * width + x] = line[y];
    }
}

// original, repaired: [n][3]; mask [n]; stats: PIL_STATS_WORDS uint32
void hm_pil_means(const uint8_t* original, const uint8_t* repaired, const uint8_t* mask, int64_t n, int32_t parallel, uint32_t* stats) {
    uint32_t count = 0;
    uint64_t sums[6];
    std::vector<uint8_t> v((size_t)n);
    for (int64_t p = 0; p < n; ++p) count += mask[p] >= PIL_SELECT_FROM ? 1u : 0u;
    for (int k = 0; k < 6; ++k) {
        const uint8_t* src = k < 3 ? original + k : repaired + (k - 3);
        for (int64_t p = 0; p < n; ++p) v[(size_t)p] = mask[p] >= PIL_SELECT_FROM ? src[p * 3] : 0;
        sums[k] = parallel ? sum_parallel(v) : np_walk(0, v.data(), (int32_t)n, 1);
    }
    np_finish(count, sums, 0.65f, stats);
}

// the box of one frame: shifted (stats of hm_pil_means) when `shifted`, then pasted under the mask
void hm_pil_paste(const uint8_t* original, const uint8_t* repaired, const uint8_t* mask, int64_t n, int32_t shifted, const uint32_t* stats,
                  uint8_t* out) {
    const bool matched = shifted && stats[10] != 0u;
    for (int64_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c) {
            uint8_t r = repaired[p * 3 + c];
            if (matched) r = pil_shift_byte(r, f32_from_bits(stats[7 + c]));
            out[p * 3 + c] = pil_paste_byte(original[p * 3 + c], r, mask[p]);
        }
}

int32_t hm_byte_piece_hits(int32_t left, int32_t top, int32_t box_w, int32_t box_h, int32_t W, int32_t r) {
    return byte_piece_hits(left, top, box_w, box_h, W, r) ? 1 : 0;
}

int32_t hm_span_fits(int64_t offset, int64_t need, int64_t size) { return span_fits(offset, need, size) ? 1 : 0; }

// launch_chunks over n records with a callable that records (first, count) and returns `code` on its call number `fail_call` (from 1; 0 = never)
int32_t hm_launch_chunks(int64_t n, int32_t fail_call, int32_t code, int64_t* chunks, int32_t capacity, int32_t* calls) {
    *calls = 0;
    return launch_chunks(n, [&](int64_t first, int64_t count) {
        if (*calls < capacity) {
            chunks[2 * *calls] = first;
            chunks[2 * *calls + 1] = count;
        }
        return ++*calls == fail_call ? code : (int)VRG_OK;
    });
}

// the aligned form: every chunk starts on a multiple of `align`
int32_t hm_launch_chunks_aligned(int64_t n, int64_t align, int64_t* chunks, int32_t capacity, int32_t* calls) {
    *calls = 0;
    return launch_chunks(n, align, [&](int64_t first, int64_t count) {
        if (*calls < capacity) {
            chunks[2 * *calls] = first;
            chunks[2 * *calls + 1] = count;
        }
        ++*calls;
        return (int)VRG_OK;
    });
}

int64_t hm_chunk_lcm(int64_t a, int64_t b) { return chunk_lcm(a, b); }

}  // extern "C"
