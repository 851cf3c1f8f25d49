// Test scaffolding: the LTX MSR reference frames of csrc/vrg_msr_math.hpp on the host -- the header compiled with g++ (-ffp-contract=off):
// msr_frames_host is k_msr_tile's walk (tiles, strips planned by msr_plan_strip, slots, one conversion, a store per frame) in plain loops.
// Checked bit for bit against the independent numpy restatement of tests/lanczos_support.py (tests/test_msr_host.py).  With
// -DMSR_CHECK_MAIN it is a stand-alone program that walks geometries of its own -- enlarging, shrinking past 8, one-pixel sources, ragged
// tiles -- and holds every value to lz_pixel, the definition; built with the address and undefined-behaviour sanitizers by the same test.
// Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_msr_math.hpp"

using namespace vrg;

extern "C" {

int hm_msr_check(const vrg_msr_desc* desc, int64_t n_desc, int64_t n_taps, int64_t frames, int32_t out_h, int32_t out_w) {
    return msr_check(desc, n_desc, n_taps, frames, out_h, out_w);
}

// desc[i].src and taps are host pointers; out: [frames][out_h][out_w][3] floats
void hm_msr_frames(const vrg_msr_desc* desc, int64_t n_desc, const void* taps, float* out, int32_t out_h, int32_t out_w) {
    msr_frames_host(desc, n_desc, reinterpret_cast<const LzTap*>(taps), out, out_h, out_w);
}

// rows taken and slots used by the strips of one tile column of an axis: strips[2 * i], strips[2 * i + 1]; returns the strips
int32_t hm_msr_strips(int32_t in_h, int32_t out_h, int32_t y0, int32_t* strips) {
    std::vector<LzTap> taps((size_t)out_h);
    for (int32_t y = 0; y < out_h; ++y) taps[y] = lz_tap(y, in_h, out_h);
    const int32_t rows = out_h - y0 < MSR_TH ? out_h - y0 : MSR_TH;
    int32_t rs[MSR_TH], slot0[MSR_TH], srcrow[MSR_SLOTS], slots, count = 0;
    for (int32_t ly = 0; ly < rows; ++ly) rs[ly] = taps[y0 + ly].s;
    for (int32_t ly0 = 0; ly0 < rows; ++count) {
        const int32_t n = msr_plan_strip(rs, ly0, rows, in_h, slot0, srcrow, slots);
        strips[2 * count] = n;
        strips[2 * count + 1] = slots;
        ly0 += n;
    }
    return count;
}

}  // extern "C"

#ifdef MSR_CHECK_MAIN
static int run_case(int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h, int32_t repeats, uint32_t seed) {
    std::vector<uint8_t> src((size_t)in_w * in_h * 3 + 1);
    for (auto& b : src) {
        seed = seed * 1664525u + 1013904223u;
        b = (uint8_t)(seed >> 24);
    }
    const bool same = in_w == out_w && in_h == out_h;
    std::vector<LzTap> taps((size_t)out_w + out_h);
    lz_fill_taps(in_w, in_h, out_w, out_h, taps.data());
    vrg_msr_desc desc[3] = {};
    desc[0].src = src.data() + 1;                                             // an odd address
    desc[0].in_h = in_h; desc[0].in_w = in_w; desc[0].taps = same ? -1 : 0; desc[0].first_frame = 0; desc[0].repeats = repeats;
    desc[1] = desc[0];
    desc[1].first_frame = repeats; desc[1].repeats = 0;
    desc[2].taps = -1; desc[2].first_frame = repeats; desc[2].repeats = 1;
    desc[2].fill[0] = 9; desc[2].fill[1] = 127; desc[2].fill[2] = 250;
    const int64_t frames = repeats + 1, n_taps = (int64_t)taps.size();
    if (msr_check(desc, 3, n_taps, frames, out_h, out_w) != VRG_OK) return 1;
    desc[1].repeats = 1;                                                      // overlaps the fill
    if (msr_check(desc, 3, n_taps, frames, out_h, out_w) != VRG_ERR_BAD_ARG) return 2;
    desc[1].repeats = 0;
    const size_t per = (size_t)out_h * out_w * 3;
    std::vector<float> out((size_t)frames * per, -1.0f);
    msr_frames_host(desc, 3, taps.data(), out.data(), out_h, out_w);
    const uint8_t* pic = desc[0].src;
    auto load = [&](int32_t y, int32_t x, int c) { return pic[((int64_t)y * in_w + x) * 3 + c]; };
    for (int32_t y = 0; y < out_h; ++y)
        for (int32_t x = 0; x < out_w; ++x) {
            uint8_t o[3];
            lz_pixel(taps[x], taps[(size_t)out_w + y], in_w, in_h, load, o);
            for (int c = 0; c < 3; ++c) {
                const size_t at = ((size_t)y * out_w + x) * 3 + c;
                const float want = (float)(same ? load(y, x, c) : o[c]) / 255.0f;
                for (int32_t f = 0; f < repeats; ++f)
                    if (out[(size_t)f * per + at] != want) return 3;
                if (out[(size_t)repeats * per + at] != (float)desc[2].fill[c] / 255.0f) return 4;
            }
        }
    return 0;
}

int main() {
    static const int32_t cases[][5] = {{1, 1, 32, 32, 2},   {7, 5, 33, 5, 3},    {37, 53, 96, 64, 1}, {301, 203, 64, 96, 2}, {1024, 16, 32, 64, 1},
                                       {16, 1024, 70, 45, 1}, {65, 33, 65, 33, 2}, {3, 900, 5, 41, 1},  {200, 7, 130, 77, 1},  {50, 40, 49, 39, 1}};
    int bad = 0;
    for (const auto& c : cases) {
        const int rc = run_case(c[0], c[1], c[2], c[3], c[4], 12345u + (uint32_t)c[0]);
        if (rc) {
            printf("case %d x %d -> %d x %d: %d\n", c[0], c[1], c[2], c[3], rc);
            bad = 1;
        }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
