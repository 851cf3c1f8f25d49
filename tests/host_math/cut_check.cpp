// Test scaffolding: the cut-score arithmetic of csrc/vrg_area_math.hpp on the host -- the header compiled with g++ (-ffp-contract=off):
// area_fill_cells makes the table, area_thumbnail / area_histogram / area_pair_sums evaluate everything straight from the definition.
// Checked value for value against the independent numpy restatement of tests/cut_support.py (tests/test_cut_host.py).  Never loaded by
// the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_area_math.hpp"

using namespace vrg;

extern "C" {

// cells: 128 x 20 bytes, columns first
void hm_area_taps(int32_t in_h, int32_t in_w, void* cells) { area_fill_cells(in_h, in_w, reinterpret_cast<AreaCell*>(cells)); }

int32_t hm_area_mode(int32_t in_h, int32_t in_w) { return area_mode(in_h, in_w); }

// in: [frames][h][w][c] fp32, out: [frames][64][64][3] bytes
void hm_cut_thumbs(const float* in, uint8_t* out, int64_t frames, int32_t h, int32_t w, int32_t c) {
    std::vector<AreaCell> cells(2 * AREA_OUT);
    area_fill_cells(h, w, cells.data());
    for (int64_t f = 0; f < frames; ++f) area_thumbnail(in + f * (int64_t)h * w * c, h, w, c, cells.data(), out + f * AREA_THUMB_BYTES);
}

// hist: int32 [frames][1024]
void hm_cut_hist(const uint8_t* thumbs, int32_t* hist, int64_t frames) {
    for (int64_t f = 0; f < frames; ++f) area_histogram(thumbs + f * AREA_THUMB_BYTES, hist + f * AREA_HIST_BINS);
}

// sums: int64 [frames - 1][4]
void hm_cut_pair_sums(const uint8_t* thumbs, const int32_t* hist, int64_t* sums, int64_t frames) {
    for (int64_t f = 0; f + 1 < frames; ++f)
        area_pair_sums(thumbs + f * AREA_THUMB_BYTES, thumbs + (f + 1) * AREA_THUMB_BYTES, hist + f * AREA_HIST_BINS, hist + (f + 1) * AREA_HIST_BINS,
                       sums + 4 * f);
}

// h, s of one byte pixel (the HSV step alone)
void hm_cut_hsv(int32_t r, int32_t g, int32_t b, int32_t* h, int32_t* s) { area_hsv_bin(r, g, b, area_sdiv, area_hdiv, h, s); }

}  // extern "C"
