// Test scaffolding: csrc/vrg_facefix_body.hpp on the host -- the header compiled with g++ (-ffp-contract=off): one box through the shared
// bodies of the Builder's Face Fix, exactly as the kernels of csrc/vrg_facefix.hip and csrc/vrg_facefix_packed.hip call them, under the
// addressing the caller names: the box's first byte and the pixels from one of its rows to the next (the frame's width for a box inside
// a frame, box_w for a dense block).  The workgroup's sums and atomics are plain additions here, tile by tile
// (tests/test_facefix_packed_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_facefix_packed_math.hpp"

using namespace vrg;

extern "C" {

// box: [box_h] rows of `pitch` pixels; enhanced [enh_h][enh_w][3]; mask [box_h][box_w].  Out: crop [size][size][3], resized and out
// [box_h][box_w][3], sums: count, face B G R, original B G R (zeros when color_match <= 0: nothing is measured)
void hm_ffb_box(const uint8_t* box, int32_t pitch, int32_t box_w, int32_t box_h, const uint8_t* enhanced, int32_t enh_h, int32_t enh_w,
                const float* mask, float color_match, float strength, int32_t size, uint8_t* crop, uint8_t* resized, int64_t* sums,
                uint8_t* out) {
    std::vector<LzTap> taps((size_t)size * 2);
    lz_fill_taps(box_w, box_h, size, size, taps.data());
    for (int32_t y = 0; y < size; ++y)
        for (int32_t x = 0; x < size; ++x) ff_crop_pixel(box, pitch, box_w, box_h, taps[x], taps[size + y], crop + ((size_t)y * size + x) * 3);

    taps.resize((size_t)box_w + box_h);
    lz_fill_taps(enh_w, enh_h, box_w, box_h, taps.data());
    const int32_t measure = color_match > 0.0f ? 1 : 0;
    const int64_t n = (int64_t)box_w * box_h;
    unsigned long long rec[FF_STATS_WORDS] = {};
    for (int64_t p0 = 0; p0 < n; p0 += FFP_TILE) {                       // one workgroup
        uint32_t tile[FF_STAT_SUMS] = {};
        for (int64_t p = p0; p < n && p < p0 + FFP_TILE; ++p) {           // one lane
            const int32_t dy = (int32_t)(p / box_w), dx = (int32_t)(p - (int64_t)dy * box_w);
            uint32_t acc[FF_STAT_SUMS] = {};
            ff_resize_pixel(enhanced, enh_h, enh_w, taps[dx], taps[box_w + dy], resized + p * 3, mask + p, box + ((int64_t)dy * pitch + dx) * 3,
                            measure, acc);
            for (int i = 0; i < FF_STAT_SUMS; ++i) tile[i] += acc[i];
        }
        for (int i = 0; i < FF_STAT_SUMS; ++i) rec[i] += tile[i];
    }
    for (int i = 0; i < FF_STAT_SUMS; ++i) sums[i] = (int64_t)rec[i];
    if (measure) ff_finish_record(rec, color_match);

    float shift[3];
    const bool matched = ff_read_record(rec, shift);
    for (int64_t p = 0; p < n; ++p) {
        const int32_t dy = (int32_t)(p / box_w), dx = (int32_t)(p - (int64_t)dy * box_w);
        for (int c = 0; c < 3; ++c)
            out[p * 3 + c] = ff_composite_byte(box[((int64_t)dy * pitch + dx) * 3 + c], resized[p * 3 + c], matched, shift[c], mask[p], strength);
    }
}

}  // extern "C"
