// Test scaffolding: csrc/vrg_farface_body.hpp on the host -- the header compiled with g++ (-ffp-contract=off): the per-chunk means body
// the whole-frame and the packed kernels share (np_lane_fold, np_maps_merge, np_chunk_end, with a loop where the kernels have 256 lanes
// and barriers) under both addressings, the paste byte, and the packed route's tile placement (tests/test_far_face_packed_host.py).
// Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_farface_body.hpp"

using namespace vrg;

// np_means_block with the workgroup spelled out: every lane's fold, the in-order tree, one lane per sum at the end of the chunk
template <class Orig>
static void means_block(const Orig& orig, const uint8_t* rep, const uint8_t* mask, int64_t n, float strength, uint32_t* rec) {
    std::vector<uint8_t> stage_bytes((size_t)6 * NP_CHUNK);
    uint8_t (*stage)[NP_CHUNK] = reinterpret_cast<uint8_t (*)[NP_CHUNK]>(stage_bytes.data());
    std::vector<NpMap> map_cells((size_t)256 * 6);
    NpMap (*maps)[6] = reinterpret_cast<NpMap (*)[6]>(map_cells.data());
    uint64_t acc[6] = {0, 0, 0, 0, 0, 0};
    uint32_t count = 0;
    for (int64_t base = 0; base < n; base += NP_CHUNK) {
        uint32_t sh[6];
        for (int k = 0; k < 6; ++k) sh[k] = np_ulp_shift(acc[k]);
        for (int32_t t = 0; t < 256; ++t) count += np_lane_fold(orig, rep, mask, n, base, t, sh, stage, maps[t]);
        for (int32_t s = 1; s < 256; s <<= 1)
            for (int32_t t = 0; t < 256; ++t)
                if ((t & (2 * s - 1)) == 0) np_maps_merge(maps, t, s, sh);
        for (int k = 0; k < 6; ++k) acc[k] = np_chunk_end(acc[k], maps[0][k], stage[k], np_chunk_len(n, base));
    }
    np_finish(count, acc, strength, rec);
}

extern "C" {

// a dense block: original, repaired [n][3]; mask [n]; stats: PIL_STATS_WORDS uint32
void hm_pilp_means(const uint8_t* original, const uint8_t* repaired, const uint8_t* mask, int64_t n, uint32_t* stats) {
    means_block(PilDenseOrig{original}, repaired, mask, n, 0.65f, stats);
}

// the same box inside a frame of W pixels a row: `first` = the box's first pixel
void hm_pil_means_framed(const uint8_t* first, int32_t box_w, int32_t W, const uint8_t* repaired, const uint8_t* mask, int64_t n, uint32_t* stats) {
    means_block(PilFrameOrig{first, box_w, W}, repaired, mask, n, 0.65f, stats);
}

// the pixels of a dense block as k_pil_packed_paste makes them from a record of the means
void hm_pilp_paste(const uint8_t* original, const uint8_t* repaired, const uint8_t* mask, int64_t n, int32_t color_match, const uint32_t* stats,
                   uint8_t* out) {
    float shift[3] = {0.0f, 0.0f, 0.0f};
    const bool matched = color_match && pil_read_shift(stats, shift);
    for (int64_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c) out[p * 3 + c] = pil_face_byte(original[p * 3 + c], repaired[p * 3 + c], matched, shift[c], mask[p]);
}

// the tile map of csrc/vrg_packed_tiles.hpp, as k_pil_packed_paste calls it
int64_t hm_pilp_tiles(int32_t box_w, int32_t box_h) { return packed_tiles(packed_box_pixels(box_w, box_h)); }

// out: p0, count; -> 1 when `tile` is one of the record's
int32_t hm_pilp_place(int32_t box_w, int32_t box_h, int64_t first_tile, int64_t tile, int64_t* out) {
    int64_t p0 = -1;
    int32_t count = -1;
    const bool ok = tile_place(packed_box_pixels(box_w, box_h), first_tile, tile, p0, count);
    out[0] = p0;
    out[1] = count;
    return ok ? 1 : 0;
}

}  // extern "C"
