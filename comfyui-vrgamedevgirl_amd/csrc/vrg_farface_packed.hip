// vrg_farface_packed.hip -- the far-face repair composite (csrc/vrg_farface.hip) for frames that live on the host: only the boxes cross
// the bus.  gfx950 only.  What a workgroup does to a chunk of the means and to a byte of the paste, and which records it may follow:
// csrc/vrg_farface_body.hpp, the body of the whole-frame kernels, called with other addresses; where it works: csrc/vrg_packed_tiles.hpp,
// the tile map of both packed routes.
//
// Shape of the work.  The host gathers every box into one packed buffer ([box_h][box_w][3] blocks back to back) and uploads it with the
// repaired crops; the resize and the masks are the launches of csrc/vrg_farface.hip, which work on packed buffers already.  Two kernels
// touch the originals, and both grids are one-dimensional:
//   k_np_packed_means    one workgroup per record: np_means_block on the record's dense block (pixel p at src_offset + 3 p).
//   k_pil_packed_paste   one workgroup per tile of VRG_PIL_PACKED_TILE box pixels, found in the prefix table (packed_tile_pixel); a pixel's three
//                        bytes read from the box's block, pasted under the mask (pil_face_byte) and written to the block of the packed
//                        result.  A record that may not be pasted copies its block.
// Tile size: 256 pixels, one per lane of a 256-thread workgroup, as the Builder's packed route.  The reasoning, not a sweep: the
// smallest box of the tool (32 x 32) is then 4 workgroups and 64 boxes of 128 x 128 are 4096, more than the 256 CUs hold at once, so
// the launch is spread over the chip at every size it meets; a pixel is three byte loads, a mask byte and three stores, so nothing is
// gained by giving a lane more of them, and a larger tile would only leave small boxes on fewer CUs.  Both launches are latency-bound
// on a few hundred KB; nothing here is tuned.
#include "vrg_farface_body.hpp"

namespace vrg {

__global__ __launch_bounds__(256) void k_np_packed_means(const uint8_t* __restrict__ src, const uint8_t* __restrict__ repaired,
                                                          const uint8_t* __restrict__ masks, const vrg_pil_packed_desc* __restrict__ desc,
                                                          uint32_t* __restrict__ stats, PilpGeom g, float strength) {
    const int64_t i = blockIdx.x;                                         // < n: the grid is n
    const vrg_pil_packed_desc d = desc[i];                                // uniform
    uint32_t* rec = stats + i * PIL_STATS_WORDS;
    if (!packed_src_ok(d, g.src_bytes) || !pilp_blend_ok(d, g) || !d.color_match) {
        if (threadIdx.x < PIL_STATS_WORDS) rec[threadIdx.x] = 0u;
        return;
    }
    np_means_block(PilDenseOrig{src + d.src_offset}, repaired + d.rep_offset, masks + d.mask_offset, packed_box_pixels(d), strength, rec);
}

__global__ __launch_bounds__(256) void k_pil_packed_paste(const uint8_t* __restrict__ src, const uint8_t* __restrict__ repaired,
                                                           const uint8_t* __restrict__ masks, const vrg_pil_packed_desc* __restrict__ desc,
                                                           const int64_t* __restrict__ prefix, const uint32_t* __restrict__ stats,
                                                           uint8_t* __restrict__ out, PilpGeom g) {
    int64_t rec, p;
    vrg_pil_packed_desc d;                                                // workgroup-uniform
    const auto admits = [&](const vrg_pil_packed_desc& r) { return packed_blocks_ok(r, g.src_bytes, g.out_bytes); };  // else nowhere to read or to write
    if (!packed_tile_pixel(desc, prefix, g.n, admits, rec, d, p) || p < 0) return;
    uint8_t o[3];
    packed_pixel_load(src, d.src_offset, p, o);
    if (pilp_blend_ok(d, g)) {
        float shift[3] = {0.0f, 0.0f, 0.0f};
        const bool matched = d.color_match && pil_read_shift(stats + rec * PIL_STATS_WORDS, shift);
        const uint8_t m = masks[d.mask_offset + p];
        const uint8_t* face = repaired + d.rep_offset + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = pil_face_byte(o[c], face[c], matched, shift[c], m);
    }
    packed_pixel_store(out, d.dst_offset, p, o);
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_pil_packed_check(const vrg_pil_packed_desc* desc_host, int64_t n, const int64_t* tile_prefix_host, int64_t src_bytes,
                         int64_t rep_bytes, int64_t mask_bytes, int64_t out_bytes) {
    if (!packed_sizes_ok({n, src_bytes, rep_bytes, mask_bytes, out_bytes})) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!desc_host || !tile_prefix_host) return VRG_ERR_BAD_ARG;
    const PilpGeom g{n, src_bytes, rep_bytes, mask_bytes, out_bytes};
    for (int64_t i = 0; i < n; ++i)
        if (!packed_blocks_ok(desc_host[i], src_bytes, out_bytes) || !pilp_blend_ok(desc_host[i], g)) return VRG_ERR_BAD_ARG;
    const auto tiles_of = [&](int64_t i) { return packed_tiles(packed_box_pixels(desc_host[i])); };
    return tile_prefix_ok(n, tile_prefix_host, tiles_of) ? VRG_OK : VRG_ERR_BAD_ARG;
}

int vrg_np_packed_masked_means_f32(const uint8_t* src, int64_t src_bytes, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks,
                                   int64_t mask_bytes, const vrg_pil_packed_desc* desc, uint32_t* stats, int64_t n, float strength,
                                   void* stream) {
    if (!packed_sizes_ok({n, src_bytes, rep_bytes, mask_bytes})) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!src || !repaired || !masks || !desc || !stats || (reinterpret_cast<uintptr_t>(stats) & 3u) != 0) return VRG_ERR_BAD_ARG;
    if (n > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const PilpGeom g{n, src_bytes, rep_bytes, mask_bytes, 0};
    hipLaunchKernelGGL(k_np_packed_means, dim3((uint32_t)n), dim3(256), 0, (hipStream_t)stream, src, repaired, masks, desc, stats, g, strength);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_pil_packed_paste_u8(const uint8_t* src, int64_t src_bytes, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks,
                            int64_t mask_bytes, const vrg_pil_packed_desc* desc, const int64_t* tile_prefix, int64_t n, int64_t tiles,
                            const uint32_t* stats, uint8_t* out, int64_t out_bytes, void* stream) {
    if (!packed_sizes_ok({n, src_bytes, rep_bytes, mask_bytes, out_bytes}) || tiles < 0) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!src || !repaired || !masks || !desc || !tile_prefix || (reinterpret_cast<uintptr_t>(tile_prefix) & 7u) != 0 || !stats ||
        (reinterpret_cast<uintptr_t>(stats) & 3u) != 0 || !out || out == src || out == repaired || out == masks)
        return VRG_ERR_BAD_ARG;
    if (tiles > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    if (tiles == 0) return VRG_OK;
    const PilpGeom g{n, src_bytes, rep_bytes, mask_bytes, out_bytes};
    hipLaunchKernelGGL(k_pil_packed_paste, dim3((uint32_t)tiles), dim3(256), 0, (hipStream_t)stream, src, repaired, masks, desc, tile_prefix,
                       stats, out, g);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
