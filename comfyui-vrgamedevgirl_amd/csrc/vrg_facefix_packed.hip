// vrg_facefix_packed.hip -- the Builder's Face Fix (csrc/vrg_facefix.hip) for frames that live on the host: only the boxes cross the bus.
// gfx950 only.  Where a workgroup works: csrc/vrg_packed_tiles.hpp, the tile map of both packed routes; which records it follows:
// csrc/vrg_facefix_packed_math.hpp; what it does to a pixel, a byte and its sums is csrc/vrg_facefix_body.hpp, the body of the whole-frame
// kernels, called with other addresses.
//
// Shape of the work.  The host gathers every box into one packed buffer ([box_h][box_w][3] blocks back to back) and uploads it with the
// records and their tile prefix; the results come back packed the same way.  Each grid is one-dimensional.
//   k_ffp_lanczos        prepare: thread = one output pixel of one record, lz_pixel on the box's block (row pitch = box_w, so the taps clamp
//                        to the box by construction).  Every record has out_h * out_w pixels: the workgroup index divides into
//                        (record, part); no table.
//   k_ffp_resize_stats   finalize, first half: workgroup = one tile of 256 box pixels, found in the prefix table (packed_tile_pixel).  The repaired
//                        frame resized to the box into the byte scratch; with colour matching the selected count and six byte sums: lane
//                        values -> wave butterfly -> LDS -> one 64-bit integer atomic per sum and workgroup, as k_ff_resize_stats.
//                        The means and shifts of every record follow on the device: k_ff_finish of csrc/vrg_facefix.hip (ff_stats_end).
//   k_ffp_composite      finalize, second half: the same tiles; a pixel's three bytes read from the box's block, shifted, blended under
//                        the mask and written to the block of the packed result.  A record that may not be blended copies its block.
// All three are tap- or latency-bound on a few hundred KB; nothing here is tuned.
#include "vrg_facefix_packed_math.hpp"

namespace vrg {

__global__ __launch_bounds__(256) void k_ffp_lanczos(const uint8_t* __restrict__ src, const vrg_ff_packed_desc* __restrict__ desc,
                                                      uint8_t* __restrict__ out, int32_t out_h, int32_t out_w, uint32_t parts,
                                                      const LzTap* __restrict__ taps, FfpGeom g) {
    const uint32_t rec = blockIdx.x / parts;                              // < n: the grid is n * parts
    const int32_t n = out_h * out_w;
    const int32_t p = (int32_t)((blockIdx.x - rec * parts) * 256 + threadIdx.x);
    if (p >= n) return;
    const vrg_ff_packed_desc d = desc[rec];                               // wave-uniform
    uint8_t* dst = out + ((int64_t)rec * n + p) * 3;
    uint8_t o[3] = {0, 0, 0};
    if (ffp_crop_ok(d, g, out_h, out_w)) {
        const int32_t y = p / out_w, x = p - y * out_w;
        ff_crop_pixel(src + d.src_offset, d.box_w, d.box_w, d.box_h, taps[d.taps_offset + x], taps[d.taps_offset + out_w + y], o);
    }
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

__global__ __launch_bounds__(256) void k_ffp_resize_stats(const uint8_t* __restrict__ src, const uint8_t* __restrict__ enhanced,
                                                           const float* __restrict__ masks, const vrg_ff_packed_desc* __restrict__ desc,
                                                           const int64_t* __restrict__ prefix, const LzTap* __restrict__ taps,
                                                           uint8_t* __restrict__ bytes, unsigned long long* __restrict__ stats, FfpGeom g,
                                                           int32_t measure) {
    int64_t rec, p;
    vrg_ff_packed_desc d;                                                 // workgroup-uniform, and so is every return before the sums
    const auto admits = [&](const vrg_ff_packed_desc& r) { return ffp_blend_ok(r, g, true) && (!measure || packed_src_ok(r, g.src_bytes)); };
    if (!packed_tile_pixel(desc, prefix, g.n, admits, rec, d, p)) return;
    uint32_t acc[FF_STAT_SUMS] = {};
    if (p >= 0) {
        const int32_t dy = (int32_t)(p / d.box_w), dx = (int32_t)(p - (int64_t)dy * d.box_w);
        ff_resize_pixel(enhanced + (int64_t)d.enhanced_index * g.enh_h * g.enh_w * 3, g.enh_h, g.enh_w, taps[d.taps_offset + dx],
                        taps[d.taps_offset + d.box_w + dy], bytes + d.bytes_offset + p * 3, masks + d.mask_offset + p,
                        src + d.src_offset + p * 3, measure, acc);
    }
    if (measure) ff_block_stats(acc, stats + rec * FF_STATS_WORDS);     // uniform
}

__global__ __launch_bounds__(256) void k_ffp_composite(const uint8_t* __restrict__ src, const float* __restrict__ masks,
                                                        const vrg_ff_packed_desc* __restrict__ desc, const int64_t* __restrict__ prefix,
                                                        const uint8_t* __restrict__ bytes, const unsigned long long* __restrict__ stats,
                                                        uint8_t* __restrict__ out, FfpGeom g) {
    int64_t rec, p;
    vrg_ff_packed_desc d;                                                 // workgroup-uniform
    const auto admits = [&](const vrg_ff_packed_desc& r) { return packed_blocks_ok(r, g.src_bytes, g.out_bytes); };   // else nowhere to read or to write
    if (!packed_tile_pixel(desc, prefix, g.n, admits, rec, d, p) || p < 0) return;
    uint8_t o[3];
    packed_pixel_load(src, d.src_offset, p, o);
    if (ffp_blend_ok(d, g, false)) {
        float shift[3];
        const bool matched = ff_read_record(stats + rec * FF_STATS_WORDS, shift);
        const float alpha = masks[d.mask_offset + p];
        const uint8_t* fb = bytes + d.bytes_offset + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = ff_composite_byte(o[c], fb[c], matched, shift[c], alpha, d.strength);
    }
    packed_pixel_store(out, d.dst_offset, p, o);
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_ff_packed_check(const vrg_ff_packed_desc* desc_host, int64_t n, const int64_t* tile_prefix_host, int64_t src_bytes, int64_t out_bytes,
                        int64_t enhanced_frames, int64_t mask_floats, int64_t n_taps, int64_t capacity, int32_t out_h, int32_t out_w) {
    const bool crop = out_h > 0 || out_w > 0;
    if (!packed_sizes_ok({n, src_bytes, out_bytes, enhanced_frames, mask_floats, n_taps}) || capacity < 0 || out_h < 0 || out_w < 0 ||
        (crop && (out_h < 1 || out_w < 1)))
        return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!desc_host || (!crop && !tile_prefix_host)) return VRG_ERR_BAD_ARG;
    const FfpGeom g{n, src_bytes, out_bytes, enhanced_frames, mask_floats, n_taps, capacity, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const vrg_ff_packed_desc& d = desc_host[i];
        if (crop ? !ffp_crop_ok(d, g, out_h, out_w) : !(packed_blocks_ok(d, src_bytes, out_bytes) && ffp_blend_ok(d, g, true))) return VRG_ERR_BAD_ARG;
    }
    const auto tiles_of = [&](int64_t i) { return packed_tiles(packed_box_pixels(desc_host[i])); };
    if (tile_prefix_host && !tile_prefix_ok(n, tile_prefix_host, tiles_of)) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

int vrg_lanczos4_packed_u8(const uint8_t* src, int64_t src_bytes, const vrg_ff_packed_desc* desc, int64_t n, uint8_t* out, int32_t out_h,
                           int32_t out_w, const void* taps, int64_t n_taps, void* stream) {
    if (!src || !out || src == out || !desc || !taps || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || !packed_sizes_ok({n, src_bytes, n_taps}) ||
        out_h < 1 || out_w < 1)
        return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if ((int64_t)out_h * out_w * 3 > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const int64_t parts = ((int64_t)out_h * out_w + 255) / 256;
    if (n > 0x7fffffffll / parts) return VRG_ERR_UNSUPPORTED;
    const FfpGeom g{n, src_bytes, 0, 0, 0, n_taps, 0, 0, 0};
    hipLaunchKernelGGL(k_ffp_lanczos, dim3((uint32_t)(n * parts)), dim3(256), 0, (hipStream_t)stream, src, desc, out, out_h, out_w,
                       (uint32_t)parts, reinterpret_cast<const LzTap*>(taps), g);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_ff_packed_resize_stats_u8(const uint8_t* src, int64_t src_bytes, const uint8_t* enhanced, int64_t enhanced_frames, int32_t enh_h,
                                  int32_t enh_w, const float* masks, int64_t mask_floats, const vrg_ff_packed_desc* desc,
                                  const int64_t* tile_prefix, int64_t n, int64_t tiles, const void* taps, int64_t n_taps, uint8_t* bytes,
                                  int64_t capacity, void* stats, float color_match, void* stream) {
    if (!packed_sizes_ok({n, src_bytes, enhanced_frames, mask_floats, n_taps, capacity}) || tiles < 0) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!src || !enhanced || !masks || !desc || !tile_prefix || (reinterpret_cast<uintptr_t>(tile_prefix) & 7u) != 0 || !taps ||
        (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || !bytes || !stats || (reinterpret_cast<uintptr_t>(stats) & 7u) != 0 || bytes == src ||
        bytes == enhanced || enh_h < 1 || enh_w < 1)
        return VRG_ERR_BAD_ARG;
    if ((int64_t)enh_h * enh_w * 3 > 0x7fffffffll || tiles > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const int rc = ff_stats_begin(stats, n, stream);
    if (rc != VRG_OK) return rc;
    const FfpGeom g{n, src_bytes, 0, enhanced_frames, mask_floats, n_taps, capacity, enh_h, enh_w};
    if (tiles > 0) {
        hipLaunchKernelGGL(k_ffp_resize_stats, dim3((uint32_t)tiles), dim3(256), 0, (hipStream_t)stream, src, enhanced, masks, desc, tile_prefix,
                           reinterpret_cast<const LzTap*>(taps), bytes, (unsigned long long*)stats, g, color_match > 0.0f ? 1 : 0);
        VRG_CHECK_LAUNCH();
    }
    return ff_stats_end(stats, n, color_match, stream);
}

int vrg_ff_packed_composite_u8(const uint8_t* src, int64_t src_bytes, const float* masks, int64_t mask_floats, const vrg_ff_packed_desc* desc,
                               const int64_t* tile_prefix, int64_t n, int64_t tiles, const uint8_t* bytes, int64_t capacity, const void* stats,
                               uint8_t* out, int64_t out_bytes, void* stream) {
    if (!packed_sizes_ok({n, src_bytes, mask_floats, capacity, out_bytes}) || tiles < 0) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!src || !masks || !desc || !tile_prefix || (reinterpret_cast<uintptr_t>(tile_prefix) & 7u) != 0 || !bytes || !stats ||
        (reinterpret_cast<uintptr_t>(stats) & 7u) != 0 || !out || out == src || out == bytes)
        return VRG_ERR_BAD_ARG;
    if (tiles > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    if (tiles == 0) return VRG_OK;
    const FfpGeom g{n, src_bytes, out_bytes, 0, mask_floats, 0, capacity, 0, 0};
    hipLaunchKernelGGL(k_ffp_composite, dim3((uint32_t)tiles), dim3(256), 0, (hipStream_t)stream, src, masks, desc, tile_prefix, bytes,
                       (const unsigned long long*)stats, out, g);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
