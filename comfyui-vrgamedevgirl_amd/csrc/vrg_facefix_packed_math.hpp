// vrg_facefix_packed_math.hpp -- which records a workgroup of csrc/vrg_facefix_packed.hip may follow; host and device.
//
// The Builder's Face Fix on frames that stay on the host.  Where a workgroup works -- tiles, the prefix table, the spans of a box's blocks
// -- is csrc/vrg_packed_tiles.hpp, shared with the far-face route; here are the checks only this route's records have.
// vrg_ff_packed_check applies the same rules on the host.  The per-pixel body and the blend checks are csrc/vrg_facefix_body.hpp, shared
// with the whole-frame kernels.
#pragma once
#include "vrg_facefix_body.hpp"
#include "vrg_packed_tiles.hpp"

namespace vrg {

struct FfpGeom {
    int64_t n, src_bytes, out_bytes, enhanced_frames, mask_floats, n_taps, capacity;
    int32_t enh_h, enh_w;
};

// the shared tile map under this route's names, on its records and its prefix table (tests/host_math hold it by these)
constexpr int FFP_TILE = PACKED_TILE;
VRG_HD int64_t ffp_tiles(const vrg_ff_packed_desc& d) { return packed_tiles(packed_box_pixels(d)); }
VRG_HD int64_t ffp_find(const int64_t* prefix, int64_t n, int64_t tile) {
    return tile_owner(n, tile, [&](int64_t i) { return prefix[i]; });
}
VRG_HD bool ffp_place(const vrg_ff_packed_desc& d, int64_t first_tile, int64_t tile, int64_t& p0, int32_t& count) {
    return tile_place(packed_box_pixels(d), first_tile, tile, p0, count);
}

// a record of vrg_lanczos4_packed_u8
VRG_HD bool ffp_crop_ok(const vrg_ff_packed_desc& d, const FfpGeom& g, int32_t out_h, int32_t out_w) {
    return packed_src_ok(d, g.src_bytes) && span_fits(d.taps_offset, (int64_t)out_w + out_h, g.n_taps);
}

// what the composite needs, beyond its blocks, to blend: ff_blend_ok on the pixels packed_box_pixels allows
VRG_HD bool ffp_blend_ok(const vrg_ff_packed_desc& d, const FfpGeom& g, bool resized) {
    return ff_blend_ok(d, g, packed_box_pixels(d), resized);
}

}  // namespace vrg
