// vrg_facefix_packed_math.hpp -- where a workgroup of csrc/vrg_facefix_packed.hip works, and which records it may follow; host and device.
//
// The Builder's Face Fix on frames that stay on the host: every box travels as a dense [box_h][box_w][3] block of one packed buffer, so a
// launch covers boxes of unrelated sizes with a one-dimensional grid.  A workgroup is one TILE of FFP_TILE consecutive box pixels (row-major
// inside the box); the host uploads, behind the records, the running sum of the records' tile counts:
//   prefix[i] = the first tile of record i (prefix[0] = 0), prefix[n] = all tiles = the grid.
// Records without tiles (a box below 1 x 1) repeat the value of their successor, so the owner of a tile is the LAST record whose prefix is
// not above it (ffp_find; the search of rb_find in csrc/vrg_refbatch.hip on a table of its own).  A kernel never trusts the table: the tile
// index inside the record is checked against the record's own tile count (ffp_place), and every span against the stated sizes
// (ffp_*_ok).  vrg_ff_packed_check applies the same rules on the host.  The per-pixel body and the blend checks are
// csrc/vrg_facefix_body.hpp, shared with the whole-frame kernels.
#pragma once
#include "vrg_facefix_body.hpp"

namespace vrg {

constexpr int FFP_TILE = VRG_FF_PACKED_TILE;
static_assert(FFP_TILE == 256, "one tile = one workgroup of 256 threads, one pixel each");
constexpr int64_t FFP_MAX_BOX_BYTES = 0x7fffffffll;

struct FfpGeom {
    int64_t n, src_bytes, out_bytes, enhanced_frames, mask_floats, n_taps, capacity;
    int32_t enh_h, enh_w;
};

// pixels of a box; 0: no box (a side below 1, or 2^31 bytes and more)
VRG_HD int64_t ffp_pixels(const vrg_ff_packed_desc& d) {
    if (d.box_w < 1 || d.box_h < 1) return 0;
    const int64_t px = (int64_t)d.box_w * d.box_h;
    return px > FFP_MAX_BOX_BYTES / 3 ? 0 : px;
}

VRG_HD int64_t ffp_tiles(const vrg_ff_packed_desc& d) { return (ffp_pixels(d) + FFP_TILE - 1) / FFP_TILE; }

// the record that owns `tile`: the last i in [0, n) with prefix[i] <= tile; n >= 1
VRG_HD int64_t ffp_find(const int64_t* prefix, int64_t n, int64_t tile) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// (record, tile) -> the pixels [p0, p0 + count) of the record's box; false: the tile is not one of this record's
VRG_HD bool ffp_place(const vrg_ff_packed_desc& d, int64_t first_tile, int64_t tile, int64_t& p0, int32_t& count) {
    const int64_t rel = tile - first_tile, px = ffp_pixels(d);
    if (rel < 0 || rel >= ffp_tiles(d)) return false;
    p0 = rel * FFP_TILE;
    count = (int32_t)(px - p0 < FFP_TILE ? px - p0 : FFP_TILE);
    return true;
}

// the box's original bytes lie inside `src`
VRG_HD bool ffp_src_ok(const vrg_ff_packed_desc& d, const FfpGeom& g) {
    const int64_t px = ffp_pixels(d);
    return px > 0 && span_fits(d.src_offset, px * 3, g.src_bytes);
}

// a record of vrg_lanczos4_packed_u8
VRG_HD bool ffp_crop_ok(const vrg_ff_packed_desc& d, const FfpGeom& g, int32_t out_h, int32_t out_w) {
    return ffp_src_ok(d, g) && span_fits(d.taps_offset, (int64_t)out_w + out_h, g.n_taps);
}

// what the composite needs to write anything at all: where the bytes come from and where they go
VRG_HD bool ffp_blocks_ok(const vrg_ff_packed_desc& d, const FfpGeom& g) {
    return ffp_src_ok(d, g) && span_fits(d.dst_offset, ffp_pixels(d) * 3, g.out_bytes);
}

// ... and to blend: ff_blend_ok on the pixels ffp_pixels allows
VRG_HD bool ffp_blend_ok(const vrg_ff_packed_desc& d, const FfpGeom& g, bool resized) { return ff_blend_ok(d, g, ffp_pixels(d), resized); }

// prefix[0 .. n] is the running sum of the records' tile counts
inline bool ffp_prefix_ok(const vrg_ff_packed_desc* desc, int64_t n, const int64_t* prefix) {
    int64_t want = 0;                                                     // at most n * 2^23
    for (int64_t i = 0; i < n; ++i) {
        if (prefix[i] != want) return false;
        want += ffp_tiles(desc[i]);
    }
    return prefix[n] == want;
}

}  // namespace vrg
