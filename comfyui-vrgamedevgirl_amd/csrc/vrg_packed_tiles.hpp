// vrg_packed_tiles.hpp -- the tile map of the packed routes (frames that stay on the host: only the boxes cross the bus); host and device.
//
// Every box travels as a dense [box_h][box_w][3] block of one packed buffer, so a launch covers boxes of unrelated sizes with a
// one-dimensional grid.  A workgroup is one TILE of PACKED_TILE consecutive box pixels (row-major inside the box); the host uploads, behind
// the records, the running sum of their tile counts: prefix[i] = the first tile of record i, prefix[n] = all tiles = the grid.  Records
// without tiles repeat the value of their successor, so the owner of a tile is the LAST record whose first tile is not above it (tile_owner:
// the one search under csrc/, here over a prefix array, in csrc/vrg_refbatch.hip over desc[i].first_tile).  A kernel never trusts the table:
// the tile is checked against the record's own tile count (tile_place) and every span against the stated sizes (packed_*_ok and the route's
// own checks: csrc/vrg_facefix_packed_math.hpp, csrc/vrg_farface_body.hpp).  The host checks of the routes apply the same rules.
#pragma once
#include <initializer_list>

#include "vrg_common.hpp"

namespace vrg {

constexpr int PACKED_TILE = 256;
static_assert(VRG_FF_PACKED_TILE == PACKED_TILE && VRG_PIL_PACKED_TILE == PACKED_TILE, "one tile = one workgroup of 256 threads, one pixel each");
constexpr int64_t PACKED_MAX_BOX_BYTES = 0x7fffffffll;

// the stated sizes of an entry point: none is negative (host)
inline bool packed_sizes_ok(std::initializer_list<int64_t> sizes) {
    for (int64_t v : sizes)
        if (v < 0) return false;
    return true;
}

// pixels of a box; 0: no box (a side below 1, or 2^31 bytes and more)
VRG_HD int64_t packed_box_pixels(int32_t box_w, int32_t box_h) {
    if (box_w < 1 || box_h < 1) return 0;
    const int64_t px = (int64_t)box_w * box_h;
    return px > PACKED_MAX_BOX_BYTES / 3 ? 0 : px;
}

template <class D>                                                       // D: vrg_ff_packed_desc, vrg_pil_packed_desc
VRG_HD int64_t packed_box_pixels(const D& d) { return packed_box_pixels(d.box_w, d.box_h); }

VRG_HD int64_t packed_tiles(int64_t pixels) { return (pixels + PACKED_TILE - 1) / PACKED_TILE; }

// the record that owns `tile`: the last i in [0, n) with first_of(i) <= tile; n >= 1
template <class First>
VRG_HD int64_t tile_owner(int64_t n, int64_t tile, First first_of) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (first_of(mid) <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// (a box of `pixels`, tile) -> the pixels [p0, p0 + count) of the box; false: the tile is not one of this record's
VRG_HD bool tile_place(int64_t pixels, int64_t first_tile, int64_t tile, int64_t& p0, int32_t& count) {
    const int64_t rel = tile - first_tile;
    if (rel < 0 || rel >= packed_tiles(pixels)) return false;
    p0 = rel * PACKED_TILE;
    count = (int32_t)(pixels - p0 < PACKED_TILE ? pixels - p0 : PACKED_TILE);
    return true;
}

// prefix[0 .. n] is the running sum of the records' tile counts tiles_of(i)
template <class Tiles>
VRG_HD bool tile_prefix_ok(int64_t n, const int64_t* prefix, Tiles tiles_of) {
    int64_t want = 0;                                                     // at most n * 2^23
    for (int64_t i = 0; i < n; ++i) {
        if (prefix[i] != want) return false;
        want += tiles_of(i);
    }
    return prefix[n] == want;
}

// the box's original bytes lie inside `src`; D: vrg_ff_packed_desc, vrg_pil_packed_desc
template <class D>
VRG_HD bool packed_src_ok(const D& d, int64_t src_bytes) {
    const int64_t px = packed_box_pixels(d);
    return px > 0 && span_fits(d.src_offset, px * 3, src_bytes);
}

// what a composite needs to write anything at all: where the bytes come from and where they go
template <class D>
VRG_HD bool packed_blocks_ok(const D& d, int64_t src_bytes, int64_t out_bytes) {
    return packed_src_ok(d, src_bytes) && span_fits(d.dst_offset, packed_box_pixels(d) * 3, out_bytes);
}

// pixel p of the dense block at `offset` of a packed buffer: three bytes in, three bytes out
VRG_HD void packed_pixel_load(const uint8_t* buffer, int64_t offset, int64_t p, uint8_t* o) {
    const uint8_t* t = buffer + offset + p * 3;
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
}

VRG_HD void packed_pixel_store(uint8_t* buffer, int64_t offset, int64_t p, const uint8_t* o) {
    uint8_t* dst = buffer + offset + p * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

#if defined(__HIPCC__) || defined(__HIP__)
// The prologue of a workgroup of a tile grid: the record that owns tile blockIdx.x -> rec and d (workgroup-uniform), and this lane's pixel
// of its box -> p, -1 for a lane behind the last pixel of the box.  false (uniform): nothing to do -- the route's `admits(d)` refuses the
// record, or the tile is not one of its.
template <class D, class Admits>
__device__ __forceinline__ bool packed_tile_pixel(const D* __restrict__ desc, const int64_t* __restrict__ prefix, int64_t n, Admits admits,
                                                  int64_t& rec, D& d, int64_t& p) {
    rec = tile_owner(n, (int64_t)blockIdx.x, [&](int64_t i) { return prefix[i]; });
    d = desc[rec];
    if (!admits(d)) return false;
    int64_t p0;
    int32_t count;
    if (!tile_place(packed_box_pixels(d), prefix[rec], (int64_t)blockIdx.x, p0, count)) return false;
    p = (int32_t)threadIdx.x < count ? p0 + threadIdx.x : -1;
    return true;
}
#endif

}  // namespace vrg
