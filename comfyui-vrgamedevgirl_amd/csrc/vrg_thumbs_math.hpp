// vrg_thumbs_math.hpp -- the input of the landmark estimator (csrc/vrg_thumbs.hip), host side: the descriptor's rules and the thumbnail
// straight from the definition.
//
// What is restated: the first two calls of VRGDGFaceFixCompositeLandmarkAligned._landmarks (VRGDG_StandaloneFaceFixNodes.py:966-968 of the
// reference): cv2.resize(rgb, (320, 320), interpolation=cv2.INTER_AREA) of a [h][w][3] R,G,B byte image, then cv2.cvtColor(...,
// COLOR_RGB2BGR).  There is no arithmetic of its own here: the rule, the tables and every rounding are those of csrc/vrg_grid_math.hpp
// (copy, the integer fast paths, 2 x 2, the general fp32 sums, the fixed-point bilinear rule with area-mode coefficients when an axis
// enlarges); the channel flip is the `swap` of grid_resize_tile.
#pragma once
#include <stdint.h>

#include "../../include/vrgdg_hip.h"
#include "vrg_grid_math.hpp"

namespace vrg {

constexpr int THUMB_SIDE = VRG_THUMB_SIDE;                   // YuNet's input is fixed at 320 x 320
constexpr int THUMB_MAX_SIDE = VRG_THUMB_MAX_SIDE;
constexpr int THUMB_ROW_BYTES = THUMB_SIDE * 3;
constexpr int64_t THUMB_BYTES = (int64_t)THUMB_SIDE * THUMB_ROW_BYTES;
constexpr int THUMB_SEGMENTS = THUMB_SIDE / GRID_LANES;      // workgroups of one output row
static_assert(THUMB_SIDE % GRID_LANES == 0 && (GRID_LANES * 3) % 16 == 0 && THUMB_ROW_BYTES % 16 == 0 && THUMB_BYTES % 16 == 0,
              "the 192 bytes of a workgroup are twelve aligned 16-byte pieces of a 16-byte aligned output");

// HOST: what vrg_grid_plan(box_h, box_w, 3, 320, 320, ...) gives; false: the sides are not 1 .. 32767
inline bool thumb_plan(int32_t box_h, int32_t box_w, int32_t& mode, int32_t& cps, float& inv) {
    if (box_h < 1 || box_w < 1 || box_h > THUMB_MAX_SIDE || box_w > THUMB_MAX_SIDE) return false;
    mode = grid_mode(box_h, box_w, THUMB_SIDE, THUMB_SIDE);
    inv = mode == GRID_FAST || mode == GRID_FAST_2X2 ? grid_fast_inv(box_h, box_w, THUMB_SIDE, THUMB_SIDE) : 1.0f;
    AreaCell cells[THUMB_SIDE];
    grid_fill_taps(box_w, THUMB_SIDE, mode, cells);
    cps = grid_cells_per_segment(cells, THUMB_SIDE, 3);       // a column covers at most 104 pixels: never 0
    return cps >= 1;
}

// does the image of a descriptor lie inside n_bytes (host and device; the sides are checked first, so the product cannot overflow)
VRG_HD bool thumb_image_fits(int64_t offset, int32_t box_w, int32_t box_h, int64_t n_bytes) {
    if (box_w < 1 || box_h < 1 || box_w > THUMB_MAX_SIDE || box_h > THUMB_MAX_SIDE) return false;
    const int64_t need = (int64_t)box_w * box_h * 3;
    return offset >= 0 && offset <= n_bytes && need <= n_bytes - offset;                    // span_fits of vrg_common.hpp
}

// HOST: is this descriptor one the kernel follows as the caller means it
inline bool thumb_desc_ok(const vrg_thumb_desc& d, int64_t n_bytes, bool has_source) {
    if (d.which != 0 && d.which != 1) return false;
    if (d.which == 1 && !has_source) return false;
    if (!thumb_image_fits(d.offset, d.box_w, d.box_h, n_bytes)) return false;
    if (!d.xtab || !d.ytab) return false;
    int32_t mode = 0, cps = 0;
    float inv = 0.0f;
    if (!thumb_plan(d.box_h, d.box_w, mode, cps, inv)) return false;
    return d.mode == mode && d.cps == cps && d.inv == inv;
}

// ---- HOST: straight from the definition (tests/host_math/thumbs_check.cpp; never called from a kernel) ----

// in: one [box_h][box_w][3] R,G,B byte image, out: [320][320][3] bytes B,G,R
inline void thumb_from_definition(const uint8_t* in, int32_t box_h, int32_t box_w, uint8_t* out) {
    const int32_t mode = grid_mode(box_h, box_w, THUMB_SIDE, THUMB_SIDE);
    AreaCell xc[THUMB_SIDE], yc[THUMB_SIDE];
    grid_fill_taps(box_w, THUMB_SIDE, mode, xc);
    grid_fill_taps(box_h, THUMB_SIDE, mode, yc);
    grid_resize_tile<uint8_t>(in, box_h, box_w, 3, true, THUMB_SIDE, THUMB_SIDE, xc, yc, mode, out);
}

}  // namespace vrg
