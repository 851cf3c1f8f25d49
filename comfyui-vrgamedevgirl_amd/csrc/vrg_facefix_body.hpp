// vrg_facefix_body.hpp -- what the whole-frame kernels (csrc/vrg_facefix.hip) and the packed kernels (csrc/vrg_facefix_packed.hip) of the
// Builder's Face Fix do to one pixel, one byte, one record and one workgroup: written once, called with each route's own addresses (how a
// workgroup finds its record and pixel range, where the original pixel lives, which record of `stats` it adds to).  Host and device
// (tests/host_math/facefix_body_check.cpp); the end of the workgroup is device only.  Arithmetic: vrg_facefix_math.hpp, vrg_lanczos_math.hpp.
#pragma once
#include "vrg_common.hpp"
#include "vrg_facefix_math.hpp"
#include "vrg_lanczos_math.hpp"

namespace vrg {

// what a record (vrg_ff_desc / vrg_ff_packed_desc) of `px` box pixels needs to blend, held against the capacities of its launch's geometry;
// `resized` = the checks of the pass that reads the resize source as well
template <class D, class G>
VRG_HD bool ff_blend_ok(const D& d, const G& g, int64_t px, bool resized) {
    if (!(d.strength > 0.0f) || px < 1) return false;
    if (!span_fits(d.mask_offset, px, g.mask_floats) || !span_fits(d.bytes_offset, px * 3, g.capacity)) return false;
    if (!resized) return true;
    if (d.enhanced_index < 0 || d.enhanced_index >= g.enhanced_frames) return false;
    return span_fits(d.taps_offset, (int64_t)d.box_w + d.box_h, g.n_taps);
}

// prepare: one pixel of the crop.  `box` = the box's first byte, `pitch` = pixels from one of its rows to the next (the frame's width, or
// box_w for a dense block); the taps clamp to the box.  Tap records by value, here and below: a lane works on its own copy.
VRG_HD void ff_crop_pixel(const uint8_t* box, int32_t pitch, int32_t box_w, int32_t box_h, LzTap cx, LzTap ry, uint8_t o[3]) {
    lz_pixel(cx, ry, box_w, box_h, [&](int32_t sy, int32_t sx, int c) { return box[((int64_t)sy * pitch + sx) * 3 + c]; }, o);
}

// finalize, first half: one box pixel of the repaired frame `ef` ([enh_h][enh_w][3]) into the byte scratch at `dst`; with `measure` (else
// *alpha is not read), and the pixel selected by its mask value *alpha, its share of the seven sums (`original` = the bytes it is blended into)
VRG_HD void ff_resize_pixel(const uint8_t* ef, int32_t enh_h, int32_t enh_w, LzTap cx, LzTap ry, uint8_t* dst, const float* alpha,
                            const uint8_t* original, int32_t measure, uint32_t (&acc)[FF_STAT_SUMS]) {
    uint8_t o[3];
    lz_pixel(cx, ry, enh_w, enh_h, [&](int32_t sy, int32_t sx, int c) { return ef[((int64_t)sy * enh_w + sx) * 3 + c]; }, o);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    if (measure && ff_selected(*alpha)) {
        acc[0] = 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[1 + c] = o[c];
            acc[4 + c] = original[c];
        }
    }
}

// finalize, second half: one byte of the output
VRG_HD uint8_t ff_composite_byte(uint8_t original, uint8_t face, bool matched, float shift, float alpha, float strength) {
    if (matched) face = ff_shift_byte(face, shift);
    return ff_blend_byte(original, face, alpha, strength);
}

// The statistics of n records around a route's own tile launch: ff_stats_begin zeroes them, ff_stats_end fills in the means and shifts when
// color_match > 0 (k_ff_finish).  Host functions of csrc/vrg_facefix.hip, the one translation unit of that kernel (no relocatable device code).
int ff_stats_begin(void* stats, int64_t n, void* stream);
int ff_stats_end(void* stats, int64_t n, float color_match, void* stream);

#if defined(__HIPCC__) || defined(__HIP__)
// the end of a resize-and-measure workgroup (every thread calls it): lane sums -> wave butterfly -> LDS -> one 64-bit integer atomic per
// sum into `rec`, the workgroup's record of `stats` (integer addition: the same bits in any order)
__device__ __forceinline__ void ff_block_stats(uint32_t (&acc)[FF_STAT_SUMS], unsigned long long* rec) {
    __shared__ uint32_t part[4][FF_STAT_SUMS];
    block_sum_4waves(acc, part);
    if (threadIdx.x < FF_STAT_SUMS) {
        const int t = threadIdx.x;
        const uint32_t s = part[0][t] + part[1][t] + part[2][t] + part[3][t];             // <= 256 * 255
        if (s) atomicAdd(rec + t, (unsigned long long)s);
    }
}
#endif

}  // namespace vrg
