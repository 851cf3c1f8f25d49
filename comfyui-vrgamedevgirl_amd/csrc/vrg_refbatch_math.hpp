// vrg_refbatch_math.hpp -- arithmetic of the multi-reference image batches (csrc/vrg_refbatch.hip), host and device.
//
// What is restated: VRGDG_MultiReferenceConditioning._scale_to_total_pixels / ._batch_for_image_output and
// VRGDG_ImageBatchMultiFromPaths.load_batch of the reference (VRGDG_GeneralNodes2.py:3859-3910, :4112-4145).  Pictures of unrelated sizes
// and channel counts go through comfy.utils.common_upscale(image.movedim(-1, 1), w, h, method, crop): the channels-last view, narrowed to
// a centre-crop rectangle when crop == "center" (planned on the host, ops.center_crop_rect), and F.interpolate(mode = "nearest-exact" |
// "bilinear" | "area" | "bicubic") over it -- or, for "lanczos", a round trip through bytes and Pillow.  EVERY channel is resampled, taps are
// clamped to the rectangle and the result is NOT clamped to [0, 1]: overshoot, out-of-range values, Inf and NaN pass as torch passes them.
//
// Only what vrg_resize_math.hpp does not hold is written here; bicubic (rs_taps / rs_dot), bilinear (rs_linear_taps / rs_bilinear_value,
// torch's kernel choice rs_bilinear_paired) and area (rs_area_window, two divisions) are called from there.  New:
//   nearest-exact   index = min((int)floorf(((float)d + 0.5f) * scale), in - 1), scale = (float)in / (float)out (ATen/native/UpSample.h:
//                   nearest_exact_idx).
//   equal sizes     _scale_to_total_pixels calls F.interpolate even when source and target sizes agree, so the filter IS evaluated: bicubic
//                   multiplies the neighbours by weights of 0 (an Inf next to a pixel makes it NaN) and torch's linear kernels short-cut an
//                   axis with in == out to taps (d, d), weights (1, 0) -- x * 1 + x * 0, which makes an Inf NaN but leaves its neighbours
//                   alone (compute_source_index_and_lambda).  rs_linear_taps gives (d, d + 1), (1, 0): the same for finite values only, so
//                   rb_linear_taps adds the short-cut.  The batch step is different: a picture that already has the base's height and width
//                   is not resampled by the reference and takes RB_COPY, bit for bit.
//   channel pad     F.pad(picture, value=1.0) comes BEFORE the resize in the reference.  Here a missing channel loads as 1.0f and runs
//                   through the same filter as the others -- it is computed, not assumed constant (fl(1 - t) + t need not be 1).
//   byte source     RB_BYTES: out = (float)byte / 255.0f, one IEEE division: numpy's astype(float32) / 255.0.
//   quantise        comfy's lanczos goes through np.clip(255. * x, 0, 255).astype(np.uint8): the product formed in fp32, clipped, truncated.
//                   numpy's conversion of NaN is undefined; here NaN becomes 0.  The bytes are resampled by vrg_pil_resize_u8.
// Not restated: an "area" resize to a 1 x 1 TARGET is torch's mean() reduction (vrg_resize_math.hpp, rs_area_window); such a record gets
// the window rule and is a few ulp away.  An area window of more than RB_AREA_MAX_WINDOW source pixels per output pixel is refused: one
// lane walks the window.
// tests/test_refbatch_host.py holds this header, compiled for the host, to torch itself run live.
#pragma once
#include "vrg_common.hpp"
#include "vrg_packed_tiles.hpp"
#include "vrg_resize_math.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace vrg {

enum { RB_BICUBIC = RS_BICUBIC, RB_BILINEAR = RS_BILINEAR, RB_AREA = RS_AREA, RB_NEAREST_EXACT = 3, RB_COPY = 4, RB_BYTES = 5 };
constexpr int32_t RB_TILE = VRG_REFBATCH_TILE;          // elements of one frame one workgroup writes: 256 lanes x 4
constexpr int64_t RB_AREA_MAX_WINDOW = 1 << 16;         // source pixels under one output pixel

VRG_HD int32_t rb_nearest_exact(int32_t d, float scale, int32_t in) {
    const int32_t i = (int32_t)__builtin_floorf(((float)d + 0.5f) * scale);
    return i < in - 1 ? i : in - 1;
}

// torch's linear taps of one axis, with its short-cut for in == out (see above)
VRG_HD void rb_linear_taps(int32_t d, int32_t in, int32_t out, int32_t (&idx)[2], float (&w)[2]) {
    if (in == out) {
        idx[0] = idx[1] = d;
        w[0] = 1.0f;
        w[1] = 0.0f;
        return;
    }
    rs_linear_taps(d, rs_scale(in, out), in, idx, w);
}

VRG_HD float rb_from_byte(uint8_t b) { return (float)b / 255.0f; }

VRG_HD uint8_t rb_quantise(float x) {
    const float v = 255.0f * x;
    if (!(v > 0.0f)) return 0;                          // negatives, -0.0, -Inf and NaN
    return v >= 255.0f ? (uint8_t)255 : (uint8_t)v;     // truncation, as astype(np.uint8)
}

VRG_HD int64_t rb_src_frame(const vrg_refbatch_desc& d) { return (int64_t)d.src_h * d.src_w * d.src_c; }
VRG_HD int64_t rb_dst_frame(const vrg_refbatch_desc& d) { return (int64_t)d.dst_h * d.dst_w * d.dst_c; }
VRG_HD int64_t rb_tiles(const vrg_refbatch_desc& d) { return (int64_t)d.frames * ((rb_dst_frame(d) + RB_TILE - 1) / RB_TILE); }

// the record tile `tile` belongs to: the last one whose first_tile is <= tile -- tile_owner of csrc/vrg_packed_tiles.hpp over the records
VRG_HD int64_t rb_find(const vrg_refbatch_desc* desc, int64_t n, int32_t tile) {
    return tile_owner(n, tile, [&](int64_t i) { return desc[i].first_tile; });
}

// The rules of one record, which the launch and the kernel apply as well: VRG_OK, VRG_ERR_BAD_ARG or VRG_ERR_UNSUPPORTED
VRG_HD int rb_desc_status(const vrg_refbatch_desc& d) {
    if (d.frames < 0 || d.src_h < 1 || d.src_w < 1 || d.dst_h < 1 || d.dst_w < 1 || d.src_offset < 0 || d.dst_offset < 0) return VRG_ERR_BAD_ARG;
    if ((d.src_c != 3 && d.src_c != 4) || (d.dst_c != 3 && d.dst_c != 4) || d.dst_c < d.src_c) return VRG_ERR_BAD_ARG;
    if (d.src_x0 < 0 || d.src_y0 < 0 || d.src_rw < 1 || d.src_rh < 1 || (int64_t)d.src_x0 + d.src_rw > d.src_w ||
        (int64_t)d.src_y0 + d.src_rh > d.src_h)
        return VRG_ERR_BAD_ARG;
    if (d.method < RB_BICUBIC || d.method > RB_BYTES) return VRG_ERR_BAD_ARG;
    if ((d.method == RB_COPY || d.method == RB_BYTES) && (d.dst_h != d.src_rh || d.dst_w != d.src_rw)) return VRG_ERR_BAD_ARG;
    // in-picture offsets are 32-bit; pictures and frames are addressed with 64 bits
    if (rb_src_frame(d) > 0x7fffffff || rb_dst_frame(d) > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    if (d.method == RB_AREA) {
        const int64_t wh = ((int64_t)d.src_rh + d.dst_h - 1) / d.dst_h + 1, ww = ((int64_t)d.src_rw + d.dst_w - 1) / d.dst_w + 1;
        if (wh * ww > RB_AREA_MAX_WINDOW) return VRG_ERR_UNSUPPORTED;
    }
    return VRG_OK;
}

// what the kernel asks of a record before it follows it: the rules above and spans that lie inside the buffers
VRG_HD bool rb_desc_fits(const vrg_refbatch_desc& d, int64_t src_floats, int64_t src_bytes, int64_t out_elems) {
    if (rb_desc_status(d) != VRG_OK) return false;
    return span_fits(d.src_offset, d.frames * rb_src_frame(d), d.method == RB_BYTES ? src_bytes : src_floats) &&
           span_fits(d.dst_offset, d.frames * rb_dst_frame(d), out_elems);
}

// vrg_refbatch_quantise_u8 takes records that copy: fp32 rectangle in, the same rectangle in bytes out, no pad
VRG_HD bool rb_quantise_ok(const vrg_refbatch_desc& d) { return d.method == RB_COPY && d.dst_c == d.src_c; }

// torch's bilinear kernel choice for the narrowed view of `frames` pictures [src_h][src_w][dst_c] (the pad comes first)
VRG_HD bool rb_paired(const vrg_refbatch_desc& d) {
    return rs_bilinear_paired(rs_view_contiguous(d.frames, d.src_h, d.src_w, d.src_rw, d.src_rh), d.dst_c, d.dst_h, d.dst_w);
}

// The taps of one output pixel, shared by its channels.  bicubic: ix / iy / wx / wy[0..3]; bilinear: [0..1]; area: the window
// [ix[0], ix[1]) x [iy[0], iy[1]); nearest-exact, copy, bytes: (ix[0], iy[0]).  Rectangle coordinates.
struct RbTaps {
    int32_t ix[4], iy[4];
    float wx[4], wy[4];
};

VRG_HD void rb_taps(const vrg_refbatch_desc& d, int32_t y, int32_t x, RbTaps& t) {
    if (d.method == RB_BICUBIC) {
        rs_taps(x, rs_scale(d.src_rw, d.dst_w), d.src_rw, t.ix, t.wx);
        rs_taps(y, rs_scale(d.src_rh, d.dst_h), d.src_rh, t.iy, t.wy);
    } else if (d.method == RB_BILINEAR) {
        int32_t i2[2];
        float w2[2];
        rb_linear_taps(x, d.src_rw, d.dst_w, i2, w2);
        t.ix[0] = i2[0], t.ix[1] = i2[1], t.wx[0] = w2[0], t.wx[1] = w2[1];
        rb_linear_taps(y, d.src_rh, d.dst_h, i2, w2);
        t.iy[0] = i2[0], t.iy[1] = i2[1], t.wy[0] = w2[0], t.wy[1] = w2[1];
    } else if (d.method == RB_AREA) {
        rs_area_window(x, d.src_rw, d.dst_w, t.ix[0], t.ix[1]);
        rs_area_window(y, d.src_rh, d.dst_h, t.iy[0], t.iy[1]);
    } else if (d.method == RB_NEAREST_EXACT) {
        t.ix[0] = rb_nearest_exact(x, rs_scale(d.src_rw, d.dst_w), d.src_rw);
        t.iy[0] = rb_nearest_exact(y, rs_scale(d.src_rh, d.dst_h), d.src_rh);
    } else {
        t.ix[0] = x;
        t.iy[0] = y;
    }
}

// One channel of the pixel whose taps are `t`.  `load(y, x, ch)`: the padded picture in rectangle coordinates (1.0f for ch >= src_c).
template <typename LOAD>
VRG_HD float rb_value(const vrg_refbatch_desc& d, bool paired, const RbTaps& t, int32_t ch, LOAD load) {
    if (d.method == RB_BICUBIC) {
        float rows[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = load(t.iy[j], t.ix[i], ch);
            rows[j] = rs_dot<4>(t.wx, v);
        }
        return rs_dot<4>(t.wy, rows);
    }
    if (d.method == RB_BILINEAR) {
        const float wx[2] = {t.wx[0], t.wx[1]}, wy[2] = {t.wy[0], t.wy[1]};
        return rs_bilinear_value(paired, wx, wy, load(t.iy[0], t.ix[0], ch), load(t.iy[0], t.ix[1], ch), load(t.iy[1], t.ix[0], ch),
                                 load(t.iy[1], t.ix[1], ch));
    }
    if (d.method == RB_AREA) {
        float sum = 0.0f;
        for (int32_t y = t.iy[0]; y < t.iy[1]; ++y)
            for (int32_t x = t.ix[0]; x < t.ix[1]; ++x) sum = sum + load(y, x, ch);
        return sum / (float)(t.iy[1] - t.iy[0]) / (float)(t.ix[1] - t.ix[0]);
    }
    return load(t.iy[0], t.ix[0], ch);
}

// element i of one padded source frame of a record, rectangle coordinates
VRG_HD uint32_t rb_src_index(const vrg_refbatch_desc& d, int32_t y, int32_t x, int32_t ch) {
    return ((uint32_t)(d.src_y0 + y) * (uint32_t)d.src_w + (uint32_t)(d.src_x0 + x)) * (uint32_t)d.src_c + (uint32_t)ch;
}

// vrg_refbatch_check: every record by rb_desc_status, the spans inside the buffers, first_tile the running sum of rb_tiles, no two
// outputs overlapping.  `out_elems`: floats of `out` (bytes of `dst` for vrg_refbatch_quantise_u8).
inline int rb_check(const vrg_refbatch_desc* desc, int64_t n, int64_t src_floats, int64_t src_bytes, int64_t out_elems) {
    if (n < 0 || src_floats < 0 || src_bytes < 0 || out_elems < 0 || (n > 0 && !desc)) return VRG_ERR_BAD_ARG;
    int64_t tiles = 0;
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (int64_t i = 0; i < n; ++i) {
        const vrg_refbatch_desc& d = desc[i];
        const int rc = rb_desc_status(d);
        if (rc != VRG_OK) return rc;
        if (!rb_desc_fits(d, src_floats, src_bytes, out_elems) || d.first_tile != tiles) return VRG_ERR_BAD_ARG;
        tiles += rb_tiles(d);
        if (tiles > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
        if (d.frames > 0) spans.emplace_back(d.dst_offset, d.dst_offset + d.frames * rb_dst_frame(d));
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first < spans[i - 1].second) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

// vrg_refbatch_f32 in plain loops (tests/host_math/refbatch_check.cpp)
inline void rb_records_host(const float* src_f32, const uint8_t* src_u8, const vrg_refbatch_desc* desc, int64_t n, float* out) {
    for (int64_t i = 0; i < n; ++i) {
        const vrg_refbatch_desc& d = desc[i];
        const bool paired = rb_paired(d);
        for (int64_t f = 0; f < d.frames; ++f) {
            const int64_t s0 = d.src_offset + f * rb_src_frame(d);
            float* o = out + d.dst_offset + f * rb_dst_frame(d);
            auto load = [&](int32_t y, int32_t x, int32_t ch) -> float {
                if (ch >= d.src_c) return 1.0f;
                const int64_t at = s0 + rb_src_index(d, y, x, ch);
                return d.method == RB_BYTES ? rb_from_byte(src_u8[at]) : src_f32[at];
            };
            for (int32_t y = 0; y < d.dst_h; ++y)
                for (int32_t x = 0; x < d.dst_w; ++x) {
                    RbTaps t;
                    rb_taps(d, y, x, t);
                    for (int32_t ch = 0; ch < d.dst_c; ++ch) *o++ = rb_value(d, paired, t, ch, load);
                }
        }
    }
}

// vrg_refbatch_quantise_u8 in plain loops
inline void rb_quantise_host(const float* src_f32, const vrg_refbatch_desc* desc, int64_t n, uint8_t* dst) {
    for (int64_t i = 0; i < n; ++i) {
        const vrg_refbatch_desc& d = desc[i];
        for (int64_t f = 0; f < d.frames; ++f) {
            uint8_t* o = dst + d.dst_offset + f * rb_dst_frame(d);
            for (int32_t y = 0; y < d.dst_h; ++y)
                for (int32_t x = 0; x < d.dst_w; ++x)
                    for (int32_t ch = 0; ch < d.dst_c; ++ch) *o++ = rb_quantise(src_f32[d.src_offset + f * rb_src_frame(d) + rb_src_index(d, y, x, ch)]);
        }
    }
}

}  // namespace vrg
