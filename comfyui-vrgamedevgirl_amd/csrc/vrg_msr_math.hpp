// vrg_msr_math.hpp -- what the LTX MSR reference frames (csrc/vrg_msr.hip) add to vrg_lanczos_math.hpp and vrg_grid_math.hpp, host and device.
//
// What is restated: VRGDG_LTXMSRReferenceBuilder.build_reference and _pil_to_image_tensor of the reference
// (vrgdg_ltx_msr_reference_builder.py:37-58, 96-134): every distinct picture -- up to four subject stills and a background -- is stretched
// with cv2.resize(..., INTER_LANCZOS4) on bytes (vrg_lanczos_math.hpp: 8 x 8 taps, 11-bit weights, int32 sums, one rounding, taps clamped,
// no antialiasing) unless it already has the output size, repeated into its run of frames (_expand_frames) and returned as
// np.stack(frames).astype(np.float32) / 255.0 = (float)byte / 255.0f, correctly rounded (grid_unit).
//
// A workgroup owns one MSR_TW x MSR_TH tile of one descriptor.  The rows of a tile are taken in STRIPS: the longest run of consecutive
// output rows whose distinct source rows fit MSR_SLOTS rows of horizontal sums in LDS.  msr_plan_strip gives every output row the slot of
// its first source row and every slot its source row; rows of neighbours that overlap (enlarging) share slots, rows that do not (shrinking
// by more than 8) follow each other without the gap between them, so no source row is filtered that no tap reads.  One output row needs
// at most 8 slots, so any ratio fits.  The planner takes any record content: rows that do not ascend are placed afresh.
// The host walk below (msr_tile_host, msr_frames_host) is the kernel's walk in plain loops over the same planner; tests/host_math/msr_check.cpp
// holds it to the independent numpy restatement of tests/lanczos_support.py.
#pragma once
#include "vrg_common.hpp"
#include "vrg_grid_math.hpp"
#include "vrg_lanczos_math.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace vrg {

constexpr int MSR_TW = 64, MSR_TH = 32;             // output pixels of one tile
constexpr int MSR_SLOTS = 40;                       // source rows of horizontal sums a strip holds (>= LZ_TAPS)
constexpr int MSR_ROW_VALUES = MSR_TW * 3;          // floats of one tile row: 48 groups of four

// What the kernel checks of a descriptor before it follows it: frames inside the batch, sizes, the table range.
VRG_HD bool msr_desc_ok(const vrg_msr_desc& d, int64_t n_taps, int64_t frames, int32_t out_h, int32_t out_w) {
    if (d.repeats < 0 || d.first_frame < 0 || (int64_t)d.first_frame + (int64_t)d.repeats > frames) return false;
    if (!d.src) return true;
    if (d.in_h < 1 || d.in_w < 1) return false;
    if (d.taps == -1) return d.in_h == out_h && d.in_w == out_w;
    return d.taps >= 0 && span_fits((int64_t)d.taps, (int64_t)out_w + (int64_t)out_h, n_taps);
}

// The strip that starts at tile row ly0 (rs[ly] = s of the row's record, rows = rows of the tile inside the picture): slot0[ly] = slot of
// the row's first distinct source row clamp(s - 3), srcrow[slot] = the source row a slot holds, slots = slots used.  Returns the rows taken
// (at least 1).  Tap k of row ly reads slot0[ly] + clamp(s - 3 + k) - clamp(s - 3).
VRG_HD int32_t msr_plan_strip(const int32_t* rs, int32_t ly0, int32_t rows, int32_t in_h, int32_t* slot0, int32_t* srcrow, int32_t& slots) {
    int32_t n = 0, prev_a = 0, prev_b = -1;
    slots = 0;
    for (int32_t ly = ly0; ly < rows; ++ly) {
        const int32_t a = lz_clampi(rs[ly] - 3, in_h - 1), b = lz_clampi(rs[ly] + LZ_TAPS - 4, in_h - 1);
        const bool shares = slots > 0 && a >= prev_a && a <= prev_b && b >= prev_b;
        const int32_t from = shares ? prev_b + 1 : a;
        if (slots + (b - from + 1) > MSR_SLOTS) break;
        slot0[ly] = shares ? slots - 1 - (prev_b - a) : slots;
        for (int32_t r = from; r <= b; ++r) srcrow[slots++] = r;
        prev_a = a;
        prev_b = b;
        ++n;
    }
    return n;
}

// The vertical pass of one output value: h(slot) = the horizontal sum of that slot
template <typename H>
VRG_HD uint8_t msr_vertical(const LzTap& ry, int32_t first_slot, int32_t in_h, H h) {
    const int32_t a = lz_clampi(ry.s - 3, in_h - 1);
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < LZ_TAPS; ++k) v = lz_mac(v, h(first_slot + lz_clampi(ry.s - 3 + k, in_h - 1) - a), (int32_t)ry.w[k]);
    return lz_cast(v);
}

// ---- HOST ----

// Are the frame ranges disjoint and do they cover 0 .. frames - 1 exactly?  (every descriptor has passed msr_desc_ok)
inline bool msr_covers(const vrg_msr_desc* desc, int64_t n_desc, int64_t frames) {
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (int64_t i = 0; i < n_desc; ++i)
        if (desc[i].repeats > 0) runs.emplace_back((int64_t)desc[i].first_frame, (int64_t)desc[i].repeats);
    std::sort(runs.begin(), runs.end());
    int64_t next = 0;
    for (const auto& r : runs) {
        if (r.first != next) return false;
        next += r.second;
    }
    return next == frames;
}

inline int msr_check(const vrg_msr_desc* desc, int64_t n_desc, int64_t n_taps, int64_t frames, int32_t out_h, int32_t out_w) {
    if (n_desc < 0 || n_taps < 0 || frames < 0 || out_h < 1 || out_w < 1 || (n_desc > 0 && !desc)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_desc; ++i)
        if (!msr_desc_ok(desc[i], n_taps, frames, out_h, out_w)) return VRG_ERR_BAD_ARG;
    return msr_covers(desc, n_desc, frames) ? VRG_OK : VRG_ERR_BAD_ARG;
}

// The bytes of the tile at (x0, y0) of one descriptor, tile[MSR_TH][MSR_ROW_VALUES], as k_msr_tile makes them (src and taps on the host)
inline void msr_tile_host(const vrg_msr_desc& d, const LzTap* table, int32_t out_h, int32_t out_w, int32_t x0, int32_t y0, uint8_t* tile) {
    const int32_t cols = out_w - x0 < MSR_TW ? out_w - x0 : MSR_TW, rows = out_h - y0 < MSR_TH ? out_h - y0 : MSR_TH;
    if (!d.src || d.taps < 0) {
        for (int32_t ly = 0; ly < rows; ++ly)
            for (int32_t i = 0; i < cols * 3; ++i)
                tile[ly * MSR_ROW_VALUES + i] = d.src ? d.src[((int64_t)(y0 + ly) * d.in_w + x0) * 3 + i] : d.fill[i % 3];
        return;
    }
    const LzTap* cx = table + d.taps + x0;
    const LzTap* ry = table + d.taps + out_w + y0;
    int32_t rs[MSR_TH], slot0[MSR_TH], srcrow[MSR_SLOTS], slots;
    std::vector<int32_t> h((size_t)MSR_SLOTS * 3 * MSR_TW);
    for (int32_t ly = 0; ly < rows; ++ly) rs[ly] = ry[ly].s;
    for (int32_t ly0 = 0; ly0 < rows;) {
        const int32_t n = msr_plan_strip(rs, ly0, rows, d.in_h, slot0, srcrow, slots);
        for (int32_t slot = 0; slot < slots; ++slot) {
            const uint8_t* row = d.src + (int64_t)srcrow[slot] * d.in_w * 3;
            for (int32_t c = 0; c < 3; ++c)
                for (int32_t x = 0; x < cols; ++x)
                    h[((size_t)slot * 3 + c) * MSR_TW + x] = lz_hsum(cx[x], d.in_w, [&](int32_t sx) { return row[sx * 3 + c]; });
        }
        for (int32_t ly = ly0; ly < ly0 + n; ++ly)
            for (int32_t x = 0; x < cols; ++x)
                for (int32_t c = 0; c < 3; ++c)
                    tile[ly * MSR_ROW_VALUES + x * 3 + c] =
                        msr_vertical(ry[ly], slot0[ly], d.in_h, [&](int32_t slot) { return h[((size_t)slot * 3 + c) * MSR_TW + x]; });
        ly0 += n;
    }
}

// vrg_msr_frames_f32 on the host: every tile of every descriptor, converted once and written to each of its frames
inline void msr_frames_host(const vrg_msr_desc* desc, int64_t n_desc, const LzTap* table, float* out, int32_t out_h, int32_t out_w) {
    std::vector<uint8_t> tile((size_t)MSR_TH * MSR_ROW_VALUES);
    for (int64_t i = 0; i < n_desc; ++i) {
        const vrg_msr_desc& d = desc[i];
        if (d.repeats < 1) continue;
        for (int32_t y0 = 0; y0 < out_h; y0 += MSR_TH)
            for (int32_t x0 = 0; x0 < out_w; x0 += MSR_TW) {
                msr_tile_host(d, table, out_h, out_w, x0, y0, tile.data());
                const int32_t cols = out_w - x0 < MSR_TW ? out_w - x0 : MSR_TW, rows = out_h - y0 < MSR_TH ? out_h - y0 : MSR_TH;
                for (int32_t f = d.first_frame; f < d.first_frame + d.repeats; ++f)
                    for (int32_t ly = 0; ly < rows; ++ly) {
                        float* o = out + (((int64_t)f * out_h + (y0 + ly)) * out_w + x0) * 3;
                        for (int32_t v = 0; v < cols * 3; ++v) o[v] = grid_unit((int32_t)tile[ly * MSR_ROW_VALUES + v]);
                    }
            }
    }
}

}  // namespace vrg
