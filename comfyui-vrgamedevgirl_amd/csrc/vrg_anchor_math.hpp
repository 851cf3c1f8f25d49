// vrg_anchor_math.hpp -- the anchor round trip of the Video Enhance and Face Fix pipelines (csrc/vrg_anchor.hip), host and device: the
// per-pixel rules, the record checks and the launch plan.  Pinned against live Pillow and numpy by tests/test_anchor_host.py.
//   load    VRGDGVideoEnhanceLoadAnchorsMetaBatch / VRGDGFaceFixLoadAnchorsMetaBatch (_meta_image_generator of the reference): every decoded
//           R,G,B byte picture is stretched to the size of the first with Image.resize(size, LANCZOS) and becomes
//           np.asarray(image, dtype=np.float32) / 255.0, i.e. (float)byte / 255.0f by the IEEE division.  A picture that already has the
//           size is its own bytes (Pillow's resize returns a copy).  The resize is csrc/vrg_pil_resample.hpp: horizontal pass into a
//           rounded byte image, then the vertical pass; an axis whose size does not change has no pass.  The vertical sum is formed in
//           chunks of ANC_SLOTS source rows (anchor_vacc): integer adds, so any split gives Pillow's sum.  NOT built: Image.resize takes
//           a picture more than PIL_TALL_RATIO times as tall as wide, when its height shrinks, vertically first (anchor_tall); such a
//           record is refused on the host (VRG_ERR_UNSUPPORTED) and not followed by the kernel.
//   store   VRGDGVideoEnhanceStoreAnchors / VRGDGFaceFixStoreAnchors: (image[..., :3].clamp(0, 1).numpy() * 255).round().astype("uint8"),
//           the product in fp32, round half to even; R,G,B or (cv2.cvtColor(.., COLOR_RGB2BGR)) B,G,R.  torch.clamp keeps a NaN and numpy's
//           conversion of NaN to uint8 is platform-defined: x86 numpy yields 0 (cvttss2si gives 0x80000000, whose low byte is 0), so
//           ANCHOR_NAN_BYTE = 0 -- the one platform-dependent value.
#pragma once
#include "vrg_common.hpp"
#include "vrg_pil_resample.hpp"

namespace vrg {

constexpr int ANC_TW = 64, ANC_TH = 16;                   // one workgroup: 64 x 16 output pixels of one picture
constexpr int ANC_ROW_VALUES = ANC_TW * 3;
constexpr int ANC_SLOTS = 128;                            // source rows, filtered horizontally, that LDS holds at a time
constexpr int ANCHOR_RGB = 0, ANCHOR_BGR = 1;             // include/vrgdg_hip.h: VRG_ANCHOR_RGB / VRG_ANCHOR_BGR
constexpr uint8_t ANCHOR_NAN_BYTE = 0;

VRG_HD float anchor_unit(uint8_t b) { return (float)b / 255.0f; }

VRG_HD uint8_t anchor_store_byte(float x) {
    if (x != x) return ANCHOR_NAN_BYTE;
    const float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    return (uint8_t)(int32_t)__builtin_rintf(c * 255.0f);
}

// the channel of the source pixel that byte c of an output pixel takes
VRG_HD int32_t anchor_store_channel(int32_t c, int32_t order) { return order == ANCHOR_BGR ? 2 - c : c; }

struct AnchorGeom {
    int64_t src_bytes, table_ints;
    int32_t out_h, out_w;
};

// workgroups of one picture (blockIdx.x)
VRG_HD int64_t anchor_tiles(int32_t out_h, int32_t out_w) {
    return (((int64_t)out_w + ANC_TW - 1) / ANC_TW) * (((int64_t)out_h + ANC_TH - 1) / ANC_TH);
}

// the pictures Image.resize takes vertically first
VRG_HD bool anchor_tall(const vrg_anchor_desc& d, int32_t out_h) { return d.in_h > (int64_t)d.in_w * PIL_TALL_RATIO && out_h < d.in_h; }

// may the record be followed: the picture inside the byte buffer, the tables of the axes that change inside the table buffer
VRG_HD bool anchor_desc_ok(const vrg_anchor_desc& d, const AnchorGeom& g) {
    if (d.in_w < 1 || d.in_h < 1 || g.out_w < 1 || g.out_h < 1 || anchor_tall(d, g.out_h)) return false;
    if (!span_fits(d.src_offset, (int64_t)d.in_h * d.in_w * 3, g.src_bytes)) return false;
    if (d.in_w != g.out_w && (d.h_ksize < 1 || !span_fits(d.h_table, (int64_t)g.out_w * (2 + (int64_t)d.h_ksize), g.table_ints))) return false;
    if (d.in_h != g.out_h && (d.v_ksize < 1 || !span_fits(d.v_table, (int64_t)g.out_h * (2 + (int64_t)d.v_ksize), g.table_ints))) return false;
    return true;
}

// one pixel of the horizontal pass: source row `row` ([in_w][3] bytes) at output column x; the bytes themselves where the width stays
VRG_HD void anchor_hpixel(const vrg_anchor_desc& d, const AnchorGeom& g, const int32_t* tables, const uint8_t* row, int32_t x, uint8_t* o) {
    if (d.in_w == g.out_w) {
        for (int c = 0; c < 3; ++c) o[c] = row[(int64_t)x * 3 + c];
        return;
    }
    const PilRecord t = pil_record(tables + d.h_table, g.out_w, x, d.h_ksize, 0, d.in_w);
    if (!t.ok) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const uint8_t* at = row + (int64_t)t.first * 3;
    pil_taps<3>(t.w, t.n, [&](int32_t i, int c) { return at[i * 3 + c]; }, o);
}

// the part of a vertical sum that the source rows [c0, c0 + cn) hold: load(r) = the horizontally filtered byte of source row r
template <class Load>
VRG_HD int32_t anchor_vacc(int32_t acc, const PilRecord& t, int32_t c0, int32_t cn, Load load) {
    const int32_t lo = t.first > c0 ? t.first : c0, hi = t.first + t.n < c0 + cn ? t.first + t.n : c0 + cn;
    for (int32_t r = lo; r < hi; ++r) acc += (int32_t)load(r) * t.w[r - t.first];
    return acc;
}

// the source rows [r0, r1) that the output rows [y0, y0 + rows) of a picture whose height changes take their taps from
VRG_HD void anchor_tile_rows(const vrg_anchor_desc& d, const AnchorGeom& g, const int32_t* tables, int32_t y0, int32_t rows, int32_t& r0,
                             int32_t& r1) {
    r0 = d.in_h;
    r1 = 0;
    for (int32_t y = y0; y < y0 + rows; ++y) {
        const PilRecord t = pil_record(tables + d.v_table, g.out_h, y, d.v_ksize, 0, d.in_h);
        if (!t.ok) continue;
        r0 = t.first < r0 ? t.first : r0;
        r1 = t.first + t.n > r1 ? t.first + t.n : r1;
    }
    if (r1 < r0) r0 = r1 = 0;
}

// HOST.  VRG_OK, VRG_ERR_BAD_ARG for a record the kernel would not follow or a table record that leaves its axis, or
// VRG_ERR_UNSUPPORTED for a picture of anchor_tall and a frame of more tiles than a launch takes
inline int anchor_check(const vrg_anchor_desc* desc, int64_t n, const int32_t* tables, int64_t table_ints, int64_t src_bytes, int32_t out_h,
                        int32_t out_w) {
    if (n < 0 || table_ints < 0 || src_bytes < 0 || out_h < 1 || out_w < 1) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!desc || (table_ints > 0 && !tables)) return VRG_ERR_BAD_ARG;
    if (anchor_tiles(out_h, out_w) > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const AnchorGeom g{src_bytes, table_ints, out_h, out_w};
    for (int64_t i = 0; i < n; ++i) {
        const vrg_anchor_desc& d = desc[i];
        if (d.in_w >= 1 && d.in_h >= 1 && anchor_tall(d, out_h)) return VRG_ERR_UNSUPPORTED;
        if (!anchor_desc_ok(d, g)) return VRG_ERR_BAD_ARG;
        if (d.in_w != out_w)
            for (int32_t x = 0; x < out_w; ++x)
                if (!pil_record(tables + d.h_table, out_w, x, d.h_ksize, 0, d.in_w).ok) return VRG_ERR_BAD_ARG;
        if (d.in_h != out_h)
            for (int32_t y = 0; y < out_h; ++y)
                if (!pil_record(tables + d.v_table, out_h, y, d.v_ksize, 0, d.in_h).ok) return VRG_ERR_BAD_ARG;
    }
    return VRG_OK;
}

// HOST.  One record in plain loops, tile by tile and chunk by chunk as the kernel goes: out = [out_h][out_w][3] fp32
inline void anchor_frame_host(const uint8_t* src, const vrg_anchor_desc& d, const int32_t* tables, const AnchorGeom& g, float* out) {
    const uint8_t* pic = src + d.src_offset;
    const int64_t in_pitch = (int64_t)d.in_w * 3;
    uint8_t* hb = new uint8_t[(size_t)ANC_SLOTS * g.out_w * 3];
    int32_t* acc = new int32_t[(size_t)ANC_TH * g.out_w * 3];
    for (int32_t y0 = 0; y0 < g.out_h; y0 += ANC_TH) {
        const int32_t rows = g.out_h - y0 < ANC_TH ? g.out_h - y0 : ANC_TH;
        if (d.in_h == g.out_h) {
            for (int32_t ly = 0; ly < rows; ++ly)
                for (int32_t x = 0; x < g.out_w; ++x) {
                    uint8_t o[3];
                    anchor_hpixel(d, g, tables, pic + (int64_t)(y0 + ly) * in_pitch, x, o);
                    for (int c = 0; c < 3; ++c) out[((int64_t)(y0 + ly) * g.out_w + x) * 3 + c] = anchor_unit(o[c]);
                }
            continue;
        }
        int32_t r0, r1;
        anchor_tile_rows(d, g, tables, y0, rows, r0, r1);
        for (int64_t i = 0; i < (int64_t)rows * g.out_w * 3; ++i) acc[i] = 1 << (PIL_PRECISION_BITS - 1);
        for (int32_t c0 = r0; c0 < r1; c0 += ANC_SLOTS) {
            const int32_t cn = r1 - c0 < ANC_SLOTS ? r1 - c0 : ANC_SLOTS;
            for (int32_t s = 0; s < cn; ++s)
                for (int32_t x = 0; x < g.out_w; ++x) anchor_hpixel(d, g, tables, pic + (int64_t)(c0 + s) * in_pitch, x, hb + ((int64_t)s * g.out_w + x) * 3);
            for (int32_t ly = 0; ly < rows; ++ly) {
                const PilRecord t = pil_record(tables + d.v_table, g.out_h, y0 + ly, d.v_ksize, 0, d.in_h);
                if (!t.ok) continue;
                for (int32_t v = 0; v < g.out_w * 3; ++v) {
                    int32_t& a = acc[(int64_t)ly * g.out_w * 3 + v];
                    a = anchor_vacc(a, t, c0, cn, [&](int32_t r) { return hb[(int64_t)(r - c0) * g.out_w * 3 + v]; });
                }
            }
        }
        for (int32_t ly = 0; ly < rows; ++ly) {
            const bool ok = pil_record(tables + d.v_table, g.out_h, y0 + ly, d.v_ksize, 0, d.in_h).ok;
            for (int32_t v = 0; v < g.out_w * 3; ++v)
                out[(int64_t)(y0 + ly) * g.out_w * 3 + v] = anchor_unit(ok ? pil_clip8(acc[(int64_t)ly * g.out_w * 3 + v]) : (uint8_t)0);
        }
    }
    delete[] hb;
    delete[] acc;
}

// HOST.  vrg_anchor_store_u8 in plain loops: in = [pixels][channels] fp32, out = [pixels][3] bytes
inline void anchor_store_host(const float* in, int64_t pixels, int32_t channels, int32_t order, uint8_t* out) {
    for (int64_t p = 0; p < pixels; ++p)
        for (int32_t c = 0; c < 3; ++c) out[p * 3 + c] = anchor_store_byte(in[p * channels + anchor_store_channel(c, order)]);
}

// The launches of n records, one record per blockIdx.y: launch(first, count) for the chunks of the chunked launcher (launch_chunks of
// csrc/vrg_common.hpp).  Stated here, with the plan, so that the host tests walk the same chunks the kernel is launched in
// (tests/test_anchor_host.py); the seam is crossed on the GPU by tests/test_gpu_anchor.py::test_load_past_one_launch.
template <class Launch>
inline int anchor_launches(int64_t n, Launch launch) {
    return launch_chunks(n, launch);
}

}  // namespace vrg
