// vrg_assemble_math.hpp -- arithmetic and checks of the music-video assembly (csrc/vrg_assemble.hip), host and device.
//
// What is restated: the pixel work of VRGDG_CombinevideosV2 / V3 (HumoAutomation.py:50-133, :892-1030), VRGDG_CombinevideosV5
// (HumoAutomationExtra2.py:309-498), VRGDG_PadVideoWithLastFrame (GeneralVideoNodes.py:1945-1987) and VRGDG_LoadVideos (nodes.py:1327-1377)
// of the reference.  Which frame of which clip becomes which output frame is planned on the host (ops.assemble_plan) and arrives as a
// table of (source, frame) entries; the joined batch is those frames, bit for bit (fp32 clips) or byte / 255 (decoded uint8 R,G,B clips,
// LoadVideos' astype(float32) / 255.0: unit_from_u8, the IEEE quotient for all 256 bytes).
//
// The labelled MP4 of V5: _add_label_bar takes (frame * 255).astype(uint8), swaps to B,G,R, puts a 60-row bar under the frame, draws the
// label, swaps back to R,G,B and divides by 255; _save_video multiplies by 255, truncates and swaps to B,G,R again for the writer.  Per
// value that is q1 = trunc(x * 255f), f = (float)q1 / 255f, q2 = trunc(f * 255f), and the two swaps leave the writer's bytes in B,G,R.
// BOTH roundings are evaluated as the reference evaluates them, not assumed away.  Enumerated (tests/test_assemble_host.py, all 256
// levels, this header on the host against numpy): with a correctly rounded quotient fl(fl(k / 255) * 255) >= k for every byte k, so
// asm_q2(k) == k and no level drops -- the chain costs a division per value and changes nothing today; it stays so that the bytes
// follow the reference's expressions rather than a theorem about them.  The bar's bytes -- 0, or the label pixels of an overlay made on
// the host -- pass through the same second quantisation.
// astype(uint8) has no clip and the C cast under it is undefined outside 0 .. 255, so parity with the reference is claimed for finite x
// with 0 <= x * 255 < 256 -- every real IMAGE.  Outside that range the rule here is this header's own: saturate to 0 / 255, NaN -> 0.
#pragma once
#include "vrg_common.hpp"

namespace vrg {

constexpr int ASM_MAX_SOURCES = VRG_ASSEMBLE_MAX_SOURCES;
constexpr int ASM_BAR = VRG_ASSEMBLE_BAR;           // rows of the label bar
constexpr int ASM_TILE_PX = 1024;                   // pixels a workgroup of the labelled kernel takes through LDS at a time
constexpr int ASM_TILE_UNITS = 1024;                // 16-byte (or, off the grid, 4-byte) pieces a workgroup of the join moves per step
constexpr int64_t ASM_TARGET_GROUPS = 8192;         // workgroups a launch aims for: 256 CUs x 8 resident x 4 rounds (cdna_hip_programming.md, Guideline 11)

// trunc(p) as a byte for p = x * 255f; the contract range is 0 <= p < 256, outside it: saturate, NaN -> 0
VRG_HD uint8_t asm_trunc_u8(float p) {
    if (p >= 256.0f) return 255;
    return p > 0.0f ? (uint8_t)(int)p : (uint8_t)0;                                    // NaN fails both tests
}
VRG_HD uint8_t asm_q1(float x) { return asm_trunc_u8(x * 255.0f); }
VRG_HD uint8_t asm_q2(uint8_t q1) { return asm_trunc_u8(unit_from_u8(q1) * 255.0f); }
VRG_HD uint8_t asm_label_byte(float x) { return asm_q2(asm_q1(x)); }

// first element of frame `frame` of a batch of `n`-element frames: 64-bit (a set of 16 x 97 frames of 1080p is 9.7 G floats)
VRG_HD int64_t asm_frame_offset(int64_t frame, uint32_t n) { return frame * (int64_t)n; }

// byte e of a frame's R,G,B stream lands at this byte of its B,G,R stream (3p + 2 - c = e + 2 - 2c)
VRG_HD uint32_t asm_bgr_position(uint32_t e) { return e + 2u - 2u * (e % 3u); }

// the x tiles of a launch of `frames` output frames whose frame has `tiles` tiles
inline uint32_t asm_grid_x(int64_t tiles, int64_t frames) {
    int64_t gx = (ASM_TARGET_GROUPS + frames - 1) / (frames > 0 ? frames : 1);
    gx = gx < 1 ? 1 : gx;
    gx = gx < tiles ? gx : tiles;
    return (uint32_t)(gx < 1 ? 1 : gx);
}

// What the launches refuse, on the host.  `map` may be null (the launches hold the table in device memory and the kernels follow no entry
// that leaves its source); out_f32 / out_u8 may be null.
inline int asm_check(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, const void* out_f32, const void* out_u8,
                     int32_t labelled) {
    if (!d || n_out < 0 || d->n_src < 1 || d->n_src > ASM_MAX_SOURCES || (d->bytes != 0 && d->bytes != 1)) return VRG_ERR_BAD_ARG;
    const int32_t h = d->height[0], w = d->width[0], c = d->channels[0];
    if (h < 1 || w < 1 || c < 1) return VRG_ERR_BAD_ARG;
    for (int i = 0; i < d->n_src; ++i) {
        if (d->height[i] != h || d->width[i] != w || d->channels[i] != c || d->frames[i] < 0) return VRG_ERR_BAD_ARG;
        if (d->frames[i] > 0 && !d->src[i]) return VRG_ERR_BAD_ARG;
        if (!d->bytes && (reinterpret_cast<uintptr_t>(d->src[i]) & 3u)) return VRG_ERR_BAD_ARG;
    }
    if (labelled && c != 3) return VRG_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out_f32) & 3u) != 0) return VRG_ERR_BAD_ARG;
    if (map)
        for (int64_t f = 0; f < n_out; ++f)
            if (map[f].source < 0 || map[f].source >= d->n_src || map[f].frame < 0 || map[f].frame >= d->frames[map[f].source])
                return VRG_ERR_BAD_ARG;
    const int64_t n = (int64_t)h * w * c, bar = (int64_t)ASM_BAR * w * 3;
    if (n > 0x7fffffff || (labelled && n + bar > 0x7fffffff)) return VRG_ERR_UNSUPPORTED;   // in-frame offsets are 32-bit, frames 64-bit
    if (n_out > 0x7fffffffffffffffll / 4 / (n + bar)) return VRG_ERR_UNSUPPORTED;
    const int64_t f32_bytes = n_out * n * 4, u8_bytes = n_out * (n + bar);
    if (vrg_ranges_overlap(out_f32, f32_bytes, out_u8, u8_bytes)) return VRG_ERR_BAD_ARG;
    for (int i = 0; i < d->n_src; ++i) {
        const int64_t src_bytes = (int64_t)d->frames[i] * n * (d->bytes ? 1 : 4);
        if (vrg_ranges_overlap(out_f32, f32_bytes, d->src[i], src_bytes) || vrg_ranges_overlap(out_u8, u8_bytes, d->src[i], src_bytes)) return VRG_ERR_BAD_ARG;
        if (labelled && (vrg_ranges_overlap(out_f32, f32_bytes, d->overlay[i], bar) || vrg_ranges_overlap(out_u8, u8_bytes, d->overlay[i], bar)))
            return VRG_ERR_BAD_ARG;
    }
    return VRG_OK;
}

// the 16-byte route: every base on the 16-byte grid and a frame a whole number of 16-byte pieces (then every frame starts on the grid)
inline bool asm_on_grid(const vrg_assemble_desc* d, const void* out_f32, const void* out_u8, bool labelled) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(out_f32) | reinterpret_cast<uintptr_t>(out_u8);
    for (int i = 0; i < d->n_src; ++i) {
        bits |= reinterpret_cast<uintptr_t>(d->src[i]);
        if (labelled) bits |= reinterpret_cast<uintptr_t>(d->overlay[i]);
    }
    const int64_t n = (int64_t)d->height[0] * d->width[0] * d->channels[0];
    return (bits & 15u) == 0 && n % 4 == 0;         // labelled: n = 3 px, so px % 4 == 0 and the byte frame (n + 180 w) is whole dwords
}

// the launches in plain loops (tests/host_math/assemble_check.cpp)
inline void asm_join_host(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, float* out) {
    const uint32_t n = (uint32_t)((int64_t)d->height[0] * d->width[0] * d->channels[0]);
    for (int64_t f = 0; f < n_out; ++f) {
        const int64_t at = asm_frame_offset(map[f].frame, n);
        uint32_t* o = reinterpret_cast<uint32_t*>(out) + asm_frame_offset(f, n);
        for (uint32_t e = 0; e < n; ++e) {
            if (d->bytes) out[asm_frame_offset(f, n) + e] = unit_from_u8(static_cast<const uint8_t*>(d->src[map[f].source])[at + e]);
            else o[e] = static_cast<const uint32_t*>(d->src[map[f].source])[at + e];
        }
    }
}

inline void asm_labelled_host(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, uint8_t* out) {
    const uint32_t n = (uint32_t)((int64_t)d->height[0] * d->width[0] * 3), bar = (uint32_t)(ASM_BAR * d->width[0] * 3);
    for (int64_t f = 0; f < n_out; ++f) {
        const int s = map[f].source;
        const int64_t at = asm_frame_offset(map[f].frame, n);
        uint8_t* o = out + f * (int64_t)(n + bar);
        for (uint32_t e = 0; e < n; ++e) {
            const float x = d->bytes ? unit_from_u8(static_cast<const uint8_t*>(d->src[s])[at + e]) : static_cast<const float*>(d->src[s])[at + e];
            o[asm_bgr_position(e)] = asm_label_byte(x);
        }
        for (uint32_t e = 0; e < bar; ++e) o[n + e] = d->overlay[s] ? asm_q2(d->overlay[s][e]) : (uint8_t)0;
    }
}

}  // namespace vrg
