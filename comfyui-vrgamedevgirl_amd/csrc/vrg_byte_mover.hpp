// vrg_byte_mover.hpp -- the one pass of the byte composites (k_ff_composite of csrc/vrg_facefix.hip, k_pil_paste of csrc/vrg_farface.hip):
// the output batch as a flat run of bytes, 16 per thread, at most one box per frame.  A piece that misses the box (nearly all of a frame)
// is one 16-byte non-temporal load and store; a piece that touches it is rebuilt byte by byte in registers; pieces that cross a frame
// boundary, end the batch or are not 16-byte aligned go byte by byte and reload the frame's record at each seam.  What a byte inside the box
// becomes is the caller's (a Policy); the geometry, the hit test and the launch arithmetic are here, host and device (tests/host_math).
#pragma once
#include "vrg_common.hpp"

namespace vrg {

struct ByteBox {
    int32_t left, top, box_w, box_h;
    int32_t W;                           // the width of the frame the box lies in
};

// do bytes r .. r + 15 of a frame of width W touch the box?  (a piece spans at most two rows unless the frame is narrower than six pixels)
VRG_HD bool byte_piece_hits(int32_t left, int32_t top, int32_t box_w, int32_t box_h, int32_t W, int32_t r) {
    const int32_t pitch = W * 3;
    const int32_t y0 = (int32_t)((uint32_t)r / (uint32_t)pitch), y1 = (int32_t)((uint32_t)(r + 15) / (uint32_t)pitch);
    if (y1 < top || y0 >= top + box_h) return false;
    if (y0 != y1) return true;
    const int32_t xs = (r - y0 * pitch) / 3, xe = (r + 15 - y0 * pitch) / 3;
    return xe >= left && xs < left + box_w;
}

VRG_HD bool byte_piece_hits(const ByteBox& b, int32_t r) { return byte_piece_hits(b.left, b.top, b.box_w, b.box_h, b.W, r); }

// byte r of the frame: false outside the box, else its pixel i of the box (row-major) and its channel c
VRG_HD bool byte_in_box(const ByteBox& b, int32_t r, int64_t& i, int32_t& c) {
    const int32_t px = (int32_t)((uint32_t)r / 3u);
    c = r - px * 3;
    const int32_t y = (int32_t)((uint32_t)px / (uint32_t)b.W), x = px - y * b.W;
    const int32_t dx = x - b.left, dy = y - b.top;
    if (dx < 0 || dx >= b.box_w || dy < 0 || dy >= b.box_h) return false;
    i = (int64_t)dy * b.box_w + dx;
    return true;
}

// what the two entry points pass to their kernel besides their own arguments
struct ByteMoverLaunch {
    int64_t frame_bytes, total;
    uint32_t blocks;                     // of 256 threads, 16 bytes each
    int32_t aligned;                     // originals and out both start on 16 bytes
};

// frames >= 1, height >= 1, width >= 1.  In-frame offsets are 32-bit (a piece may start 15 bytes before a frame's end); frames are addressed with 64.
inline int byte_mover_launch(const void* originals, const void* out, int64_t frames, int32_t height, int32_t width, ByteMoverLaunch& l) {
    l.frame_bytes = (int64_t)height * width * 3;
    if (l.frame_bytes > 0x7fffffffll - 16) return VRG_ERR_UNSUPPORTED;
    l.total = frames * l.frame_bytes;
    const int64_t blocks = ((l.total + 15) / 16 + 255) / 256;
    if (blocks > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    l.blocks = (uint32_t)blocks;
    l.aligned = ((reinterpret_cast<uintptr_t>(originals) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0 ? 1 : 0;
    return VRG_OK;
}

#if defined(__HIPCC__) || defined(__HIP__)
typedef uint32_t bmu4 __attribute__((ext_vector_type(4)));

// the per-frame state of a Policy: the frame's record, whether it is valid, and the colour shifts of its statistics
template <class Desc>
struct MoverFrame {
    Desc d;
    bool ok, matched;
    float shift[3];
};

// The body of a mover kernel (256 threads, thread = 16 bytes of `total`).  Policy:
//   typename Frame                  a MoverFrame
//   load(Frame&, f)                 reads and validates the record of frame f; no shifts yet
//   load_stats(Frame&, f)           the shifts: read only by a thread that touches the box
//   box(const Frame&)               the ByteBox of a valid record
//   byte(const Frame&, r, v)        byte r of the frame (value v in the original): what the composite leaves there
template <class Policy>
__device__ __forceinline__ void move_bytes(const Policy& p, const uint8_t* __restrict__ originals, uint8_t* __restrict__ out, int64_t frame_bytes,
                                           int64_t total, int32_t aligned) {
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (b0 >= total) return;
    int64_t f = b0 / frame_bytes;
    int32_t r = (int32_t)(b0 - f * frame_bytes);
    typename Policy::Frame fr;
    p.load(fr, f);
    const uint8_t* src = originals + b0;
    uint8_t* dst = out + b0;
    if (aligned && (int64_t)r + 16 <= frame_bytes) {
        bmu4 q = __builtin_nontemporal_load(reinterpret_cast<const bmu4*>(src));
        if (fr.ok && byte_piece_hits(p.box(fr), r)) {
            p.load_stats(fr, f);
            uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint8_t v = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                const uint8_t n = p.byte(fr, r + k, v);
                w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)n << (8 * (k & 3)));
            }
            q = bmu4{w[0], w[1], w[2], w[3]};
        }
        __builtin_nontemporal_store(q, reinterpret_cast<bmu4*>(dst));
        return;
    }
    if (fr.ok) p.load_stats(fr, f);
    for (int k = 0; k < 16 && b0 + k < total; ++k) {
        if (r >= frame_bytes) {
            r = 0;
            ++f;
            p.load(fr, f);
            if (fr.ok) p.load_stats(fr, f);
        }
        const uint8_t v = src[k];
        dst[k] = fr.ok ? p.byte(fr, r, v) : v;
        ++r;
    }
}
#endif

}  // namespace vrg
