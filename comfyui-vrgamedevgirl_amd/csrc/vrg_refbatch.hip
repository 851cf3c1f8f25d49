// vrg_refbatch.hip -- the multi-reference image batches (VRGDG_GeneralNodes2.py:3801-4145 of the reference): up to 50 pictures of unrelated
// sizes and channel counts, each resampled by comfy.utils.common_upscale's rule into its own place of one buffer, in one launch.  gfx950
// only.  Arithmetic: csrc/vrg_refbatch_math.hpp.
//
// The work is small and ragged, so workgroups map to (record, frame, tile) through the records' first_tile prefix: blockIdx.x is a tile
// number, a binary search over the table (wave-uniform, scalar loads) finds its record, and a 1 x 1 picture costs one workgroup whatever its
// neighbours are.  A tile is RB_TILE = 1024 consecutive floats of one flattened [h][w][c] output frame; a lane owns four of them, whatever
// pixels and rows they belong to, walks (y, x, channel) forward from its first element, evaluates the taps once per pixel and the filter
// once per channel straight from global memory, and stores 16 bytes when the frame starts on the 16-byte grid and four 4-byte values
// when it does not (the choice is per frame and uniform); the lane at the end of a frame stores its 1 .. 3 floats singly.  The method is
// uniform per workgroup.  Bicubic runs this direct form too: 16 loads a value, but neighbouring lanes share them in L1 / L2, and at
// about 1 MP a picture the sources of a call stay cache-resident -- tools/bench_refbatch.py records what it costs (profiles/refbatch.json).
// A record that breaks the rules of vrg_refbatch_check, or whose spans leave the buffers, is not followed.
#include "vrg_common.hpp"
#include "vrg_refbatch_math.hpp"

namespace vrg {

typedef float rb_f4 __attribute__((ext_vector_type(4)));

// (frame, first element) of this lane in record d; false: nothing to do
__device__ inline bool rb_place(const vrg_refbatch_desc& d, int32_t tile, int64_t& frame, uint32_t& e, uint32_t& valid) {
    const int64_t rel = (int64_t)tile - d.first_tile;
    if (rel < 0 || rel >= rb_tiles(d)) return false;
    const uint32_t n = (uint32_t)rb_dst_frame(d), per_frame = (n + RB_TILE - 1) / RB_TILE;
    frame = rel / per_frame;
    const uint64_t e0 = ((uint64_t)(rel - frame * per_frame) * 256u + threadIdx.x) * 4u;
    if (e0 >= n) return false;
    e = (uint32_t)e0;
    valid = n - e < 4u ? n - e : 4u;
    return true;
}

__global__ __launch_bounds__(256) void k_refbatch(const float* __restrict__ src_f32, int64_t src_floats, const uint8_t* __restrict__ src_u8,
                                                  int64_t src_bytes, const vrg_refbatch_desc* __restrict__ desc, int64_t n_desc,
                                                  float* __restrict__ out, int64_t out_floats) {
    const vrg_refbatch_desc d = desc[rb_find(desc, n_desc, (int32_t)blockIdx.x)];
    if (!rb_desc_fits(d, src_floats, src_bytes, out_floats)) return;
    int64_t frame;
    uint32_t e, valid;
    if (!rb_place(d, (int32_t)blockIdx.x, frame, e, valid)) return;
    const bool bytes = d.method == RB_BYTES, paired = rb_paired(d);
    const int64_t s0 = d.src_offset + frame * rb_src_frame(d);
    auto load = [&](int32_t y, int32_t x, int32_t ch) -> float {
        if (ch >= d.src_c) return 1.0f;
        const int64_t at = s0 + rb_src_index(d, y, x, ch);
        return bytes ? rb_from_byte(src_u8[at]) : src_f32[at];
    };
    const uint32_t px = e / (uint32_t)d.dst_c;
    int32_t ch = (int32_t)(e - px * (uint32_t)d.dst_c), y = (int32_t)(px / (uint32_t)d.dst_w), x = (int32_t)(px - (uint32_t)y * (uint32_t)d.dst_w);
    RbTaps t;
    rb_taps(d, y, x, t);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((uint32_t)k >= valid) break;
        v[k] = rb_value(d, paired, t, ch, load);
        if (++ch == d.dst_c && (uint32_t)k + 1 < valid) {                              // the next element opens a pixel of this frame
            ch = 0;
            if (++x == d.dst_w) x = 0, ++y;
            rb_taps(d, y, x, t);
        }
    }
    float* frame_out = out + d.dst_offset + frame * rb_dst_frame(d);
    float* p = frame_out + e;
    if ((reinterpret_cast<uintptr_t>(frame_out) & 15u) == 0 && valid == 4u) {
        __builtin_nontemporal_store(rb_f4{v[0], v[1], v[2], v[3]}, reinterpret_cast<rb_f4*>(p));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint32_t)k < valid) __builtin_nontemporal_store(v[k], p + k);
    }
}

// four bytes a lane: one 4-byte store where the frame starts on the 4-byte grid, single bytes elsewhere and at the end of a frame
__global__ __launch_bounds__(256) void k_refbatch_quantise(const float* __restrict__ src_f32, int64_t src_floats,
                                                           const vrg_refbatch_desc* __restrict__ desc, int64_t n_desc, uint8_t* __restrict__ dst,
                                                           int64_t dst_bytes) {
    const vrg_refbatch_desc d = desc[rb_find(desc, n_desc, (int32_t)blockIdx.x)];
    if (!rb_quantise_ok(d) || !rb_desc_fits(d, src_floats, 0, dst_bytes)) return;
    int64_t frame;
    uint32_t e, valid;
    if (!rb_place(d, (int32_t)blockIdx.x, frame, e, valid)) return;
    const int64_t s0 = d.src_offset + frame * rb_src_frame(d);
    const uint32_t px = e / (uint32_t)d.dst_c;
    int32_t ch = (int32_t)(e - px * (uint32_t)d.dst_c), y = (int32_t)(px / (uint32_t)d.dst_w), x = (int32_t)(px - (uint32_t)y * (uint32_t)d.dst_w);
    uint8_t q[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((uint32_t)k >= valid) break;
        q[k] = rb_quantise(src_f32[s0 + rb_src_index(d, y, x, ch)]);
        if (++ch == d.dst_c) {
            ch = 0;
            if (++x == d.dst_w) x = 0, ++y;
        }
    }
    uint8_t* frame_out = dst + d.dst_offset + frame * rb_dst_frame(d);
    uint8_t* p = frame_out + e;
    if ((reinterpret_cast<uintptr_t>(frame_out) & 3u) == 0 && valid == 4u) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint32_t)k < valid) p[k] = q[k];
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_refbatch_check(const vrg_refbatch_desc* desc_host, int64_t n, int64_t src_floats, int64_t src_bytes, int64_t out_elems) {
    return rb_check(desc_host, n, src_floats, src_bytes, out_elems);
}

int vrg_refbatch_f32(const float* src_f32, int64_t src_floats, const uint8_t* src_u8, int64_t src_bytes, const vrg_refbatch_desc* desc,
                     int64_t n, int64_t tiles, float* out, int64_t out_floats, void* stream) {
    if (n < 0 || tiles < 0 || src_floats < 0 || src_bytes < 0 || out_floats < 0) return VRG_ERR_BAD_ARG;
    if (tiles > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    if (n == 0 || tiles == 0) return VRG_OK;
    if (!desc || !out || (!src_f32 && src_floats > 0) || (!src_u8 && src_bytes > 0) || (!src_f32 && !src_u8)) return VRG_ERR_BAD_ARG;
    if (((reinterpret_cast<uintptr_t>(src_f32) | reinterpret_cast<uintptr_t>(out)) & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0)
        return VRG_ERR_BAD_ARG;
    if (reinterpret_cast<const void*>(out) == reinterpret_cast<const void*>(src_f32) ||
        reinterpret_cast<const void*>(out) == reinterpret_cast<const void*>(src_u8))
        return VRG_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_refbatch, dim3((uint32_t)tiles), dim3(256), 0, (hipStream_t)stream, src_f32, src_floats, src_u8, src_bytes, desc, n, out,
                       out_floats);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_refbatch_quantise_u8(const float* src_f32, int64_t src_floats, const vrg_refbatch_desc* desc, int64_t n, int64_t tiles, uint8_t* dst,
                             int64_t dst_bytes, void* stream) {
    if (n < 0 || tiles < 0 || src_floats < 0 || dst_bytes < 0) return VRG_ERR_BAD_ARG;
    if (tiles > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    if (n == 0 || tiles == 0) return VRG_OK;
    if (!desc || !dst || !src_f32 || (reinterpret_cast<uintptr_t>(src_f32) & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0)
        return VRG_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_refbatch_quantise, dim3((uint32_t)tiles), dim3(256), 0, (hipStream_t)stream, src_f32, src_floats, desc, n, dst, dst_bytes);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
