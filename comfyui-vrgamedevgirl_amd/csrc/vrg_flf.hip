// vrg_flf.hip -- the LTX First / Last temporal guide (VRGDG_LTXFirstLastGuide.py:52-69 of the reference): two pictures, `last` centre-cropped
// and bilinearly resampled to the size of `first`, cross-faded into a batch of fp32 frames.  gfx950 only.  Arithmetic: csrc/vrg_flf_math.hpp.
//
// The output is `frames` times what is read, so the launch is bounded by its stores.  A lane owns 16 bytes of a frame -- four consecutive
// floats of the flattened [h][w][c] picture, whatever pixels and rows they belong to -- evaluates its four `first` values and its four
// resampled `last` values once, keeps them in registers and walks the FLF_CHUNK frames of its workgroup's chunk (blockIdx.x = 256 lanes of
// the picture, blockIdx.y = chunk of frames): per frame two weights (the frame index is uniform, so they are scalar loads), eight
// multiplies, four adds and one store.  A frame whose first float lies on the 16-byte grid takes one non-temporal global_store_dwordx4
// per lane; a frame that starts off it (h * w * c no multiple of 4, or an `out` that is itself off the grid) takes the same four values
// as 4-byte non-temporal stores: the choice is per frame and uniform.  The lane at the end of the picture stores its 1 .. 3 floats singly.
#include "vrg_common.hpp"
#include "vrg_flf_math.hpp"

namespace vrg {

typedef float flf_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_flf_guide(const float* __restrict__ first, const float* __restrict__ last,
                                                   const float* __restrict__ weights, float* __restrict__ out, int64_t frames, FlfGeom g) {
    const uint32_t n = (uint32_t)g.h * (uint32_t)g.w * (uint32_t)g.c;                  // <= 2^31 - 1 (flf_check)
    const uint64_t e0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (e0 >= n) return;
    const uint32_t e = (uint32_t)e0, valid = n - e < 4u ? n - e : 4u;
    const bool plain = flf_plain(g), paired = flf_paired(g);
    float a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t ek = (uint32_t)k < valid ? e + (uint32_t)k : e;                 // past the end: a value that is never stored
        a[k] = first[ek];
        b[k] = flf_last_value(g, plain, paired, ek, [&](int64_t i) { return last[i]; });
    }
    const int64_t f0 = (int64_t)blockIdx.y * FLF_CHUNK, f1 = f0 + FLF_CHUNK < frames ? f0 + FLF_CHUNK : frames;
    for (int64_t f = f0; f < f1; ++f) {
        const float w0 = weights[2 * f], w1 = weights[2 * f + 1];
        const flf_f4 v = flf_f4{flf_blend(a[0], b[0], w0, w1), flf_blend(a[1], b[1], w0, w1), flf_blend(a[2], b[2], w0, w1),
                                flf_blend(a[3], b[3], w0, w1)};
        float* frame = out + f * (int64_t)n;
        float* p = frame + e;
        if ((reinterpret_cast<uintptr_t>(frame) & 15u) == 0 && valid == 4u) {
            __builtin_nontemporal_store(v, reinterpret_cast<flf_f4*>(p));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)k < valid) __builtin_nontemporal_store(v[k], p + k);
        }
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_flf_check(int64_t frames, int32_t h, int32_t w, int32_t channels, int32_t last_h, int32_t last_w, int32_t src_x0, int32_t src_y0,
                  int32_t src_w, int32_t src_h) {
    return flf_check(frames, h, w, channels, last_h, last_w, src_x0, src_y0, src_w, src_h);
}

int vrg_flf_guide_f32(const float* first, const float* last, const float* weights, float* out, int64_t frames, int32_t h, int32_t w,
                      int32_t channels, int32_t last_h, int32_t last_w, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                      void* stream) {
    const int rc = flf_check(frames, h, w, channels, last_h, last_w, src_x0, src_y0, src_w, src_h);
    if (rc != VRG_OK) return rc;
    if (frames == 0) return VRG_OK;
    if (!first || !last || !weights || !out || out == first || out == last) return VRG_ERR_BAD_ARG;
    if (((reinterpret_cast<uintptr_t>(first) | reinterpret_cast<uintptr_t>(last) | reinterpret_cast<uintptr_t>(weights) |
          reinterpret_cast<uintptr_t>(out)) & 3u) != 0)
        return VRG_ERR_BAD_ARG;
    const FlfGeom g{h, w, channels, last_h, last_w, src_x0, src_y0, src_w, src_h};
    const int64_t lanes = ((int64_t)h * w * channels + 3) / 4;
    const dim3 grid((uint32_t)((lanes + 255) / 256), (uint32_t)((frames + FLF_CHUNK - 1) / FLF_CHUNK));
    hipLaunchKernelGGL(k_flf_guide, grid, dim3(256), 0, (hipStream_t)stream, first, last, weights, out, frames, g);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
