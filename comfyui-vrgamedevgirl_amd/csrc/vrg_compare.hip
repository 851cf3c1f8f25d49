// vrg_compare.hip -- the Video Compare Slider's IMAGE batch as the rgb24 bytes its ffmpeg pipe takes (VRGDG_VideoCompareNode.py:63-107 of
// the reference): fp32 [pixels][channels] to bytes [pixels][3], R,G,B, further channels never read.  gfx950 only.  The per-value rule:
// csrc/vrg_compare_math.hpp; the flat run of 16-byte pieces: pil_flat_plan / pil_flat_write of csrc/vrg_pil_resample.hpp.
//
//   k_rgb24   the output batch as a flat run of bytes, 16 per thread, as k_anchor_store of csrc/vrg_anchor.hip: every 16-byte piece on the
//             grid is one non-temporal store, whichever frames it spans -- byte e of the run is channel e % 3 of pixel e / 3, so a frame
//             seam inside a piece needs no case of its own; the bytes in front of the first boundary and behind the last piece are stored
//             one by one by one more thread.  With three channels the sixteen floats of a piece are contiguous: four non-temporal 16-byte
//             loads where they lie on the grid, sixteen 4-byte ones where the source is only 4-byte aligned.  With more channels a piece
//             takes its bytes from up to six pixels (22 floats with four channels), three 4-byte loads a pixel.
#include "vrg_compare_math.hpp"
#include "vrg_pil_resample.hpp"

namespace vrg {

typedef float cmp_f4 __attribute__((ext_vector_type(4)));

// the bytes of the output run, in order: element e is channel e % 3 of pixel e / 3
struct Rgb24Cursor {
    const float* __restrict__ in;
    int32_t channels;
    int64_t p;
    int32_t c;
    __device__ __forceinline__ void seek(int64_t e) {
        p = e / 3;
        c = (int32_t)(e - p * 3);
    }
    __device__ __forceinline__ uint8_t next() {
        const uint8_t b = rgb24_byte(__builtin_nontemporal_load(in + p * channels + c));
        if (++c == 3) {
            c = 0;
            ++p;
        }
        return b;
    }
    __device__ __forceinline__ float unit(uint8_t b) const { return (float)b; }      // (a byte canvas: never asked)
};

// contiguous: three channels, float e is byte e; aligned: in + lead lies on the 16-byte grid (then so does every piece's first float)
__global__ __launch_bounds__(256) void k_rgb24(const float* __restrict__ in, uint8_t* __restrict__ out, int64_t total, int64_t lead, int64_t pieces,
                                                int32_t channels, int32_t contiguous, int32_t aligned) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (contiguous && t < pieces) {
        const int64_t e0 = lead + t * 16;
        float f[16];
        if (aligned) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const cmp_f4 q = __builtin_nontemporal_load(reinterpret_cast<const cmp_f4*>(in + e0) + j);
#pragma unroll
                for (int k = 0; k < 4; ++k) f[4 * j + k] = q[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) f[k] = __builtin_nontemporal_load(in + e0 + k);
        }
        pil_u4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k >> 2] |= (uint32_t)rgb24_byte(f[k]) << (8 * (k & 3));
        __builtin_nontemporal_store(v, reinterpret_cast<pil_u4*>(out + e0));
        return;
    }
    pil_flat_write(out, total, lead, pieces, t, Rgb24Cursor{in, channels, 0, 0});
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_rgb24_frames_u8(const float* src, uint8_t* dst, int64_t pixels, int32_t channels, void* stream) {
    if (pixels < 0 || channels < 3) return VRG_ERR_BAD_ARG;
    if (pixels == 0) return VRG_OK;
    if (!src || !dst || (reinterpret_cast<uintptr_t>(src) & 3u) != 0) return VRG_ERR_BAD_ARG;
    if (pixels > 0x7fffffffffffffffll / 4 / channels) return VRG_ERR_UNSUPPORTED;
    const int64_t total = pixels * 3;
    if (vrg_ranges_overlap(src, pixels * channels * 4, dst, total)) return VRG_ERR_BAD_ARG;
    PilFlat f;
    if (!pil_flat_plan(dst, 1, total, 256, f)) return VRG_ERR_UNSUPPORTED;
    const int32_t contiguous = channels == 3;
    const int32_t aligned = (reinterpret_cast<uintptr_t>(src + f.lead) & 15u) == 0;
    hipLaunchKernelGGL(k_rgb24, dim3((uint32_t)f.blocks), dim3(256), 0, (hipStream_t)stream, src, dst, total, f.lead, f.pieces, channels,
                       contiguous, aligned);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
