// vrg_assemble.hip -- the music-video assembly (VRGDG_CombinevideosV2 / V3 / V5, VRGDG_PadVideoWithLastFrame, VRGDG_LoadVideos of the
// reference): up to 16 clips trimmed, padded and joined into one fp32 batch by ONE launch, and -- for V5's labelled MP4 -- the writer's
// B,G,R bytes with the 60-row label bar from the same read.  gfx950 only.  Arithmetic and checks: csrc/vrg_assemble_math.hpp.
//
// Shape of the work.  Every byte is read once and written once: a streaming copy whose only freedom is which frame goes where, and that
// is a table of (source, frame) entries in device memory, one per output frame, read as a scalar by the workgroups of that frame
// (blockIdx.y = output frame).  The 16 source base pointers travel by value in the kernel arguments.  Loads and stores carry the
// non-temporal hint (nothing is read twice, so nothing should displace what the next node wants in L2), four 16-byte loads are in flight
// per lane before the first store, and a workgroup strides over the tiles of its frame so that a launch has about ASM_TARGET_GROUPS
// workgroups whatever the frame count -- 1552 frames of 1080p would otherwise be 2.4 M workgroups of 16 KiB each.  Two routes, the same
// bits: 16-byte pieces when every base pointer and the frame size lie on the 16-byte grid, 4-byte pieces otherwise (a 5 x 7 x 3 frame,
// a clip that is a slice starting at frame 1).  fp32 clips are moved as 32-bit words, so NaN payloads, -0.0 and subnormals pass.
//
// k_assemble_labelled: a workgroup takes ASM_TILE_PX pixels at a time: 3 (or 12) coalesced loads per lane, the clean fp32 values stored
// straight from registers where a clean batch is asked for, the quantised bytes put at their B,G,R position in LDS and the tile's 3 KiB
// written out as whole dwords (bytes off the grid).  After the frame's tiles the same workgroups write the bar rows.
#include "vrg_common.hpp"
#include "vrg_assemble_math.hpp"

namespace vrg {

typedef uint32_t asm_u4 __attribute__((ext_vector_type(4)));
typedef float asm_f4 __attribute__((ext_vector_type(4)));

struct AsmK {
    const void* src[ASM_MAX_SOURCES];
    const uint8_t* overlay[ASM_MAX_SOURCES];
    int32_t frames[ASM_MAX_SOURCES];
    const vrg_assemble_entry* map;                   // of this launch: entry blockIdx.y
    float* out_f32;                                  // frame blockIdx.y of this launch, or null (labelled only)
    uint8_t* out_u8;
    int32_t n_src;
    uint32_t n;                                      // elements of a frame, <= 2^31 - 1
    uint32_t bar;                                    // bytes of a frame's bar rows (labelled)
};

// the entry of this workgroup's frame, or source -1: an entry that leaves its source is not followed
__device__ __forceinline__ vrg_assemble_entry asm_entry(const AsmK& k) {
    vrg_assemble_entry m = k.map[blockIdx.y];
    if (m.source < 0 || m.source >= k.n_src || m.frame < 0 || m.frame >= k.frames[m.source]) m.source = -1;
    return m;
}

template <bool VEC, bool U8>
__global__ __launch_bounds__(256) void k_assemble(AsmK k) {
    const vrg_assemble_entry m = asm_entry(k);
    if (m.source < 0) return;
    constexpr int DEPTH = 4;
    const uint32_t units = VEC ? k.n / 4u : k.n;
    const int64_t at = asm_frame_offset(m.frame, k.n);
    uint32_t* dst = reinterpret_cast<uint32_t*>(k.out_f32) + asm_frame_offset(blockIdx.y, k.n);
    const uint8_t* s8 = static_cast<const uint8_t*>(k.src[m.source]) + (U8 ? at : 0);
    const uint32_t* s32 = static_cast<const uint32_t*>(k.src[m.source]) + (U8 ? 0 : at);
    for (int64_t u0 = (int64_t)blockIdx.x * ASM_TILE_UNITS; u0 < units; u0 += (int64_t)gridDim.x * ASM_TILE_UNITS) {
        asm_u4 v[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            const int64_t u = u0 + threadIdx.x + i * 256;
            if (u >= units) continue;
            if (VEC && U8) {
                const uint32_t b = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(s8) + u);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[i][j] = __float_as_uint(unit_from_u8((uint8_t)(b >> (8 * j))));
            } else if (VEC) {
                v[i] = __builtin_nontemporal_load(reinterpret_cast<const asm_u4*>(s32) + u);
            } else if (U8) {
                v[i][0] = __float_as_uint(unit_from_u8(__builtin_nontemporal_load(s8 + u)));
            } else {
                v[i][0] = __builtin_nontemporal_load(s32 + u);
            }
        }
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            const int64_t u = u0 + threadIdx.x + i * 256;
            if (u >= units) continue;
            if (VEC) __builtin_nontemporal_store(v[i], reinterpret_cast<asm_u4*>(dst) + u);
            else __builtin_nontemporal_store(v[i][0], dst + u);
        }
    }
}

template <bool VEC, bool U8>
__global__ __launch_bounds__(256) void k_assemble_labelled(AsmK k) {
    constexpr int W = VEC ? 4 : 1, NV = ASM_TILE_PX * 3 / 256 / W;                      // values per piece, pieces per lane and tile
    __shared__ __attribute__((aligned(16))) uint8_t bb[ASM_TILE_PX * 3];
    const vrg_assemble_entry m = asm_entry(k);
    if (m.source < 0) return;                                                          // workgroup-uniform, as every branch around a barrier below
    const int tid = (int)threadIdx.x;
    const int64_t at = asm_frame_offset(m.frame, k.n);
    const float* s32 = static_cast<const float*>(k.src[m.source]) + (U8 ? 0 : at);
    const uint8_t* s8 = static_cast<const uint8_t*>(k.src[m.source]) + (U8 ? at : 0);
    float* clean = k.out_f32 ? k.out_f32 + asm_frame_offset(blockIdx.y, k.n) : nullptr;
    uint8_t* bytes = k.out_u8 + (int64_t)blockIdx.y * ((int64_t)k.n + k.bar);
    for (int64_t e0 = (int64_t)blockIdx.x * (ASM_TILE_PX * 3); e0 < k.n; e0 += (int64_t)gridDim.x * (ASM_TILE_PX * 3)) {
        const uint32_t valid = k.n - (uint32_t)e0 < (uint32_t)(ASM_TILE_PX * 3) ? k.n - (uint32_t)e0 : (uint32_t)(ASM_TILE_PX * 3);
        float v[NV][W];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const uint32_t el = (uint32_t)(tid + i * 256) * W;                         // VEC: valid is a multiple of 12, so a piece is whole or absent
            if (el >= valid) continue;
            if (VEC && U8) {
                const uint32_t b = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(s8 + e0 + el));
#pragma unroll
                for (int j = 0; j < W; ++j) v[i][j] = unit_from_u8((uint8_t)(b >> (8 * j)));
            } else if (VEC) {
                const asm_f4 q = __builtin_nontemporal_load(reinterpret_cast<const asm_f4*>(s32 + e0 + el));
#pragma unroll
                for (int j = 0; j < W; ++j) v[i][j] = q[j];
            } else if (U8) {
                v[i][0] = unit_from_u8(__builtin_nontemporal_load(s8 + e0 + el));
            } else {
                v[i][0] = __builtin_nontemporal_load(s32 + e0 + el);
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const uint32_t el = (uint32_t)(tid + i * 256) * W;
            if (el >= valid) continue;
            if (clean) {
                if (VEC) __builtin_nontemporal_store(asm_f4{v[i][0], v[i][1], v[i][2], v[i][3]}, reinterpret_cast<asm_f4*>(clean + e0 + el));
                else __builtin_nontemporal_store(v[i][0], clean + e0 + el);
            }
#pragma unroll
            for (int j = 0; j < W; ++j) bb[asm_bgr_position(el + j)] = asm_label_byte(v[i][j]);    // the tile starts at a pixel: el % 3 is the channel
        }
        __syncthreads();
        if (VEC) {
#pragma unroll
            for (int i = 0; i < ASM_TILE_PX * 3 / 4 / 256; ++i) {
                const uint32_t b = (uint32_t)(tid + i * 256) * 4u;
                if (b < valid) __builtin_nontemporal_store(*reinterpret_cast<const uint32_t*>(bb + b), reinterpret_cast<uint32_t*>(bytes + e0 + b));
            }
        } else {
            for (uint32_t b = (uint32_t)tid; b < valid; b += 256u) bytes[e0 + b] = bb[b];
        }
        __syncthreads();                                                               // the next tile overwrites the buffer
    }
    // the bar rows: 0, or the overlay's bytes through the second quantisation
    const uint8_t* ov = k.overlay[m.source];
    uint8_t* barp = bytes + k.n;
    if (VEC) {
        for (int64_t b = ((int64_t)blockIdx.x * 256 + tid) * 4; b < k.bar; b += (int64_t)gridDim.x * 1024) {
            uint32_t word = 0;
            if (ov) {
                const uint32_t src = *reinterpret_cast<const uint32_t*>(ov + b);
#pragma unroll
                for (int j = 0; j < 4; ++j) word |= (uint32_t)asm_q2((uint8_t)(src >> (8 * j))) << (8 * j);
            }
            __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(barp + b));
        }
    } else {
        for (int64_t b = (int64_t)blockIdx.x * 256 + tid; b < k.bar; b += (int64_t)gridDim.x * 256) barp[b] = ov ? asm_q2(ov[b]) : (uint8_t)0;
    }
}

static int asm_launch(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, float* out_f32, uint8_t* out_u8, bool labelled,
                      hipStream_t st) {
    const int rc = asm_check(d, nullptr, n_out, out_f32, out_u8, labelled ? 1 : 0);
    if (rc != VRG_OK) return rc;
    if (n_out == 0) return VRG_OK;
    if (!map || (reinterpret_cast<uintptr_t>(map) & 3u) || (labelled ? !out_u8 : !out_f32)) return VRG_ERR_BAD_ARG;
    AsmK k;
    for (int i = 0; i < ASM_MAX_SOURCES; ++i) {
        const bool on = i < d->n_src;
        k.src[i] = on ? d->src[i] : nullptr;
        k.overlay[i] = on && labelled ? d->overlay[i] : nullptr;
        k.frames[i] = on ? d->frames[i] : 0;
    }
    k.n_src = d->n_src;
    k.n = (uint32_t)((int64_t)d->height[0] * d->width[0] * d->channels[0]);
    k.bar = labelled ? (uint32_t)(ASM_BAR * (int64_t)d->width[0] * 3) : 0u;
    const bool vec = asm_on_grid(d, out_f32, out_u8, labelled), u8 = d->bytes != 0;
    const int64_t tiles = labelled ? ((int64_t)k.n + ASM_TILE_PX * 3 - 1) / (ASM_TILE_PX * 3)
                                   : ((vec ? k.n / 4u : k.n) + (int64_t)ASM_TILE_UNITS - 1) / ASM_TILE_UNITS;
    return launch_chunks(n_out, [&](int64_t f0, int64_t nf) {
        AsmK c = k;
        c.map = map + f0;
        c.out_f32 = out_f32 ? out_f32 + asm_frame_offset(f0, k.n) : nullptr;
        c.out_u8 = out_u8 ? out_u8 + f0 * ((int64_t)k.n + k.bar) : nullptr;
        const dim3 grid(asm_grid_x(tiles, n_out), (uint32_t)nf);
#define ASM_GO(KERNEL)                                                                                          \
        do {                                                                                                    \
            if (vec && u8) hipLaunchKernelGGL((KERNEL<true, true>), grid, dim3(256), 0, st, c);                 \
            else if (vec) hipLaunchKernelGGL((KERNEL<true, false>), grid, dim3(256), 0, st, c);                 \
            else if (u8) hipLaunchKernelGGL((KERNEL<false, true>), grid, dim3(256), 0, st, c);                  \
            else hipLaunchKernelGGL((KERNEL<false, false>), grid, dim3(256), 0, st, c);                         \
        } while (0)
        if (labelled) ASM_GO(k_assemble_labelled);
        else ASM_GO(k_assemble);
#undef ASM_GO
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_assemble_check(const vrg_assemble_desc* desc, const vrg_assemble_entry* map_host, int64_t n_out, const float* out_f32,
                       const uint8_t* out_u8, int32_t labelled) {
    return asm_check(desc, map_host, n_out, out_f32, out_u8, labelled);
}

int vrg_assemble_f32(const vrg_assemble_desc* desc, const vrg_assemble_entry* map, int64_t n_out, float* out, void* stream) {
    return asm_launch(desc, map, n_out, out, nullptr, false, (hipStream_t)stream);
}

int vrg_assemble_labelled_u8(const vrg_assemble_desc* desc, const vrg_assemble_entry* map, int64_t n_out, float* out_f32, uint8_t* out_u8,
                             void* stream) {
    return asm_launch(desc, map, n_out, out_f32, out_u8, true, (hipStream_t)stream);
}

}  // extern "C"
