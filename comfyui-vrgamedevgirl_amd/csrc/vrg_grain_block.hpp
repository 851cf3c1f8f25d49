// vrg_grain_block.hpp -- what the shared-Philox grain kernels of vrg_pointwise.hip have in common (k_grain, k_sharpen_grain,
// k_sharpen_grain_u8, k_sharpen_grain_u8_any): the decode of a block index, the noise stage and the 3x3 window of a vector whose taps
// lie three elements away.  A block is 256 threads = GRAIN_N consecutive Philox subsequences (GRAIN_IPT per thread) of one call k of one
// unit (a noise chunk in k_grain, a frame in the fused kernels): GRAIN_N Philox calls feed the 4 x GRAIN_N elements {idx + G*(4k+ii)}.
#pragma once
#include "vrg_common.hpp"

namespace vrg {

// Host and device, and all that a plain host compiler sees of this header (tests/host_math/grain_block_check.cpp).
constexpr int GRAIN_IPT = 4;                    // subsequences per thread
constexpr int GRAIN_N = 256 * GRAIN_IPT;        // subsequences per block

struct GrainBlock {
    uint32_t unit, k;                           // chunk or frame of the launch, call of that unit
    uint32_t idx_base, valid_n;                 // first subsequence of the block, and how many of its GRAIN_N exist (a multiple of 256: whole waves)
    uint64_t seed, off, ctr;
};

// linear block index -> (unit, call, segment); groups = calls per unit = ceil(unit elements / (4 G))
VRG_HD GrainBlock grain_block(uint32_t b, const NoiseK& nk, uint32_t groups) {
    const uint32_t G = nk.G;
    const uint32_t segs = (G + GRAIN_N - 1) / GRAIN_N;
    const uint32_t per_unit = segs * groups;
    GrainBlock gb;
    gb.unit = b / per_unit;
    const uint32_t rem = b - gb.unit * per_unit;
    gb.k = rem / segs;
    gb.idx_base = (rem - gb.k * segs) * GRAIN_N;
    gb.valid_n = (G - gb.idx_base) < (uint32_t)GRAIN_N ? (G - gb.idx_base) : (uint32_t)GRAIN_N;
    gb.seed = chunk_seed(nk, gb.unit);
    gb.off = chunk_offset(nk, gb.unit);
    gb.ctr = (gb.off >> 2) + gb.k;
    return gb;
}

// workgroup `block` of a grid padded to a multiple of 8 runs on XCD block % 8: every XCD gets one contiguous run of the linear indices b.
// False for the padding blocks.
VRG_HD bool xcd_block(uint32_t block, uint32_t total_blocks, uint32_t& b) {
    const uint32_t per_xcd = (total_blocks + 7u) >> 3;
    b = (block & 7u) * per_xcd + (block >> 3);
    return (block >> 3) < per_xcd && b < total_blocks;
}

}  // namespace vrg

#if defined(__HIPCC__) || defined(__HIP__)
#include "vrg_lanes.hpp"

namespace vrg {

// Everything between the decode and a kernel's own loop (the kernel requests its frame data in between, so that the ~700 instructions of
// noise synthesis run under the HBM latency): the thread's Philox / Box-Muller rounds into nz[subsequence][ii], the block's normals
// transposed into sn[ii][4 + element of run ii], and the normals just outside the block's four runs -- HALO per side and run, at
// sn[ii][3 - d] and sn[ii][4 + valid_n + d], by the general per-element routine on 8 * HALO threads (an element's green normal is the
// element itself or a neighbour; the byte kernels reach two elements far).  numel = elements of the unit.  Every thread of the block
// must call it (barrier); returns whether the thread goes on (whole waves).
template <int HALO>
__device__ __forceinline__ bool grain_stage_normals(float (&sn)[4][GRAIN_N + 8], const GrainBlock& gb, uint32_t G, int64_t numel,
                                                    float (&nz)[GRAIN_IPT][4]) {
    const uint32_t tid = threadIdx.x, t4 = tid * GRAIN_IPT;
#pragma unroll
    for (int j = 0; j < GRAIN_IPT; ++j) {
        const u32x4 r = philox_for(gb.seed, gb.idx_base + t4 + j, gb.ctr);
        const f32x2 a = box_muller(r.x, r.y);
        const f32x2 b = box_muller(r.z, r.w);
        nz[j][0] = a.x; nz[j][1] = a.y; nz[j][2] = b.x; nz[j][3] = b.y;
    }
    if (t4 < gb.valid_n) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) *reinterpret_cast<float4*>(&sn[ii][4 + t4]) = make_float4(nz[0][ii], nz[1][ii], nz[2][ii], nz[3][ii]);
    }
    const int64_t group_base = (int64_t)4 * G * gb.k + gb.idx_base;   // unit-local element of (ii = 0, first idx)
    if (tid < 8u * HALO) {
        const int ii = (int)(tid / (2u * HALO));
        const int right = (int)((tid / HALO) & 1u), d = (int)(tid % HALO);
        const int64_t li = group_base + (int64_t)G * ii + (right ? (int64_t)gb.valid_n + d : -1 - d);
        float nv = 0.0f;
        if (li >= 0 && li < numel) nv = torch_randn_element(gb.seed, gb.off, G, (uint64_t)li);
        sn[ii][right ? 4 + gb.valid_n + d : 3 - d] = nv;
    }
    __syncthreads();
    return t4 < gb.valid_n;
}

// The 3x3 window of element kk of a four-element vector: o = the vector's three rows, pl / nr = the three elements left / right of it
template <class T>
__device__ __forceinline__ void window3(const T (&o)[3][4], const T (&pl)[3][3], const T (&nr)[3][3], int kk, T (&p)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[r][0] = kk >= 3 ? o[r][kk >= 3 ? kk - 3 : 0] : pl[r][kk < 3 ? kk : 0];
        p[r][1] = o[r][kk];
        p[r][2] = kk < 1 ? o[r][kk < 1 ? kk + 3 : 0] : nr[r][kk >= 1 ? kk - 1 : 0];
    }
}

// The rows around a thread's vector (sg4 of floats, or a dword of bytes) as loaded: halo = the neighbouring vector for lanes 0 / 63
template <class V>
struct SgRaw { V own[3], halo[3]; };

// One row of a byte kernel: the dword's four bytes and the three bytes on either side (the previous / next dword of the row come from
// the neighbouring lanes with one DPP wave shift of the raw dword each), every tap converted with the reference's own v / 255
__device__ __forceinline__ void sg_unpack_row(uint32_t own, uint32_t halo, float (&o)[4], float (&pl)[3], float (&nr)[3]) {
    const uint32_t prev = lane_prev_or(halo, own), next = lane_next_or(halo, own);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = unit_from_u8((uint8_t)(own >> (8 * i)));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pl[i] = unit_from_u8((uint8_t)(prev >> (8 * (1 + i))));   // bytes -3 + i of this dword = the previous dword's tail
        nr[i] = unit_from_u8((uint8_t)(next >> (8 * i)));         // bytes 4 + i = the next dword's head
    }
}

// Byte kk of a thread's dword from its window: run = sn[ii], at = 4 + t4 (the dword's first element in it), jj = position of the byte in
// its pixel (0 = B, 1 = G, 2 = R), stepped to the next byte's.  The byte comes back shifted into its place in the dword.
__device__ __forceinline__ uint32_t sg_pack_byte(const float (&p)[3][3], const float (&run)[GRAIN_N + 8], uint32_t at, int kk, int& jj,
                                                 float strength, bool zero, float I, float S, float T) {
    const float n_own = run[at + kk + 2 - 2 * jj];                // element 3 p + 2 - jj of byte 3 p + jj
    const float n_green = run[at + kk + 1 - jj];                  // element 3 p + 1
    const uint32_t byte = sharpen_grain_byte<true, true>(p, strength, zero ? 1 : 0, n_own, n_green, 2 - jj, I, S, T);
    jj = (jj == 2) ? 0 : jj + 1;
    return byte << (8 * kk);
}

}  // namespace vrg
#endif
