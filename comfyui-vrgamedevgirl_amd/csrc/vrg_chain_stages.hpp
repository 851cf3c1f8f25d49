// vrg_chain_stages.hpp -- the "pre" stages of the fused chain (grain, LUT, colour match) as pure
// per-pixel device functions shared by the tile / point-wise kernels (vrg_chain.hip), the statistics
// reduction and the wave-march kernel (vrg_march.hip).
#pragma once
#include "vrg_common.hpp"

namespace vrg {

// What the pre stages need per FRAME: the colour-match statistics rows and the Philox stream of the frame's noise chunk.
// Every kernel's workgroups stay inside one frame, so this is wave-uniform; it is resolved once per workgroup (the frame
// index is 64-bit, and `f % ref_frames` / `f / chunk_frames` written per pixel cost ~130 scalar instructions each that the
// compiler does not hoist out of a divergent pixel loop).
struct FrameCtx {
    float ims[6], rms[6];        // [3][2] (mean, std) of the frame / of the reference frame it is matched to
    SigmaRecip sr;               // the frame's refined reciprocals of std (vrg_pixel_math.hpp: the unscaled form of (lab - mean) / std)
    uint64_t seed, off;          // generator seed / offset of the frame's noise chunk
    uint64_t elem0;              // element index of the frame's first element inside its chunk
};

template <int STAGES>
__device__ __forceinline__ FrameCtx frame_ctx(const ChainK& D, int64_t f) {
    FrameCtx C;
    if (STAGES & VRG_STAGE_COLORMATCH) {
        const float* ims = D.cm.img_ms + f * 6;
        const float* rms = D.cm.ref_ms + (D.cm.ref_frames == 1 ? 0 : (f % D.cm.ref_frames)) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) { C.ims[i] = ims[i]; C.rms[i] = rms[i]; }
        C.sr = sigma_recip(C.ims);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) { C.ims[i] = 0.0f; C.rms[i] = 0.0f; }
        C.sr.usable = false;
        C.sr.y1[0] = C.sr.y1[1] = C.sr.y1[2] = 0.0f;
    }
    if (STAGES & VRG_STAGE_GRAIN) {
        const int64_t chunk = f / D.noise.chunk_frames;
        const int64_t fl = f - chunk * D.noise.chunk_frames;
        C.elem0 = (uint64_t)(fl * D.noise.frame_elems);
        C.seed = chunk_seed(D.noise, chunk);
        C.off = chunk_offset(D.noise, chunk);
    } else {
        C.elem0 = 0; C.seed = 0; C.off = 0;
    }
    return C;
}

// grain (with the pixel's three raw normals n) -> LUT -> colour match for a pixel of the frame described by C
// KEEP_BRANCH: clamp01_3's, for the colour match from a stored Lab image (the apply march)
template <int STAGES, bool KEEP_BRANCH = false, class MATH>
__device__ __forceinline__ void chain_apply_stages(const ChainK& D, const FrameCtx& C, const float xin[3], const float n[3], float o[3],
                                                   const MATH& PT, const f32x4* lut_nodes = nullptr) {
    float v[3] = {xin[0], xin[1], xin[2]};
    if (STAGES & VRG_STAGE_GRAIN) {
        float g[3];
        grain_pixel(v, n, D.I, D.S, D.T, g);
        v[0] = g[0]; v[1] = g[1]; v[2] = g[2];
    }
    if (STAGES & VRG_STAGE_LUT) {
        float g[3];
        if (lut_nodes) lut_pixel_nodes(D.lut, lut_nodes, v, g);      // small cube staged in LDS by the kernel (uniform choice)
        else lut_pixel(D.lut, v, g);
        v[0] = g[0]; v[1] = g[1]; v[2] = g[2];
    }
    if (STAGES & VRG_STAGE_COLORMATCH) {
        float g[3];
        if (STAGES & VRG_STAGE_FROM_LAB)
            colormatch_from_lab<KEEP_BRANCH>(v, C.ims, C.rms, D.cm.K, D.cm.T, g, PT, &C.sr);     // the input pixel is already Lab
        else
            colormatch_pixel(v, C.ims, C.rms, D.cm.K, D.cm.T, g, PT, &C.sr);
        v[0] = g[0]; v[1] = g[1]; v[2] = g[2];
    }
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// Same, drawing the pixel's normals with the general per-element routine (one Philox call per element):
// for pixel p of the frame described by C.
template <int STAGES, class MATH>
__device__ __forceinline__ void chain_pre(const ChainK& D, const FrameCtx& C, int32_t p, const float xin[3], float o[3],
                                          const MATH& PT) {
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (STAGES & VRG_STAGE_GRAIN) {
        const uint64_t li = C.elem0 + (uint64_t)p * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = torch_randn_element(C.seed, C.off, D.noise.G, li + c);
    }
    chain_apply_stages<STAGES>(D, C, xin, n, o, PT);
}

// ---- the general form of the noise mapping: a draw that torch splits ------------------------------------------------------------------
// The kernels of vrg_chain.hip take their noise source as a last argument: NoSplit (the chunks of ChainK::noise, the code above, and an
// empty argument that leaves their instantiations as they were) or a NoiseSplitK, the leaves of one randn of more than 2^29 elements.
// The leaves are not frame -- not even pixel -- aligned, so an element finds its leaf: element e of the launch lies in exactly one leaf
// (start, size, G, off) and is torch_randn_element(seed, off, G, e - start).  That costs one Philox call per element like chain_pre above;
// kernels that share a Philox call among four elements of ONE grid (the march, the produce pass, k_grain) have no such form.
struct NoSplit {};
__device__ __forceinline__ NoSplit noise_source() { return NoSplit{}; }
__device__ __forceinline__ const NoiseSplitK& noise_source(const NoiseSplitK& s) { return s; }

template <int STAGES>
__device__ __forceinline__ FrameCtx frame_ctx(const ChainK& D, int64_t f, const NoSplit&) { return frame_ctx<STAGES>(D, f); }
template <int STAGES, class MATH>
__device__ __forceinline__ void chain_pre(const ChainK& D, const FrameCtx& C, int32_t p, const float xin[3], float o[3], const MATH& PT,
                                          const NoSplit&) {
    chain_pre<STAGES>(D, C, p, xin, o, PT);
}

struct SplitFrameCtx : FrameCtx {
    int64_t base;                // element of the frame's first element inside the launch
    uint32_t G;                  // one_leaf: the grid of the leaf that holds the whole frame (seed / off / elem0 are then that leaf's)
    bool one_leaf;
};

// Resolved once per workgroup: does frame f lie inside ONE leaf?  Then seed / off / G / elem0 are workgroup-uniform and the pixel's
// normals are drawn as for an ordinary chunk; otherwise every element looks its leaf up (chain_pre below).
template <int STAGES>
__device__ __forceinline__ SplitFrameCtx frame_ctx(const ChainK& D, int64_t f, const NoiseSplitK& S) {
    SplitFrameCtx C;
    static_cast<FrameCtx&>(C) = frame_ctx<STAGES & ~VRG_STAGE_GRAIN>(D, f);
    C.base = f * D.noise.frame_elems;
    const int first = split_leaf_of(S, C.base), last = split_leaf_of(S, C.base + D.noise.frame_elems - 1);
    C.one_leaf = first == last;
    NoiseLeafK L = S.leaf[0];
#pragma unroll
    for (int i = 1; i < NOISE_LEAVES_MAX; ++i)
        if (i == first) L = S.leaf[i];          // (selects: a dynamic index would put the by-value table into scratch)
    C.seed = S.seed;
    C.off = L.off;
    C.G = L.G;
    C.elem0 = (uint64_t)(C.base - L.start);
    return C;
}

// the normal of element e of the launch
__device__ __forceinline__ float split_randn_element(const NoiseSplitK& S, int64_t e) {
    NoiseLeafK L = S.leaf[0];
#pragma unroll
    for (int i = 1; i < NOISE_LEAVES_MAX; ++i)
        if (i < S.count && S.leaf[i].start <= e) L = S.leaf[i];
    return torch_randn_element32(S.seed, L.off, L.G, (uint32_t)(e - L.start));      // inside a leaf: below 2^32, no 64-bit divide
}

template <int STAGES, class MATH>
__device__ __forceinline__ void chain_pre(const ChainK& D, const SplitFrameCtx& C, int32_t p, const float xin[3], float o[3], const MATH& PT,
                                          const NoiseSplitK& S) {
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (STAGES & VRG_STAGE_GRAIN) {
        if (C.one_leaf) {
            const uint32_t li = (uint32_t)C.elem0 + (uint32_t)p * 3u;
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = torch_randn_element32(C.seed, C.off, C.G, li + c);
        } else {
            const int64_t e = C.base + (int64_t)p * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = split_randn_element(S, e + c);       // a leaf may begin inside the pixel
        }
    }
    chain_apply_stages<STAGES>(D, C, xin, n, o, PT);
}

}  // namespace vrg
