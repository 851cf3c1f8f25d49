// vrg_farface_body.hpp -- what the far-face composite does to a chunk of the means and to a byte of the paste, wherever the original's
// pixels lie; host and device.  csrc/vrg_farface.hip calls it on whole frames (pixel p of a box lies at row pitch W inside its frame),
// csrc/vrg_farface_packed.hip on dense blocks (pixel p lies at 3 p): one body, two addressings.  Arithmetic: csrc/vrg_pil_math.hpp.
//
// The means of one box are the work of one workgroup of 256 lanes, chunk by chunk of NP_CHUNK pixels:
//   np_lane_fold     a lane folds its NP_RUN consecutive pixels into six maps and stages their values (0 where not selected);
//   np_maps_merge    one step of the in-order pairwise reduction, (t) then (t + s);
//   np_chunk_end     the chunk's map applied to a sum at once, or the staged values walked with real fp32 adds.
// np_means_block strings them together with LDS and barriers on the device; tests/host_math/farface_packed_check.cpp runs the same three
// with a loop for the lanes.
//
// The packed route (frames that stay on the host, only the boxes cross the bus): where a workgroup of the paste works -- tiles, the prefix
// table, the spans of a box's blocks -- is csrc/vrg_packed_tiles.hpp, shared with the Builder's route; here is the check only this route's
// records have (pilp_blend_ok).  vrg_pil_packed_check applies the same rules on the host.
#pragma once
#include "vrg_common.hpp"
#include "vrg_packed_tiles.hpp"
#include "vrg_pil_math.hpp"

namespace vrg {

// ---------------------------------------------------------------------------------------------------------------------------------
// where pixel p (row-major inside the box) of the original lies
// ---------------------------------------------------------------------------------------------------------------------------------
struct PilFrameOrig {                     // inside a frame of row pitch W pixels; `first` = the box's first pixel
    const uint8_t* first;
    int32_t box_w, W;
    VRG_HD const uint8_t* at(int64_t p) const {
        const int32_t dy = (int32_t)(p / box_w), dx = (int32_t)(p - (int64_t)dy * box_w);
        return first + ((int64_t)dy * W + dx) * 3;
    }
};

struct PilDenseOrig {                     // a dense [box_h][box_w][3] block
    const uint8_t* first;
    VRG_HD const uint8_t* at(int64_t p) const { return first + p * 3; }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// the means, per chunk
// ---------------------------------------------------------------------------------------------------------------------------------
// lane t of 256: pixels base + t * NP_RUN ... of a box of n pixels -> m[6] (original x3, repaired x3) under the shifts sh[6], their values
// into stage[k][t * NP_RUN ...]; returns how many of them are selected
template <class Orig>
VRG_HD uint32_t np_lane_fold(const Orig& orig, const uint8_t* rep, const uint8_t* mask, int64_t n, int64_t base, int32_t t, const uint32_t* sh,
                             uint8_t (*stage)[NP_CHUNK], NpMap* m) {
    uint32_t count = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k].d[0] = m[k].d[1] = 0u;
#pragma unroll
    for (int e = 0; e < NP_RUN; ++e) {
        const int32_t i = t * NP_RUN + e;
        const int64_t p = base + i;
        uint8_t v[6] = {0, 0, 0, 0, 0, 0};
        if (p < n && mask[p] >= PIL_SELECT_FROM) {
            const uint8_t* o = orig.at(p);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = o[c];
                v[3 + c] = rep[p * 3 + c];
            }
            ++count;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            stage[k][i] = v[k];
            np_map_push(m[k], v[k], sh[k]);
        }
    }
    return count;
}

// step s (1, 2, 4 ... 128) of the reduction for lane t with t % 2s == 0: in order, (t) then (t + s)
VRG_HD void np_maps_merge(NpMap (*maps)[6], int32_t t, int32_t s, const uint32_t* sh) {
#pragma unroll
    for (int k = 0; k < 6; ++k) maps[t][k] = np_map_then(maps[t][k], maps[t + s][k], sh[k]);
}

// the sum after a chunk of `len` pixels whose reduced map is m and whose values are staged
VRG_HD uint64_t np_chunk_end(uint64_t acc, const NpMap& m, const uint8_t* staged, int32_t len) {
    if (!np_apply(acc, m, np_ulp_shift(acc))) acc = np_walk(acc, staged, len, 1);
    return acc;
}

VRG_HD int32_t np_chunk_len(int64_t n, int64_t base) { return (int32_t)(n - base < NP_CHUNK ? n - base : NP_CHUNK); }

// ---------------------------------------------------------------------------------------------------------------------------------
// the paste, per byte
// ---------------------------------------------------------------------------------------------------------------------------------
// the record of the means kernel -> matched and the three shifts
VRG_HD bool pil_read_shift(const uint32_t* rec, float* shift) {
    for (int c = 0; c < 3; ++c) shift[c] = f32_from_bits(rec[7 + c]);
    return rec[10] != 0u;
}

// one byte inside the box: the repaired byte, shifted where the box was matched, pasted over the original under the mask
VRG_HD uint8_t pil_face_byte(uint8_t original, uint8_t face, bool matched, float shift, uint8_t m) {
    if (matched) face = pil_shift_byte(face, shift);
    return pil_paste_byte(original, face, m);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the packed route: what its records need besides the blocks
// ---------------------------------------------------------------------------------------------------------------------------------
struct PilpGeom {
    int64_t n, src_bytes, rep_bytes, mask_bytes, out_bytes;
};

// what the paste needs, beyond its blocks, to paste (and the means to measure): the resized crop and the mask
VRG_HD bool pilp_blend_ok(const vrg_pil_packed_desc& d, const PilpGeom& g) {
    const int64_t px = packed_box_pixels(d);
    return px > 0 && span_fits(d.mask_offset, px, g.mask_bytes) && span_fits(d.rep_offset, px * 3, g.rep_bytes);
}

#if defined(__HIPCC__) || defined(__HIP__)
// numpy's sequential fp32 means of one box of n pixels, by one workgroup of 256 threads (all of them call, uniformly) -> rec
template <class Orig>
__device__ __forceinline__ void np_means_block(const Orig& orig, const uint8_t* __restrict__ rep, const uint8_t* __restrict__ mask, int64_t n,
                                               float strength, uint32_t* __restrict__ rec) {
    __shared__ uint8_t stage[6][NP_CHUNK];                               // the chunk's values (0 where not selected), for the walk
    __shared__ NpMap maps[256][6];
    __shared__ uint64_t acc[6];
    __shared__ uint32_t counts[4];
    const int32_t t = threadIdx.x;
    if (t < 6) acc[t] = 0ull;
    uint32_t count = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += NP_CHUNK) {
        uint32_t sh[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[k] = np_ulp_shift(acc[k]);
        NpMap m[6];
        count += np_lane_fold(orig, rep, mask, n, base, t, sh, stage, m);
#pragma unroll
        for (int k = 0; k < 6; ++k) maps[t][k] = m[k];
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            if ((t & (2 * s - 1)) == 0) np_maps_merge(maps, t, s, sh);
            __syncthreads();
        }
        if (t < 6) acc[t] = np_chunk_end(acc[t], maps[0][t], stage[t], np_chunk_len(n, base));
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) count += (uint32_t)__shfl_xor((int)count, off, 64);
    if ((t & 63) == 0) counts[t >> 6] = count;
    __syncthreads();
    if (t == 0) {
        uint64_t sums[6];
        for (int k = 0; k < 6; ++k) sums[k] = acc[k];
        uint32_t out[PIL_STATS_WORDS];
        np_finish(counts[0] + counts[1] + counts[2] + counts[3], sums, strength, out);
        for (int i = 0; i < PIL_STATS_WORDS; ++i) rec[i] = out[i];
    }
}
#endif

}  // namespace vrg
