// vrg_anchor.hip -- the anchor round trip of the Video Enhance and Face Fix pipelines: decoded anchor stills to the fp32 batch the image
// model reads (the Load Anchors nodes), and the model's fp32 output to the bytes of the PNG files (the Store Anchors nodes).  gfx950
// only.  Arithmetic, record checks and launch plan: csrc/vrg_anchor_math.hpp; Pillow's tables and passes: csrc/vrg_pil_resample.hpp.
//
//   k_anchor_tile    one workgroup = one 64 x 16 tile of one picture (blockIdx.x = tile, blockIdx.y = record; the record is uniform).
//     equal size     the picture's bytes go to LDS as they are;
//     width only     one thread = one pixel of the tile: the horizontal pass, its byte to LDS;
//     height changes thread 0 finds the source rows the tile's 16 output rows take taps from; they pass through LDS in chunks of 128
//                    rows: one thread = one (row, column) of the horizontal pass -- or of the copy, where the width stays -- into the
//                    rounded byte image Pillow keeps between its passes; then every thread adds what the chunk holds of the vertical sums
//                    of its 12 output values (registers).  The resized bytes exist in LDS only;
//     convert, store as k_msr_tile: four bytes of a tile row are one LDS dword and become four (float)byte / 255.0f; a group whose address
//                    is a multiple of 16 is one non-temporal global_store_dwordx4, any other takes 4-byte non-temporal stores.
//     LDS: 128 x 192 B of rows + 16 x 192 B of bytes = 27.0 KB: five workgroups per CU.
//   k_anchor_store   the output batch as a flat run of bytes, 16 per thread (pil_flat_plan / pil_flat_write): every 16-byte piece on the
//                    grid is one non-temporal store, whichever frames it spans -- the frames of both tensors are contiguous, so byte e of the
//                    run is channel e % 3 of pixel e / 3 and a frame seam inside a piece needs no case of its own; the bytes in front of
//                    the first boundary and behind the last piece are stored one by one by one more thread.  With three channels in
//                    R,G,B order the sixteen floats of a piece are contiguous: four non-temporal 16-byte loads where they lie on the grid.
#include "vrg_anchor_math.hpp"

namespace vrg {

typedef float anc_f4 __attribute__((ext_vector_type(4)));

struct AnchorShared {
    uint8_t hb[ANC_SLOTS][ANC_ROW_VALUES];
    uint32_t ub[ANC_TH][ANC_ROW_VALUES / 4];
    int32_t r0, r1;
};

__global__ __launch_bounds__(256) void k_anchor_tile(const uint8_t* __restrict__ src, const vrg_anchor_desc* __restrict__ desc,
                                                      const int32_t* __restrict__ tables, float* __restrict__ out, AnchorGeom g,
                                                      int32_t tiles_x) {
    __shared__ AnchorShared sh;
    const int tid = (int)threadIdx.x;
    const vrg_anchor_desc d = desc[blockIdx.y];
    if (!anchor_desc_ok(d, g)) return;                                             // uniform: the whole workgroup leaves
    const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * (uint32_t)tiles_x);
    const int32_t x0 = tx * ANC_TW, y0 = ty * ANC_TH;
    const int32_t cols = g.out_w - x0 < ANC_TW ? g.out_w - x0 : ANC_TW, rows = g.out_h - y0 < ANC_TH ? g.out_h - y0 : ANC_TH;
    uint8_t* ub = reinterpret_cast<uint8_t*>(&sh.ub[0][0]);
    const uint8_t* pic = src + d.src_offset;
    const int64_t in_pitch = (int64_t)d.in_w * 3;

    if (d.in_h == g.out_h) {
        // no vertical pass: the tile's own rows, filtered (or copied) straight into the bytes
        for (int it = tid; it < rows * ANC_TW; it += 256) {
            const int ly = it / ANC_TW, col = it - ly * ANC_TW;
            if (col < cols) anchor_hpixel(d, g, tables, pic + (int64_t)(y0 + ly) * in_pitch, x0 + col, ub + ly * ANC_ROW_VALUES + col * 3);
        }
    } else {
        if (tid == 0) {
            int32_t r0, r1;
            anchor_tile_rows(d, g, tables, y0, rows, r0, r1);
            sh.r0 = r0;
            sh.r1 = r1;
        }
        // value q = tid + 256 i of the tile's 16 x 192 values: its record and its sum stay in registers over the chunks
        constexpr int PER = ANC_TH * ANC_ROW_VALUES / 256;
        int32_t acc[PER];
        PilRecord rec[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int q = tid + 256 * i, ly = q / ANC_ROW_VALUES, v = q - ly * ANC_ROW_VALUES;
            acc[i] = 1 << (PIL_PRECISION_BITS - 1);
            rec[i] = PilRecord{0, 0, tables, false};
            if (ly < rows && v < cols * 3) rec[i] = pil_record(tables + d.v_table, g.out_h, y0 + ly, d.v_ksize, 0, d.in_h);
        }
        __syncthreads();
        const int32_t r0 = sh.r0, r1 = sh.r1;
        for (int32_t c0 = r0; c0 < r1; c0 += ANC_SLOTS) {
            const int32_t cn = r1 - c0 < ANC_SLOTS ? r1 - c0 : ANC_SLOTS;
            __syncthreads();                                                       // the previous chunk has been read
            for (int it = tid; it < cn * ANC_TW; it += 256) {
                const int slot = it / ANC_TW, col = it - slot * ANC_TW;
                if (col < cols) anchor_hpixel(d, g, tables, pic + (int64_t)(c0 + slot) * in_pitch, x0 + col, &sh.hb[slot][col * 3]);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (!rec[i].ok) continue;
                const int q = tid + 256 * i, v = q % ANC_ROW_VALUES;
                acc[i] = anchor_vacc(acc[i], rec[i], c0, cn, [&](int32_t r) { return sh.hb[r - c0][v]; });
            }
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) ub[tid + 256 * i] = rec[i].ok ? pil_clip8(acc[i]) : (uint8_t)0;
    }
    __syncthreads();

    // convert once: group q = tid + 256 i of the tile's 16 x 48 groups of four values
    constexpr int GROUPS = ANC_ROW_VALUES / 4, NG = ANC_TH * GROUPS / 256;
    float* fout = out + (int64_t)blockIdx.y * ((int64_t)g.out_h * g.out_w * 3);
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int q = tid + 256 * i, ly = q / GROUPS, j = q - ly * GROUPS;
        const uint32_t b4 = sh.ub[ly][j];
        const anc_f4 v = {anchor_unit((uint8_t)(b4 & 255u)), anchor_unit((uint8_t)((b4 >> 8) & 255u)), anchor_unit((uint8_t)((b4 >> 16) & 255u)),
                          anchor_unit((uint8_t)(b4 >> 24))};
        const int32_t left = cols * 3 - 4 * j;
        const int32_t valid = ly < rows ? (left < 0 ? 0 : (left > 4 ? 4 : left)) : 0;
        float* p = fout + ((int64_t)(y0 + ly) * g.out_w + x0) * 3 + 4 * j;
        if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            __builtin_nontemporal_store(v, reinterpret_cast<anc_f4*>(p));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < valid) __builtin_nontemporal_store(v[k], p + k);
        }
    }
}

// the bytes of the output run, in order: element e is byte e % 3 of pixel e / 3
struct AnchorStoreCursor {
    const float* __restrict__ in;
    int32_t channels, order;
    int64_t p;
    int32_t c;
    __device__ __forceinline__ void seek(int64_t e) {
        p = e / 3;
        c = (int32_t)(e - p * 3);
    }
    __device__ __forceinline__ uint8_t next() {
        const uint8_t b = anchor_store_byte(__builtin_nontemporal_load(in + p * channels + anchor_store_channel(c, order)));
        if (++c == 3) {
            c = 0;
            ++p;
        }
        return b;
    }
    __device__ __forceinline__ float unit(uint8_t b) const { return anchor_unit(b); }
};

__global__ __launch_bounds__(256) void k_anchor_store(const float* __restrict__ in, uint8_t* __restrict__ out, int64_t total, int64_t lead,
                                                       int64_t pieces, int32_t channels, int32_t order, int32_t contiguous) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (contiguous && t < pieces) {                                                // R,G,B of three channels: float e is byte e
        const int64_t e0 = lead + t * 16;
        pil_u4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const anc_f4 f = __builtin_nontemporal_load(reinterpret_cast<const anc_f4*>(in + e0) + j);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[j] |= (uint32_t)anchor_store_byte(f[k]) << (8 * k);
        }
        __builtin_nontemporal_store(v, reinterpret_cast<pil_u4*>(out + e0));
        return;
    }
    pil_flat_write(out, total, lead, pieces, t, AnchorStoreCursor{in, channels, order, 0, 0});
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_anchor_check(const vrg_anchor_desc* desc_host, int64_t n, const int32_t* tables_host, int64_t table_ints, int64_t src_bytes,
                     int32_t out_h, int32_t out_w) {
    return anchor_check(desc_host, n, tables_host, table_ints, src_bytes, out_h, out_w);
}

int vrg_anchor_frames_f32(const uint8_t* src, int64_t src_bytes, const vrg_anchor_desc* desc, int64_t n, const int32_t* tables,
                          int64_t table_ints, float* out, int32_t out_h, int32_t out_w, void* stream) {
    if (n < 0 || src_bytes < 0 || table_ints < 0 || out_h < 1 || out_w < 1) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!src || !desc || !out || (reinterpret_cast<uintptr_t>(out) & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0 ||
        (table_ints > 0 && (!tables || (reinterpret_cast<uintptr_t>(tables) & 3u) != 0)))
        return VRG_ERR_BAD_ARG;
    const int64_t tiles = anchor_tiles(out_h, out_w);
    if (tiles > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const int32_t tiles_x = (int32_t)(((int64_t)out_w + ANC_TW - 1) / ANC_TW);
    const AnchorGeom g{src_bytes, table_ints, out_h, out_w};
    const int64_t frame_values = (int64_t)out_h * out_w * 3;
    return anchor_launches(n, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL(k_anchor_tile, dim3((uint32_t)tiles, (uint32_t)count), dim3(256), 0, (hipStream_t)stream, src, desc + first, tables,
                           out + first * frame_values, g, tiles_x);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

int vrg_anchor_store_u8(const float* in, uint8_t* out, int64_t pixels, int32_t channels, int32_t order, void* stream) {
    if (pixels < 0 || channels < 3 || (order != ANCHOR_RGB && order != ANCHOR_BGR)) return VRG_ERR_BAD_ARG;
    if (pixels == 0) return VRG_OK;
    if (!in || !out || (reinterpret_cast<uintptr_t>(in) & 3u) != 0) return VRG_ERR_BAD_ARG;
    if (pixels > 0x7fffffffffffffffll / 4 / channels) return VRG_ERR_UNSUPPORTED;
    const int64_t total = pixels * 3;
    PilFlat f;
    if (!pil_flat_plan(out, 1, total, 256, f)) return VRG_ERR_UNSUPPORTED;
    const int32_t contiguous = channels == 3 && order == ANCHOR_RGB && (reinterpret_cast<uintptr_t>(in + f.lead) & 15u) == 0;
    hipLaunchKernelGGL(k_anchor_store, dim3((uint32_t)f.blocks), dim3(256), 0, (hipStream_t)stream, in, out, total, f.lead, f.pieces, channels,
                       order, contiguous);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
