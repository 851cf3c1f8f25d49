// vrg_msr.hip -- the LTX MSR reference frames (vrgdg_ltx_msr_reference_builder.py of the reference): a few distinct byte pictures, each
// stretched with cv2's byte Lanczos-4 and repeated into a run of fp32 / 255 frames.  gfx950 only.  Arithmetic: csrc/vrg_lanczos_math.hpp
// (integer, exact), grid_unit of csrc/vrg_grid_math.hpp, the strip planner of csrc/vrg_msr_math.hpp.
//
// The output is `repeats` times what is computed, so the launch is bounded by its stores: k_msr_tile filters a tile once and writes it
// to every frame of the descriptor's run.  One workgroup = one 64 x 32 tile of one descriptor (blockIdx.x = tile, blockIdx.y = descriptor).
// The filter is the tile filter of csrc/vrg_lanczos_tile.hpp, whose comment describes the staging and the two filter passes.
//   strips   thread 0 plans the next strip of output rows (msr_plan_strip: the distinct source rows of the strip, at most MSR_SLOTS, with
//            no gap between rows that do not overlap);
//   pass 1   every slot's source row is filtered horizontally for the tile's columns: one thread = one (slot, column);
//   pass 2   one thread = one output pixel of the strip, its taps' rows found through the slots; the bytes stay in LDS.  A picture that
//            already has the output size, or a constant colour, puts its bytes there directly;
//   convert  one thread = six groups of four consecutive values of a tile row (a row is 192 values = 48 groups): four bytes are one LDS
//            dword, each becomes (float)byte / 255.0f by the IEEE division, once;
//   store    the same 24 registers go to every frame of the run.  A group whose address is a multiple of 16 is one non-temporal
//            global_store_dwordx4 (a row of a full tile is 768 consecutive bytes); any other group -- a frame that starts off the 16-byte
//            grid because out_h * out_w * 3 is no multiple of 4, a width that is no multiple of 4, a tile's ragged end -- takes 4-byte
//            non-temporal stores.
// LDS: 40 x 3 x 64 x 4 B = 30.0 KB of sums + 6.0 KB of bytes + 2.8 KB of records and plans: four workgroups per CU.
#include "vrg_common.hpp"
#include "vrg_lanczos_tile.hpp"
#include "vrg_msr_math.hpp"

namespace vrg {

typedef float msr_f4 __attribute__((ext_vector_type(4)));

struct MsrShared {
    int32_t h[MSR_SLOTS][3][MSR_TW];
    uint32_t ub[MSR_TH][MSR_ROW_VALUES / 4];
    int32_t cs[MSR_TW], rs[MSR_TH];
    uint32_t cw[MSR_TW][4], rw[MSR_TH][4];
    int32_t slot0[MSR_TH], srcrow[MSR_SLOTS];
    int32_t strip_rows, strip_slots;
};

__global__ __launch_bounds__(256) void k_msr_tile(const vrg_msr_desc* __restrict__ desc, const uint32_t* __restrict__ taps, int64_t n_taps,
                                                   float* __restrict__ out, int64_t frames, int32_t out_h, int32_t out_w, int32_t tiles_x) {
    __shared__ MsrShared sh;
    const int tid = (int)threadIdx.x;
    const vrg_msr_desc d = desc[blockIdx.y];
    if (d.repeats < 1 || !msr_desc_ok(d, n_taps, frames, out_h, out_w)) return;            // uniform: the whole workgroup leaves
    const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * (uint32_t)tiles_x);
    const int32_t x0 = tx * MSR_TW, y0 = ty * MSR_TH;
    const int32_t cols = out_w - x0 < MSR_TW ? out_w - x0 : MSR_TW, rows = out_h - y0 < MSR_TH ? out_h - y0 : MSR_TH;
    uint8_t* ub = reinterpret_cast<uint8_t*>(&sh.ub[0][0]);

    if (!d.src || d.taps < 0) {
        // no filter: the constant colour, or the bytes of a picture that already has the output size
        const int64_t pitch = (int64_t)out_w * 3;
        const uint32_t fill = (uint32_t)d.fill[0] | (uint32_t)d.fill[1] << 8 | (uint32_t)d.fill[2] << 16;
        for (int it = tid; it < rows * MSR_ROW_VALUES; it += 256) {
            const int ly = it / MSR_ROW_VALUES, i = it - ly * MSR_ROW_VALUES;
            if (i >= cols * 3) continue;
            ub[it] = d.src ? d.src[(int64_t)(y0 + ly) * pitch + (int64_t)x0 * 3 + i] : (uint8_t)(fill >> (8 * (i % 3)));
        }
    } else {
        lz_stage_records(taps + (int64_t)d.taps * 5, x0, y0, out_w, out_h, tid, sh.cs, sh.cw, sh.rs, sh.rw);
        const int64_t in_pitch = (int64_t)d.in_w * 3;
        for (int32_t ly0 = 0; ly0 < rows;) {
            __syncthreads();                       // the records are staged; the previous strip's sums have been read
            if (tid == 0) {
                int32_t slots;
                sh.strip_rows = msr_plan_strip(sh.rs, ly0, rows, d.in_h, sh.slot0, sh.srcrow, slots);
                sh.strip_slots = slots;
            }
            __syncthreads();
            const int32_t n = sh.strip_rows, slots = sh.strip_slots;

            // pass 1: horizontal
            for (int it = tid; it < slots * MSR_TW; it += 256) {
                const int slot = it / MSR_TW, col = it - slot * MSR_TW;
                if (col >= cols) continue;
                const uint8_t* src = d.src + (int64_t)sh.srcrow[slot] * in_pitch;
                uint32_t w6[6];
                int32_t h[3];
                lz_window(src, sh.cs[col], d.in_w, w6);
                lz_hsum3(w6, sh.cw[col], h);
#pragma unroll
                for (int c = 0; c < 3; ++c) sh.h[slot][c][col] = h[c];
            }
            __syncthreads();

            // pass 2: vertical
            for (int it = tid; it < n * MSR_TW; it += 256) {
                const int ly = ly0 + it / MSR_TW, lx = it % MSR_TW;
                if (lx >= cols) continue;
                const int32_t s = sh.rs[ly], a = lz_clampi(s - 3, d.in_h - 1), first = sh.slot0[ly];
                int32_t wk[LZ_TAPS], sk[LZ_TAPS];
                lz_unpack_weights(sh.rw[ly], wk);
#pragma unroll
                for (int k = 0; k < LZ_TAPS; ++k) {
                    const int32_t slot = first + lz_clampi(s - 3 + k, d.in_h - 1) - a;
                    sk[k] = slot < 0 ? 0 : (slot > MSR_SLOTS - 1 ? MSR_SLOTS - 1 : slot);       // never taken (see msr_plan_strip)
                }
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    ub[ly * MSR_ROW_VALUES + lx * 3 + c] = lz_vsum(wk, [&](int k) { return sh.h[sk[k]][c][lx]; });
            }
            ly0 += n;
        }
    }
    __syncthreads();

    // convert once: group q = tid + 256 i of the tile's 32 x 48 groups of four values
    constexpr int GROUPS = MSR_ROW_VALUES / 4, PER = MSR_TH * GROUPS / 256;
    msr_f4 v[PER];
    int32_t valid[PER];                            // values of the group inside the picture: 0 .. 4
    int64_t at[PER];                               // the group's first value in a frame
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int q = tid + 256 * i, ly = q / GROUPS, j = q - ly * GROUPS;
        const uint32_t b4 = sh.ub[ly][j];
        v[i] = msr_f4{grid_unit((int32_t)(b4 & 255u)), grid_unit((int32_t)((b4 >> 8) & 255u)), grid_unit((int32_t)((b4 >> 16) & 255u)),
                      grid_unit((int32_t)(b4 >> 24))};
        const int32_t left = cols * 3 - 4 * j;
        valid[i] = ly < rows ? (left < 0 ? 0 : (left > 4 ? 4 : left)) : 0;
        at[i] = ((int64_t)(y0 + ly) * out_w + x0) * 3 + 4 * j;
    }
    const int64_t frame_values = (int64_t)out_h * out_w * 3;
    for (int64_t f = d.first_frame; f < (int64_t)d.first_frame + d.repeats; ++f) {
        float* fout = out + f * frame_values;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            float* p = fout + at[i];
            if (valid[i] == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                __builtin_nontemporal_store(v[i], reinterpret_cast<msr_f4*>(p));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < valid[i]) __builtin_nontemporal_store(v[i][k], p + k);
            }
        }
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_msr_check(const vrg_msr_desc* desc_host, int64_t n_desc, int64_t n_taps, int64_t frames, int32_t out_h, int32_t out_w) {
    return msr_check(desc_host, n_desc, n_taps, frames, out_h, out_w);
}

int vrg_msr_frames_f32(const vrg_msr_desc* desc, int64_t n_desc, const void* taps, int64_t n_taps, float* out, int64_t frames, int32_t out_h,
                       int32_t out_w, void* stream) {
    if (n_desc < 0 || n_taps < 0 || frames < 0 || out_h < 1 || out_w < 1) return VRG_ERR_BAD_ARG;
    if (frames == 0 || n_desc == 0) return VRG_OK;
    if (!desc || !out || (reinterpret_cast<uintptr_t>(out) & 3u) != 0 || (n_taps > 0 && (!taps || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0)))
        return VRG_ERR_BAD_ARG;
    const int64_t tiles_x = ((int64_t)out_w + MSR_TW - 1) / MSR_TW, tiles_y = ((int64_t)out_h + MSR_TH - 1) / MSR_TH;
    if (tiles_x * tiles_y > (1ll << 23)) return VRG_ERR_UNSUPPORTED;           // 2^34 pixels a frame
    return launch_chunks(n_desc, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL(k_msr_tile, dim3((uint32_t)(tiles_x * tiles_y), (uint32_t)count), dim3(256), 0, (hipStream_t)stream, desc + first,
                           reinterpret_cast<const uint32_t*>(taps), n_taps, out, frames, out_h, out_w, (int32_t)tiles_x);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // extern "C"
