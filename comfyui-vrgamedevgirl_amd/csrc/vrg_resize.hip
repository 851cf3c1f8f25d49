// vrg_resize.hip -- frame resize (stretch / crop to fill / letterbox / letterbox undo) and the fused Video Enhance restore
// (resize back to the source size + blend over the originals + clamp) as ONE pass over the output frames.
// Reference: VRGDG_VideoEnhanceNodes.py:54-106 (_resize_batch, _restore_batch), :394-419 (restore); arithmetic: vrg_resize_math.hpp.
//
// Shape of the work.  The restore at 4K streams 24 B per output pixel (12 read from the originals, 12 written) and reads a source
// that is 6-16x smaller and stays in L2; what it must not do is spend 16 taps x 3 channels of loads and multiply-adds on every output
// pixel.  One thread owns one output COLUMN of a strip of RS_ROWS rows and marches down it:
//   * the column's source indices and x weights depend on the column only: computed once per strip, kept in registers;
//   * a row's source rows and y weights depend on the row only: wave-uniform;
//   * the value is sum_y wy * (sum_x wx * src) with the x sum innermost, so the horizontally resampled source rows (`h`, 4 rows of
//     RGB per thread) are REUSED from one output row to the next: going up in size the tap window moves by at most one source row
//     per output row, and then only one new row is gathered (4 px3 loads, 12 multiplies, 9 adds); at 4x that is one new row every
//     fourth output row.  Same products and sums in the same order as the direct form (rs_pixel), so bit-identical to it.
// Lanes of a wave are consecutive output pixels: the stores (and the loads of the originals) are contiguous 12- or 16-byte pieces,
// non-temporal as everywhere in this library for frame data that is touched once; source loads are plain (re-read by neighbours).
// This is the bicubic kernel (the node's default).  Bilinear is not separable in torch's arithmetic (four products of weight pairs),
// nearest is one tap and area a window that moves with the pixel: they run the direct form, one pixel per thread.
#include "vrg_common.hpp"
#include "vrg_resize_math.hpp"

namespace vrg {

constexpr int RS_ROWS = 32;          // output rows per strip: priming a strip costs NT gathered rows, 4 of 12 at 4x bicubic

struct RestoreK {
    const float* originals;          // [frames][out_h][out_w][channels]
    int32_t channels;
    float s, oms;
};

// out: RESTORE ? [out_h][out_w][channels] blended over the originals : [out_h][out_w][3]
template <bool RESTORE>
__device__ __forceinline__ void rs_emit(float* __restrict__ fout, const RestoreK& r, const float* __restrict__ forig, int64_t px, const float v[3]) {
    if (!RESTORE) {
        float* o = fout + px * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(v[c], o + c);
    } else {
        const float* s = forig + px * r.channels;
        float* o = fout + px * r.channels;
        float ov[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ov[c] = __builtin_nontemporal_load(s + c);
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(rs_blend(ov[c], v[c], r.s, r.oms), o + c);
        for (int c = 3; c < r.channels; ++c) __builtin_nontemporal_store(clamp01(__builtin_nontemporal_load(s + c)), o + c);
    }
}

template <bool RESTORE>
__global__ __launch_bounds__(256) void k_resize_bicubic(const float* __restrict__ in, float* __restrict__ out, ResizeGeom g, RestoreK r) {
    constexpr int NT = 4;
    const int32_t ox = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (ox >= g.out_w) return;
    const int32_t oy0 = (int32_t)blockIdx.y * RS_ROWS;
    const int32_t oy1 = oy0 + RS_ROWS < g.out_h ? oy0 + RS_ROWS : g.out_h;
    const int64_t f = blockIdx.z;
    const int32_t oc = RESTORE ? r.channels : 3;
    const float* fin = in + f * (int64_t)g.in_h * g.in_w * g.in_c;
    float* fout = out + f * (int64_t)g.out_h * g.out_w * oc;
    const float* forig = RESTORE ? r.originals + f * (int64_t)g.out_h * g.out_w * oc : nullptr;

    const int32_t dx = ox - g.dx0;
    const bool in_x = dx >= 0 && dx < g.dw;
    const float sx = rs_scale(g.sw, g.dw), sy = rs_scale(g.sh, g.dh);
    int32_t ix[NT];
    float wx[NT];
    rs_taps(in_x ? dx : 0, sx, g.sw, ix, wx);
#pragma unroll
    for (int i = 0; i < NT; ++i) ix[i] = (g.sx0 + ix[i]) * g.in_c;        // float offset inside a source row

    auto gather = [&](int32_t y, float hrow[3]) {                        // sum_x wx * src of source row y (of the rectangle)
        const float* row = fin + (int64_t)(g.sy0 + y) * g.in_w * g.in_c;
        float v[3][NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][i] = row[ix[i] + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) hrow[c] = rs_dot<NT>(wx, v[c]);
    };

    float h[NT][3];
    int32_t hy[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        hy[j] = -1;
        h[j][0] = h[j][1] = h[j][2] = 0.0f;
    }
    for (int32_t oy = oy0; oy < oy1; ++oy) {
        const int32_t dy = oy - g.dy0;                                   // wave-uniform, like everything derived from it
        float val[3] = {0.0f, 0.0f, 0.0f};
        if (dy >= 0 && dy < g.dh) {
            int32_t iy[NT];
            float wy[NT];
            rs_taps(dy, sy, g.sh, iy, wy);
            bool same = true, shifted = true;
#pragma unroll
            for (int j = 0; j < NT; ++j) same = same && iy[j] == hy[j];
#pragma unroll
            for (int j = 0; j + 1 < NT; ++j) shifted = shifted && iy[j] == hy[j + 1];
            if (!same) {
                if (shifted) {                                           // the window moved down one source row
#pragma unroll
                    for (int j = 0; j + 1 < NT; ++j) {
                        h[j][0] = h[j + 1][0]; h[j][1] = h[j + 1][1]; h[j][2] = h[j + 1][2];
                    }
                    gather(iy[NT - 1], h[NT - 1]);
                } else {
#pragma unroll
                    for (int j = 0; j < NT; ++j) gather(iy[j], h[j]);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) hy[j] = iy[j];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float rows[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) rows[j] = h[j][c];
                val[c] = in_x ? clamp01(rs_dot<NT>(wy, rows)) : 0.0f;
            }
        }
        rs_emit<RESTORE>(fout, r, forig, (int64_t)oy * g.out_w + ox, val);
    }
}

// bilinear / nearest / area: the direct form, one output pixel per thread and row
template <bool RESTORE>
__global__ __launch_bounds__(256) void k_resize_direct(const float* __restrict__ in, float* __restrict__ out, ResizeGeom g, int32_t method, RestoreK r) {
    const int32_t ox = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (ox >= g.out_w) return;
    const int32_t oy0 = (int32_t)blockIdx.y * RS_ROWS;
    const int32_t oy1 = oy0 + RS_ROWS < g.out_h ? oy0 + RS_ROWS : g.out_h;
    const int64_t f = blockIdx.z;
    const int32_t oc = RESTORE ? r.channels : 3;
    const float* fin = in + f * (int64_t)g.in_h * g.in_w * g.in_c;
    float* fout = out + f * (int64_t)g.out_h * g.out_w * oc;
    const float* forig = RESTORE ? r.originals + f * (int64_t)g.out_h * g.out_w * oc : nullptr;
    auto load = [&](int32_t y, int32_t x, int c) { return fin[((int64_t)y * g.in_w + x) * g.in_c + c]; };
    for (int32_t oy = oy0; oy < oy1; ++oy) {
        float val[3];
        rs_pixel(g, method, ox, oy, load, val);
        rs_emit<RESTORE>(fout, r, forig, (int64_t)oy * g.out_w + ox, val);
    }
}

// the unmatched tail frames of a restore: clamp(originals, 0, 1)
__global__ __launch_bounds__(256) void k_clamp_copy(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        __builtin_nontemporal_store(clamp01(__builtin_nontemporal_load(in + i)), out + i);
}

template <bool RESTORE>
static int launch_resize(const float* in, float* out, int64_t frames, const ResizeGeom& g, int32_t method, RestoreK r, hipStream_t st) {
    const int32_t oc = RESTORE ? r.channels : 3;
    if (!rs_sizes_ok(g)) return VRG_ERR_UNSUPPORTED;
    const uint32_t bx = (uint32_t)((g.out_w + 255) / 256), by = (uint32_t)((g.out_h + RS_ROWS - 1) / RS_ROWS);
    if (by > 65535u) return VRG_ERR_UNSUPPORTED;
    const int64_t in_fe = (int64_t)g.in_h * g.in_w * g.in_c, out_fe = (int64_t)g.out_h * g.out_w * oc;
    return launch_chunks(frames, [&](int64_t f0, int64_t nf) {
        const dim3 grid(bx, by, (uint32_t)nf);
        const float* src = in + f0 * in_fe;
        float* dst = out + f0 * out_fe;
        RestoreK rk = r;
        if (RESTORE) rk.originals = r.originals + f0 * out_fe;
        if (method == RS_BICUBIC) hipLaunchKernelGGL((k_resize_bicubic<RESTORE>), grid, dim3(256), 0, st, src, dst, g, rk);
        else hipLaunchKernelGGL((k_resize_direct<RESTORE>), grid, dim3(256), 0, st, src, dst, g, method, rk);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // namespace vrg

using namespace vrg;

extern "C" int vrg_resize_f32(const float* in, float* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t in_channels,
                              int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h, int32_t out_h, int32_t out_w,
                              int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h, int32_t method, void* stream) {
    const ResizeGeom g{in_h, in_w, in_channels, src_x0, src_y0, src_w, src_h, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h};
    if (!in || !out || in == out || frames < 0 || method < 0 || method > 3 || !rs_geom_ok(g)) return VRG_ERR_BAD_ARG;
    if (vrg_ranges_overlap(in, vrg_operand_bytes(frames, (int64_t)in_h * in_w * in_channels * 4), out, vrg_operand_bytes(frames, (int64_t)out_h * out_w * 12)))
        return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    return launch_resize<false>(in, out, frames, g, method, RestoreK{nullptr, 3, 0.0f, 0.0f}, (hipStream_t)stream);
}

extern "C" int vrg_restore_f32(const float* work, const float* originals, float* out, int64_t work_frames, int64_t frames,
                               int32_t in_h, int32_t in_w, int32_t in_channels, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                               int32_t out_h, int32_t out_w, int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h,
                               int32_t channels, int32_t method, float strength, float one_minus_strength, void* stream) {
    const ResizeGeom g{in_h, in_w, in_channels, src_x0, src_y0, src_w, src_h, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h};
    if (!work || !originals || !out || out == originals || out == work || work_frames < 0 || frames < 0 || channels < 3 || method < 0 ||
        method > 3 || !rs_geom_ok(g))
        return VRG_ERR_BAD_ARG;
    const int64_t out_bytes = vrg_operand_bytes(frames, (int64_t)out_h * out_w * channels * 4);           // out and originals have one shape
    if (vrg_ranges_overlap(out, out_bytes, originals, out_bytes) ||
        vrg_ranges_overlap(out, out_bytes, work, vrg_operand_bytes(work_frames, (int64_t)in_h * in_w * in_channels * 4)))
        return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    const int64_t usable = work_frames < frames ? work_frames : frames;
    const RestoreK r{originals, channels, strength, one_minus_strength};
    hipStream_t st = (hipStream_t)stream;
    if (usable > 0) {
        const int rc = launch_resize<true>(work, out, usable, g, method, r, st);
        if (rc != VRG_OK) return rc;
    }
    if (usable < frames) {                                              // source tail preserved
        const int64_t fe = (int64_t)out_h * out_w * channels;
        const int64_t n = (frames - usable) * fe;
        const int64_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(k_clamp_copy, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, originals + usable * fe,
                           out + usable * fe, n);
        VRG_CHECK_LAUNCH();
    }
    return VRG_OK;
}
