// vrg_crop.hip -- the Face Fix crop sequence: every output frame is ONE rectangle of some source frame, bicubic-resampled to the work
// size (512 x 512 in the reference) and clamped to [0, 1].  Replaces the per-frame slice / permute / F.interpolate / permute / clamp of
// both Prepare nodes, their hole filling, LTX prefix and torch.stack (VRGDG_StandaloneFaceFixNodes.py:320-351, 387-389, 486-516, 537-539).
// Arithmetic: vrg_resize_math.hpp (rs_pixel with rs_box_geom: the box is the view torch resamples, taps clamped to the BOX).
//
// Shape of the work: k_resize_bicubic's (vrg_resize.hip) with a descriptor per OUTPUT frame.  blockIdx.z is the output frame, so its
// record -- where the rectangle starts, its pitch, pixel stride and size -- is wave-uniform and arrives through scalar loads; one thread
// owns one output column of a strip of CROP_ROWS rows and marches down it with the column's taps and x weights in registers, and keeps the four
// horizontally resampled source rows from one output row to the next.  Going up (a far face: a 150-300 px box to 512) the window
// moves at most one source row per output row, so one new row is gathered every second to fourth output row; at 2x down two of the
// four rows are kept; past 4x down none is and the loop is the direct form.  Same products and sums in the same order as rs_pixel
// either way.  Two output frames may name the same rectangle (holes, the prefix): they are computed twice from the same values, so
// they are equal bit for bit.  Output stores are non-temporal, source loads plain (neighbouring columns re-read them).  No LDS.
#include "vrg_common.hpp"
#include "vrg_resize_math.hpp"

namespace vrg {

constexpr int CROP_ROWS = 32;        // output rows per strip: 512 rows = 16 strips; priming a strip costs four gathered rows

// does the rectangle lie inside [0, in_floats)?  (the caller checks the same on the host and refuses; here such a frame becomes zeros)
__device__ __forceinline__ bool crop_fits(const vrg_crop_desc& d, int64_t in_floats) {
    if (d.src_offset < 0 || d.row_pitch < 0 || d.pixel_stride < 3 || d.box_w < 1 || d.box_h < 1) return false;
    const int64_t last = d.src_offset + (int64_t)(d.box_h - 1) * d.row_pitch + (int64_t)(d.box_w - 1) * d.pixel_stride + 3;
    return (int64_t)d.box_w * d.pixel_stride <= 0x7fffffff && last <= in_floats;
}

__global__ __launch_bounds__(256) void k_crop_resize(const float* __restrict__ in, int64_t in_floats, float* __restrict__ out,
                                                     const vrg_crop_desc* __restrict__ desc, int32_t size_h, int32_t size_w) {
    constexpr int NT = 4;
    const int32_t ox = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (ox >= size_w) return;
    const int32_t oy0 = (int32_t)blockIdx.y * CROP_ROWS;
    const int32_t oy1 = oy0 + CROP_ROWS < size_h ? oy0 + CROP_ROWS : size_h;
    const vrg_crop_desc d = desc[blockIdx.z];                            // wave-uniform
    float* fout = out + (int64_t)blockIdx.z * size_h * size_w * 3;
    if (!crop_fits(d, in_floats)) {
        for (int32_t oy = oy0; oy < oy1; ++oy) {
            float* o = fout + ((int64_t)oy * size_w + ox) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(0.0f, o + c);
        }
        return;
    }
    const float* box = in + d.src_offset;
    const float sx = rs_scale(d.box_w, size_w), sy = rs_scale(d.box_h, size_h);
    int32_t ix[NT];
    float wx[NT];
    rs_taps(ox, sx, d.box_w, ix, wx);
#pragma unroll
    for (int i = 0; i < NT; ++i) ix[i] *= d.pixel_stride;                // float offset inside a row of the box

    auto gather = [&](int32_t y, float hrow[3]) {                        // sum_x wx * src of row y of the box
        const float* row = box + (int64_t)y * d.row_pitch;
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
        int32_t iy[NT];
        float wy[NT];
        rs_taps(oy, sy, d.box_h, iy, wy);                                // wave-uniform
        bool same = true, shifted = true;
#pragma unroll
        for (int j = 0; j < NT; ++j) same = same && iy[j] == hy[j];
#pragma unroll
        for (int j = 0; j + 1 < NT; ++j) shifted = shifted && iy[j] == hy[j + 1];
        if (!same) {
            if (shifted) {                                               // the window moved down one source row
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
        float* o = fout + ((int64_t)oy * size_w + ox) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float rows[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) rows[j] = h[j][c];
            __builtin_nontemporal_store(clamp01(rs_dot<NT>(wy, rows)), o + c);
        }
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" int vrg_crop_resize_f32(const float* in, int64_t in_floats, float* out, const vrg_crop_desc* desc, int64_t n_out,
                                   int32_t size_h, int32_t size_w, void* stream) {
    if (!in || !out || !desc || in == out || in_floats < 0 || n_out < 0 || size_h < 1 || size_w < 1) return VRG_ERR_BAD_ARG;
    if (vrg_ranges_overlap(in, vrg_operand_bytes(in_floats, 4), out, vrg_operand_bytes(n_out, (int64_t)size_h * size_w * 12))) return VRG_ERR_BAD_ARG;
    if (n_out == 0) return VRG_OK;
    if ((int64_t)size_h * size_w > 0x7fffffff / 4) return VRG_ERR_UNSUPPORTED;
    const uint32_t bx = (uint32_t)((size_w + 255) / 256), by = (uint32_t)((size_h + CROP_ROWS - 1) / CROP_ROWS);
    if (by > 65535u) return VRG_ERR_UNSUPPORTED;
    const int64_t out_fe = (int64_t)size_h * size_w * 3;
    return launch_chunks(n_out, [&](int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(k_crop_resize, dim3(bx, by, (uint32_t)nf), dim3(256), 0, (hipStream_t)stream, in, in_floats, out + f0 * out_fe,
                           desc + f0, size_h, size_w);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}
