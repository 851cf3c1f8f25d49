// Test scaffolding: the arithmetic of the Face Fix crop sequence (csrc/vrg_crop.hip) on the host -- csrc/vrg_resize_math.hpp compiled
// with g++ (-ffp-contract=off), rs_pixel on the box view (rs_box_geom), one record per output frame exactly as vrg_crop_resize_f32
// takes them.  Checked against the recorded digests of the reference's Prepare nodes without a GPU (tests/test_crop_host.py); the
// expected value of the GPU tests on shapes too large for a fixture.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <string.h>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_resize_math.hpp"

using namespace vrg;

extern "C" {

// rec: n_out x (src_offset, row_pitch, pixel_stride, box_w, box_h); out: [n_out][size_h][size_w][3].  A record that does not lie inside
// in_floats gives a frame of zeros, as the kernel does.
void hm_crop(const float* in, int64_t in_floats, float* out, const int64_t* rec, int64_t n_out, int32_t size_h, int32_t size_w) {
    const int64_t fe = (int64_t)size_h * size_w * 3;
    for (int64_t f = 0; f < n_out; ++f) {
        const int64_t* r = rec + f * 5;
        float* dst = out + f * fe;
        int64_t twin = -1;
        for (int64_t k = 0; k < f && twin < 0; ++k)
            if (!memcmp(rec + k * 5, r, 5 * sizeof(int64_t))) twin = k;
        if (twin >= 0) {                                                  // a hole or a prefix frame: the same record again
            memcpy(dst, out + twin * fe, fe * sizeof(float));
            continue;
        }
        const int64_t off = r[0], pitch = r[1], stride = r[2], bw = r[3], bh = r[4];
        const bool fits = off >= 0 && pitch >= 0 && stride >= 3 && bw >= 1 && bh >= 1 &&
                          off + (bh - 1) * pitch + (bw - 1) * stride + 3 <= in_floats;
        if (!fits) {
            memset(dst, 0, fe * sizeof(float));
            continue;
        }
        const ResizeGeom g = rs_box_geom((int32_t)bw, (int32_t)bh, (int32_t)stride, size_w, size_h);
        const float* box = in + off;
        auto load = [&](int32_t y, int32_t x, int c) { return box[(int64_t)y * pitch + (int64_t)x * stride + c]; };
        for (int32_t y = 0; y < size_h; ++y)
            for (int32_t x = 0; x < size_w; ++x) rs_pixel(g, RS_BICUBIC, x, y, load, dst + ((int64_t)y * size_w + x) * 3);
    }
}

}  // extern "C"
