// Test scaffolding: the Lanczos-4 byte resize of csrc/vrg_lanczos_math.hpp on the host -- the header compiled with g++
// (-ffp-contract=off): lz_fill_taps makes the table, lz_pixel evaluates every output pixel straight from the definition.  Checked byte for
// byte against the independent numpy restatement of tests/lanczos_support.py (tests/test_lanczos_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_lanczos_math.hpp"

using namespace vrg;

extern "C" {

// taps: (out_w + out_h) x 20 bytes, columns first
void hm_lanczos4_taps(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, void* taps) {
    lz_fill_taps(in_w, in_h, out_w, out_h, reinterpret_cast<LzTap*>(taps));
}

// in: [frames][in_h][in_w][3] bytes, out: [frames][out_h][out_w][3] bytes
void hm_lanczos4(const uint8_t* in, uint8_t* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
    std::vector<LzTap> taps((size_t)out_w + (size_t)out_h);
    lz_fill_taps(in_w, in_h, out_w, out_h, taps.data());
    for (int64_t f = 0; f < frames; ++f) {
        const uint8_t* fin = in + f * (int64_t)in_h * in_w * 3;
        uint8_t* fout = out + f * (int64_t)out_h * out_w * 3;
        auto load = [&](int32_t y, int32_t x, int c) { return fin[((int64_t)y * in_w + x) * 3 + c]; };
        for (int32_t y = 0; y < out_h; ++y)
            for (int32_t x = 0; x < out_w; ++x) lz_pixel(taps[x], taps[(size_t)out_w + y], in_w, in_h, load, fout + ((int64_t)y * out_w + x) * 3);
    }
}

}  // extern "C"
