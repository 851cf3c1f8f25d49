// Test scaffolding: the landmark estimator's input (csrc/vrg_thumbs_math.hpp over csrc/vrg_grid_math.hpp) on the host -- the headers
// compiled with g++ (-ffp-contract=off): thumb_from_definition makes the 320 x 320 B,G,R thumbnail of one packed R,G,B byte image straight
// from the definition, thumb_plan and thumb_desc_ok are the rules of the descriptor.  Checked byte for byte against the independent numpy
// restatement of tests/grid_support.py (tests/test_landmark_input_host.py).  Never loaded by the package.  With -DTHUMBS_CHECK_MAIN it is
// a stand-alone program (the sanitizer build).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_thumbs_math.hpp"

using namespace vrg;

extern "C" {

// in: [box_h][box_w][3] bytes R,G,B; out: [320][320][3] bytes B,G,R
void hm_thumb(const uint8_t* in, int32_t box_h, int32_t box_w, uint8_t* out) { thumb_from_definition(in, box_h, box_w, out); }

int32_t hm_thumb_plan(int32_t box_h, int32_t box_w, int32_t* mode, int32_t* cps, float* inv) { return thumb_plan(box_h, box_w, *mode, *cps, *inv) ? 1 : 0; }

int32_t hm_thumb_desc_ok(const vrg_thumb_desc* d, int64_t n_bytes, int32_t has_source) { return thumb_desc_ok(*d, n_bytes, has_source != 0) ? 1 : 0; }

int32_t hm_thumb_desc_bytes() { return (int32_t)sizeof(vrg_thumb_desc); }

}  // extern "C"

#ifdef THUMBS_CHECK_MAIN
// every rule once, and the smallest and a lopsided box: for the address and undefined-behaviour sanitizers
int main() {
    static const int32_t cases[][2] = {{320, 320}, {640, 640}, {960, 1280}, {321, 321}, {333, 517}, {319, 319}, {40, 40}, {2, 2}, {2, 500}, {200, 400}, {1, 1}, {1, 5}};
    uint32_t state = 4321u, sum = 0;
    std::vector<uint8_t> out((size_t)THUMB_BYTES);
    for (const auto& g : cases) {
        std::vector<uint8_t> raw((size_t)g[0] * g[1] * 3);
        for (auto& v : raw) { state = state * 1664525u + 1013904223u; v = (uint8_t)(state >> 24); }
        hm_thumb(raw.data(), g[0], g[1], out.data());
        for (uint8_t v : out) sum += v;
        int32_t mode = 0, cps = 0;
        float inv = 0.0f;
        if (!hm_thumb_plan(g[0], g[1], &mode, &cps, &inv)) return 1;
        vrg_thumb_desc d{&d, &d, 0, 0, g[1], g[0], mode, cps, inv};
        if (!hm_thumb_desc_ok(&d, (int64_t)raw.size(), 0) || hm_thumb_desc_ok(&d, (int64_t)raw.size() - 1, 0)) return 2;
    }
    printf("thumbs_check: %u\n", sum);
    return 0;
}
#endif
