// Test scaffolding: csrc/vrg_facefix_packed_math.hpp on the host -- the header compiled with g++: the search in the tile prefix table and
// the (record, tile) -> pixel range rule, exactly as the kernels of csrc/vrg_facefix_packed.hip call them
// (tests/test_facefix_packed_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_facefix_packed_math.hpp"

using namespace vrg;

extern "C" {

int64_t hm_ffp_find(const int64_t* prefix, int64_t n, int64_t tile) { return ffp_find(prefix, n, tile); }

int64_t hm_ffp_tiles(int32_t box_w, int32_t box_h) {
    vrg_ff_packed_desc d = {};
    d.box_w = box_w;
    d.box_h = box_h;
    return ffp_tiles(d);
}

// out: p0, count; -> 1 when `tile` is one of the record's
int32_t hm_ffp_place(int32_t box_w, int32_t box_h, int64_t first_tile, int64_t tile, int64_t* out) {
    vrg_ff_packed_desc d = {};
    d.box_w = box_w;
    d.box_h = box_h;
    int64_t p0 = -1;
    int32_t count = -1;
    const bool ok = ffp_place(d, first_tile, tile, p0, count);
    out[0] = p0;
    out[1] = count;
    return ok ? 1 : 0;
}

}  // extern "C"
