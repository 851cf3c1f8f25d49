// Test scaffolding: csrc/vrg_assemble_math.hpp compiled for the host (g++, -ffp-contract=off), so that the quantisation chain, the frame
// offsets and the checks of the assembly kernels are held to numpy without a GPU (tests/test_assemble_host.py).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in resize_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_assemble_math.hpp"

using namespace vrg;

extern "C" {

void hm_assemble_levels(uint8_t* q2, float* unit) {
    for (int k = 0; k < 256; ++k) {
        q2[k] = asm_q2((uint8_t)k);
        unit[k] = unit_from_u8((uint8_t)k);
    }
}

void hm_assemble_label_bytes(const float* x, int64_t n, uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = asm_label_byte(x[i]);
}

int64_t hm_assemble_frame_offset(int64_t frame, uint32_t n) { return asm_frame_offset(frame, n); }

uint32_t hm_assemble_grid_x(int64_t tiles, int64_t frames) { return asm_grid_x(tiles, frames); }

int hm_assemble_on_grid(const vrg_assemble_desc* d, const void* out_f32, const void* out_u8, int32_t labelled) {
    return asm_on_grid(d, out_f32, out_u8, labelled != 0) ? 1 : 0;
}

int hm_assemble_check(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, const void* out_f32, const void* out_u8,
                      int32_t labelled) {
    return asm_check(d, map, n_out, out_f32, out_u8, labelled);
}

int hm_assemble_join(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, float* out) {
    const int rc = asm_check(d, map, n_out, out, nullptr, 0);
    if (rc != VRG_OK) return rc;
    asm_join_host(d, map, n_out, out);
    return VRG_OK;
}

int hm_assemble_labelled(const vrg_assemble_desc* d, const vrg_assemble_entry* map, int64_t n_out, uint8_t* out) {
    const int rc = asm_check(d, map, n_out, nullptr, out, 1);
    if (rc != VRG_OK) return rc;
    asm_labelled_host(d, map, n_out, out);
    return VRG_OK;
}

}  // extern "C"
