// Test scaffolding: the host side of csrc/vrg_grain_block.hpp -- grain_block (linear block index -> unit, call, segment, seed, offset,
// counter) and xcd_block (the one-contiguous-run-per-XCD remap of a padded grid) compiled with g++, as the grain kernels of
// csrc/vrg_pointwise.hip call them.  Checked against the restatement of tests/test_grain_block_host.py.  Never loaded by the package.
#include <math.h>
#include <stdint.h>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_grain_block.hpp"

using namespace vrg;

extern "C" {

int32_t hm_grain_n() { return GRAIN_N; }

// noise: seed0, seed_stride, off0, off_stride, chunk0; out [n][7]: unit, k, idx_base, valid_n, seed, off, ctr of blocks 0 .. n - 1
void hm_grain_blocks(uint32_t n, uint32_t G, uint32_t groups, const uint64_t* noise, uint64_t* out) {
    NoiseK nk{};
    nk.seed0 = noise[0]; nk.seed_stride = noise[1]; nk.off0 = noise[2]; nk.off_stride = noise[3];
    nk.chunk0 = (int64_t)noise[4];
    nk.chunk_frames = 1;
    nk.G = G;
    for (uint32_t b = 0; b < n; ++b) {
        const GrainBlock gb = grain_block(b, nk, groups);
        uint64_t* o = out + (size_t)b * 7;
        o[0] = gb.unit; o[1] = gb.k; o[2] = gb.idx_base; o[3] = gb.valid_n; o[4] = gb.seed; o[5] = gb.off; o[6] = gb.ctr;
    }
}

// out [grid]: the linear index of every block of the grid, -1 for a block that sits out
void hm_xcd_blocks(uint32_t grid, uint32_t total, int64_t* out) {
    for (uint32_t block = 0; block < grid; ++block) {
        uint32_t b = 0;
        out[block] = xcd_block(block, total, b) ? (int64_t)b : -1;
    }
}

}  // extern "C"
