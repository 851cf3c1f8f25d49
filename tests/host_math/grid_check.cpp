// Test scaffolding: the grid-plot arithmetic of csrc/vrg_grid_math.hpp on the host -- the header compiled with g++ (-ffp-contract=off):
// grid_mode decides the rule, grid_fill_taps makes the tables, grid_resize_tile evaluates one frame into one tile straight from the
// definition.  Checked byte for byte against the independent numpy restatement of tests/grid_support.py (tests/test_grid_host.py).
// Never loaded by the package.  With -DGRID_CHECK_MAIN it is a stand-alone program (the sanitizer build).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_grid_math.hpp"

using namespace vrg;

extern "C" {

int32_t hm_grid_mode(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) { return grid_mode(in_h, in_w, out_h, out_w); }

// cells: n_out x 20 bytes
void hm_grid_taps(int32_t n_in, int32_t n_out, int32_t mode, void* cells) { grid_fill_taps(n_in, n_out, mode, reinterpret_cast<AreaCell*>(cells)); }

int32_t hm_grid_cps(int32_t n_in, int32_t n_out, int32_t mode, int32_t channels) {
    std::vector<AreaCell> cells(n_out);
    grid_fill_taps(n_in, n_out, mode, cells.data());
    return grid_cells_per_segment(cells.data(), n_out, channels);
}

void hm_grid_quant(const float* in, uint8_t* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = grid_quant(in[i]);
}

void hm_grid_unit(float* out) {
    for (int k = 0; k < 256; ++k) out[k] = grid_unit(k);
}

// in: [h][w][c] fp32 R,G,B (bytes == 0) or [h][w][3] bytes B,G,R (bytes != 0); out: [out_h][out_w][3] bytes R,G,B
void hm_grid_resize(const void* in, int32_t bytes, int32_t h, int32_t w, int32_t c, int32_t out_h, int32_t out_w, uint8_t* out) {
    const int32_t mode = grid_mode(h, w, out_h, out_w);
    std::vector<AreaCell> xc(out_w), yc(out_h);
    grid_fill_taps(w, out_w, mode, xc.data());
    grid_fill_taps(h, out_h, mode, yc.data());
    if (bytes) grid_resize_tile(reinterpret_cast<const uint8_t*>(in), h, w, c, true, out_h, out_w, xc.data(), yc.data(), mode, out);
    else grid_resize_tile(reinterpret_cast<const float*>(in), h, w, c, false, out_h, out_w, xc.data(), yc.data(), mode, out);
}

// the pairs n_out <= n_in, first_n_in <= n_in <= limit, whose general-rule cells differ between scale = 1.0 / ((double)n_out / n_in) and n_in / (double)n_out
void hm_grid_scale_pairs(int32_t first_n_in, int32_t limit, int64_t* count, int32_t* first_in, int32_t* first_out) {
    *count = 0;
    *first_in = *first_out = 0;
    for (int32_t n_in = first_n_in < 1 ? 1 : first_n_in; n_in <= limit; ++n_in)
        for (int32_t n_out = 1; n_out <= n_in; ++n_out) {
            const double a = grid_scale(n_in, n_out), b = (double)n_in / (double)n_out;
            if (a == b) continue;
            bool differ = false;
            for (int32_t d = 0; d < n_out && !differ; ++d) {
                const AreaCell p = area_cell_scaled(d, n_in, a), q = area_cell_scaled(d, n_in, b);
                differ = p.first != q.first || p.count != q.count || p.w_first != q.w_first || p.w_mid != q.w_mid || p.w_last != q.w_last;
            }
            if (differ && (*count)++ == 0) { *first_in = n_in; *first_out = n_out; }
        }
}

}  // extern "C"

#ifdef GRID_CHECK_MAIN
// every rule once, at sizes around the table ends: for the address and undefined-behaviour sanitizers
int main() {
    static const int32_t cases[][4] = {{48, 64, 48, 64}, {96, 128, 48, 64}, {96, 192, 32, 64}, {64, 120, 32, 40}, {70, 131, 30, 57}, {67, 65, 29, 31},
                                       {7, 100, 4, 50}, {33, 17, 1, 1}, {4, 4000, 2, 64}, {8, 3840, 4, 120}, {8, 953, 8, 413}, {12, 20, 38, 64}, {5, 3, 64, 37}, {48, 20, 48, 64}, {1, 1, 3, 2}};
    uint32_t state = 12345u, sum = 0;
    for (const auto& g : cases)
        for (int32_t c = 3; c <= 4; ++c) {
            std::vector<float> in((size_t)g[0] * g[1] * c);
            std::vector<uint8_t> raw((size_t)g[0] * g[1] * 3), out((size_t)g[2] * g[3] * 3);
            for (auto& v : in) { state = state * 1664525u + 1013904223u; v = (float)(state >> 8) / 16777216.0f * 1.2f - 0.1f; }
            for (auto& v : raw) { state = state * 1664525u + 1013904223u; v = (uint8_t)(state >> 24); }
            hm_grid_resize(in.data(), 0, g[0], g[1], c, g[2], g[3], out.data());
            for (uint8_t v : out) sum += v;
            if (c == 3) {
                hm_grid_resize(raw.data(), 1, g[0], g[1], 3, g[2], g[3], out.data());
                for (uint8_t v : out) sum += v;
            }
            if (hm_grid_cps(g[1], g[3], hm_grid_mode(g[0], g[1], g[2], g[3]), c) < 1) return 1;
        }
    printf("grid_check: %u\n", sum);
    return 0;
}
#endif
