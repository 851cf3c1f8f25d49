// Test scaffolding: the reference-sheet arithmetic of csrc/vrg_sheet_math.hpp on the host -- the header compiled with g++
// (-ffp-contract=off): sheet_fit places the picture, pil_filter_table makes the tables, sheet_plan picks rows and segments, sheet_check
// judges the records, sheet_rows_host / sheet_compose_host evaluate a whole sheet straight from the definition.  Checked byte for byte
// against installed Pillow and the reference's recorded canvases (tests/test_sheet_host.py).  Never loaded by the package.
// With -DSHEET_CHECK_MAIN it is a stand-alone program (the sanitizer build): it reads a list of sheets from the file named on its command
// line (integers: see main), fills the sources itself and composes every sheet.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_sheet_math.hpp"

using namespace vrg;

constexpr int HM_PANEL_INTS = 10;        // source index, left, top, w, h, fit (0 contain, 1 cover, 2 resize), cell R, G, B, span offset (-1: no mask)

// one sheet.  srcs[i]: [h][w][c] of shapes[3 i ..] (fp32, or bytes when `bytes`); recs: n_panels x HM_PANEL_INTS; spans: [n_spans][2].
// details (may be null): per panel new_w, new_h, win_x, win_y, pic_w, pic_h, pic_x, pic_y, row0, rows, cps, h_ksize, v_ksize.
static int sheet_run(const void* const* srcs, const int32_t* shapes, int32_t bytes, int32_t n_panels, const int32_t* recs, const int32_t* spans,
                     int64_t n_spans, int32_t width, int32_t height, uint32_t background, uint8_t* out_u8, float* out_f32, int32_t* details) {
    std::vector<vrg_sheet_panel> panels((size_t)n_panels);
    std::vector<int32_t> tables;
    int64_t tmp_bytes = 0;
    for (int32_t i = 0; i < n_panels; ++i) {
        const int32_t* r = recs + (size_t)i * HM_PANEL_INTS;
        vrg_sheet_panel& p = panels[i];
        memset(&p, 0, sizeof(p));
        p.src = srcs[r[0]];
        p.src_h = shapes[3 * r[0]];
        p.src_w = shapes[3 * r[0] + 1];
        p.channels = shapes[3 * r[0] + 2];
        p.left = r[1];
        p.top = r[2];
        p.w = r[3];
        p.h = r[4];
        p.cell[0] = (uint8_t)r[6];
        p.cell[1] = (uint8_t)r[7];
        p.cell[2] = (uint8_t)r[8];
        p.span_offset = r[9];
        int32_t fit[SHEET_FIT_WORDS];
        if (r[5] == 2) {                                                       // the picture resized to the rectangle itself
            const int32_t whole[SHEET_FIT_WORDS] = {p.w, p.h, 0, 0, p.w, p.h, 0, 0};
            memcpy(fit, whole, sizeof(fit));
        } else {
            sheet_fit(p.src_w, p.src_h, p.w, p.h, r[5] != 0, fit);
        }
        p.new_w = fit[0]; p.new_h = fit[1]; p.win_x = fit[2]; p.win_y = fit[3];
        p.pic_w = fit[4]; p.pic_h = fit[5]; p.pic_x = fit[6]; p.pic_y = fit[7];
        for (int axis = 0; axis < 2; ++axis) {
            const int32_t n_in = axis ? p.src_h : p.src_w, n_out = axis ? p.new_h : p.new_w;
            if (n_in == n_out) continue;
            const int32_t k = pil_filter_ksize(PIL_FILTER_LANCZOS, n_in, n_out);
            const size_t at = tables.size();
            tables.resize(at + (size_t)n_out * (2 + (size_t)k));
            pil_filter_table(PIL_FILTER_LANCZOS, n_in, 0.0, n_in, n_out, tables.data() + at, tables.data() + at + 2 * (size_t)n_out);
            (axis ? p.v_table : p.h_table) = (int64_t)at;
            (axis ? p.v_ksize : p.h_ksize) = k;
        }
    }
    for (int32_t i = 0; i < n_panels; ++i) {
        vrg_sheet_panel& p = panels[i];
        if (p.win_x < 0 || p.win_y < 0 || p.win_x > p.new_w - p.pic_w || p.win_y > p.new_h - p.pic_h) return VRG_ERR_BAD_ARG;
        if (!sheet_plan(p, tables.data())) return VRG_ERR_UNSUPPORTED;
        p.tmp_offset = tmp_bytes;
        tmp_bytes += (int64_t)p.rows * p.pic_w * 3;
        if (details) {
            const int32_t d[13] = {p.new_w, p.new_h, p.win_x, p.win_y, p.pic_w, p.pic_h, p.pic_x, p.pic_y, p.row0, p.rows, p.cps, p.h_ksize, p.v_ksize};
            memcpy(details + (size_t)i * 13, d, sizeof(d));
        }
    }
    const int rc = sheet_check(panels.data(), n_panels, bytes != 0, tables.data(), (int64_t)tables.size(), n_spans, tmp_bytes);
    if (rc != VRG_OK) return rc;
    std::vector<uint8_t> tmp((size_t)tmp_bytes + 1);
    for (int32_t i = 0; i < n_panels; ++i) {
        if (bytes) sheet_rows_host<uint8_t>(panels[i], tables.data(), tmp.data());
        else sheet_rows_host<float>(panels[i], tables.data(), tmp.data());
    }
    sheet_compose_host(panels.data(), n_panels, bytes != 0, tables.data(), (int64_t)tables.size(), spans, n_spans, tmp.data(), tmp_bytes, background,
                       width, height, out_u8, out_f32);
    return VRG_OK;
}

extern "C" {

int32_t hm_sheet(const void* const* srcs, const int32_t* shapes, int32_t bytes, int32_t n_panels, const int32_t* recs, const int32_t* spans,
                 int64_t n_spans, int32_t width, int32_t height, uint32_t background, uint8_t* out_u8, float* out_f32, int32_t* details) {
    return sheet_run(srcs, shapes, bytes, n_panels, recs, spans, n_spans, width, height, background, out_u8, out_f32, details);
}

void hm_sheet_fit(int32_t src_w, int32_t src_h, int32_t w, int32_t h, int32_t cover, int32_t* fit) { sheet_fit(src_w, src_h, w, h, cover != 0, fit); }

uint8_t hm_sheet_quant(float x) { return grid_quant(x); }

void hm_sheet_units(float* out256) {
    for (int b = 0; b < 256; ++b) out256[b] = sheet_unit((uint8_t)b);
}

int32_t hm_sheet_panel_bytes() { return (int32_t)sizeof(vrg_sheet_panel); }

}  // extern "C"

#ifdef SHEET_CHECK_MAIN
// file: n_sheets, then per sheet: width height background n_src, n_src x (h w c), n_panels, n_panels x HM_PANEL_INTS, n_spans, n_spans x 2
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    auto next = [&]() {
        long long v = 0;
        if (fscanf(fh, "%lld", &v) != 1) v = -1;
        return v;
    };
    const long long sheets = next();
    uint64_t sum = 0;
    uint32_t lcg = 12345u;
    for (long long s = 0; s < sheets; ++s) {
        const int32_t width = (int32_t)next(), height = (int32_t)next();
        const uint32_t background = (uint32_t)next();
        const int32_t n_src = (int32_t)next();
        if (width < 1 || height < 1 || n_src < 1) return 3;
        std::vector<int32_t> shapes((size_t)n_src * 3);
        for (auto& v : shapes) v = (int32_t)next();
        std::vector<std::vector<float>> data((size_t)n_src);
        std::vector<const void*> srcs((size_t)n_src);
        for (int32_t i = 0; i < n_src; ++i) {
            data[i].resize((size_t)shapes[3 * i] * shapes[3 * i + 1] * shapes[3 * i + 2]);
            for (auto& v : data[i]) {
                lcg = lcg * 1664525u + 1013904223u;
                v = (float)(lcg >> 8) * (1.4f / 16777216.0f) - 0.2f;
            }
            srcs[i] = data[i].data();
        }
        const int32_t n_panels = (int32_t)next();
        std::vector<int32_t> recs((size_t)n_panels * HM_PANEL_INTS);
        for (auto& v : recs) v = (int32_t)next();
        const int32_t n_spans = (int32_t)next();
        std::vector<int32_t> spans((size_t)n_spans * 2 + 2);
        for (int32_t i = 0; i < 2 * n_spans; ++i) spans[i] = (int32_t)next();
        std::vector<uint8_t> u8((size_t)width * height * 3);
        std::vector<float> f32((size_t)width * height * 3);
        const int rc = sheet_run(srcs.data(), shapes.data(), 0, n_panels, recs.data(), spans.data(), n_spans, width, height, background, u8.data(),
                                 f32.data(), nullptr);
        if (rc != VRG_OK) {
            fprintf(stderr, "sheet %lld refused: %d\n", s, rc);
            return 4;
        }
        for (size_t i = 0; i < u8.size(); ++i) {
            if (f32[i] != (float)u8[i] / 255.0f) return 5;
            sum += u8[i];
        }
    }
    fclose(fh);
    printf("sheet_check: %lld sheets, byte sum %llu\n", sheets, (unsigned long long)sum);
    return 0;
}
#endif
