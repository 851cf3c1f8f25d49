// vrg_sheet.hip -- the reference sheets (VRGDG_LTXICIngredientsGrid.build and the three sheet builders of the AI Video Builder of the
// reference): fp32 or byte pictures quantised, shrunk with Pillow's LANCZOS and pasted as panels onto a coloured canvas, byte for byte.
// gfx950 only.  Arithmetic: csrc/vrg_sheet_math.hpp (on top of vrg_pil_resample.hpp, whose byte staging and flat piece writer the kernels
// share with the contact sheet, and vrg_grid_math.hpp).
//
// k_sheet_rows     the horizontal pass.  One workgroup = SHEET_ROWS source rows of one column segment of one panel.  Per row the 256
//                  threads read the source values the segment's taps touch ONCE with 16-byte non-temporal loads, quantise them and leave
//                  the BYTES in LDS (a 4K row of three channels is 11.5 KB; the buffer holds SHEET_STAGE_VALUES = 16 KB, so several
//                  workgroups share the 160 KB of a CU); then a thread owns window columns and walks their taps
//                  out of LDS for the three channels (pil_taps) into tmp.  A window whose source span passes the buffer goes through in
//                  `cps` columns per workgroup (sheet_plan); neighbouring segments both read the taps they share.  Rows the vertical taps
//                  of the window never touch and columns outside the window's taps are not read at all.
// k_sheet_compose  one pass over the canvas as a flat run of elements, one 16-byte piece per thread (four floats or sixteen bytes): per
//                  pixel the panels are walked from last to first (sheet_panel_at), the element is the vertical pass over tmp, the cell
//                  colour or the background (sheet_canvas_byte); SheetCursor gives pil_flat_write the elements.
#include "vrg_sheet_math.hpp"

namespace vrg {

constexpr int SHEET_THREADS = 256;
constexpr int SHEET_STAGE_BYTES = SHEET_STAGE_VALUES + 32;                    // a staged value lies at the phase of its source address

__device__ __forceinline__ uint32_t sheet_quant4(const pil_f4 v) {
    return (uint32_t)grid_quant(v.x) | ((uint32_t)grid_quant(v.y) << 8) | ((uint32_t)grid_quant(v.z) << 16) | ((uint32_t)grid_quant(v.w) << 24);
}

// n floats from src quantised into rb by the whole workgroup: value i lands at rb[ph + i], ph the returned phase (the float's index mod 4),
// so that the 16-byte loads and the LDS words they fill are both aligned; bytes go through pil_stage_bytes.  n <= SHEET_STAGE_VALUES.
__device__ __forceinline__ int sheet_stage(const float* src, int n, uint8_t* rb, int tid) {
    const int ph = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
    int head = (4 - ph) & 3;
    head = head < n ? head : n;
    const int nq = (n - head) >> 2;
    if (tid < head) rb[ph + tid] = grid_quant(src[tid]);
    const pil_f4* body = reinterpret_cast<const pil_f4*>(src + head);
    uint32_t* dst = reinterpret_cast<uint32_t*>(rb + ph + head);
    int q = tid;
    for (; q + 3 * SHEET_THREADS < nq; q += 4 * SHEET_THREADS) {                // four loads in flight per thread
        const pil_f4 v0 = __builtin_nontemporal_load(body + q), v1 = __builtin_nontemporal_load(body + q + SHEET_THREADS);
        const pil_f4 v2 = __builtin_nontemporal_load(body + q + 2 * SHEET_THREADS), v3 = __builtin_nontemporal_load(body + q + 3 * SHEET_THREADS);
        dst[q] = sheet_quant4(v0);
        dst[q + SHEET_THREADS] = sheet_quant4(v1);
        dst[q + 2 * SHEET_THREADS] = sheet_quant4(v2);
        dst[q + 3 * SHEET_THREADS] = sheet_quant4(v3);
    }
    for (; q < nq; q += SHEET_THREADS) dst[q] = sheet_quant4(__builtin_nontemporal_load(body + q));
    const int t = head + 4 * nq + tid;
    if (t < n) rb[ph + t] = grid_quant(src[t]);
    return ph;
}

__device__ __forceinline__ int sheet_stage(const uint8_t* src, int n, uint8_t* rb, int tid) { return pil_stage_bytes(src, n, rb, tid, SHEET_THREADS); }

template <typename T>
__global__ __launch_bounds__(SHEET_THREADS) void k_sheet_rows(const vrg_sheet_panel* __restrict__ panels, const int32_t* __restrict__ tables,
                                                               int64_t table_ints, uint8_t* __restrict__ tmp, int64_t tmp_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t rb[SHEET_STAGE_BYTES];
    const vrg_sheet_panel p = panels[blockIdx.z];                              // workgroup-uniform, as is every return below
    if (!sheet_panel_ok(p, sizeof(T) == 1, table_ints, 0x7fffffffffffffffll, tmp_bytes)) return;       // (the spans are the compose pass's)
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * p.cps, r0 = (int64_t)blockIdx.y * SHEET_ROWS;
    if (c0 >= p.pic_w || r0 >= p.rows) return;
    const int32_t c1 = (int32_t)(c0 + p.cps < p.pic_w ? c0 + p.cps : p.pic_w);
    const int32_t r1 = (int32_t)(r0 + SHEET_ROWS < p.rows ? r0 + SHEET_ROWS : p.rows);
    int32_t lo, hi;
    sheet_source_range(p, tables, (int32_t)c0, c1, lo, hi);
    const int C = p.channels;
    if ((int64_t)(hi - lo) * C > SHEET_STAGE_VALUES) hi = lo + SHEET_STAGE_VALUES / C;              // (never taken with sheet_plan's cps)
    const int n = (hi - lo) * C;
    // rows of tmp are source rows, or -- the vertical pass skipped -- window rows, which are source rows too (src_h == new_h)
    const T* src = reinterpret_cast<const T*>(p.src);
    for (int32_t r = (int32_t)r0; r < r1; ++r) {
        const T* row = src + ((int64_t)(p.row0 + r) * p.src_w + lo) * C;
        const int ph = sheet_stage(row, n, rb, tid);
        __syncthreads();
        const uint8_t* staged = rb + ph;
        for (int32_t col = (int32_t)c0 + tid; col < c1; col += SHEET_THREADS) {
            uint8_t o[3];
            sheet_row_pixel(p, tables, col, lo, hi, [&](int32_t x, int32_t c) { return staged[(x - lo) * C + c]; }, o);
            uint8_t* out = tmp + p.tmp_offset + ((int64_t)r * p.pic_w + col) * 3;
            out[0] = o[0];
            out[1] = o[1];
            out[2] = o[2];
        }
        __syncthreads();                                                       // the next row overwrites the buffer
    }
}

struct SheetCanvas {
    int64_t n, table_ints, n_spans, tmp_bytes, total;                          // total: elements of the canvas
    int32_t width, bytes;
    uint32_t background;
};

// the elements of the canvas for pil_flat_write; `px`, `at`: the pixel resolved last and its panel
struct SheetCursor {
    const vrg_sheet_panel* __restrict__ panels;
    const int32_t* __restrict__ tables;
    const int32_t* __restrict__ spans;
    const uint8_t* __restrict__ tmp;
    const SheetCanvas& g;
    int64_t e, px, at;

    __device__ __forceinline__ void seek(int64_t to) { e = to; }
    __device__ __forceinline__ uint8_t next() {
        const int64_t pixel = e / 3;
        const int32_t c = (int32_t)(e - pixel * 3);
        const int32_t y = (int32_t)(pixel / g.width), x = (int32_t)(pixel - (int64_t)y * g.width);
        if (pixel != px) {
            px = pixel;
            at = sheet_panel_at(panels, g.n, spans, g.n_spans, g.bytes != 0, g.table_ints, g.tmp_bytes, x, y);
        }
        ++e;
        return sheet_canvas_byte(panels, at, tables, tmp, g.background, x, y, c);
    }
    static __device__ __forceinline__ float unit(uint8_t b) { return sheet_unit(b); }
};

template <typename O>
__global__ __launch_bounds__(SHEET_THREADS) void k_sheet_compose(const vrg_sheet_panel* __restrict__ panels, const int32_t* __restrict__ tables,
                                                                  const int32_t* __restrict__ spans, const uint8_t* __restrict__ tmp,
                                                                  O* __restrict__ out, SheetCanvas g, int64_t lead, int64_t pieces) {
    pil_flat_write(out, g.total, lead, pieces, (int64_t)blockIdx.x * SHEET_THREADS + threadIdx.x,
                   SheetCursor{panels, tables, spans, tmp, g, 0, -1, -1});
}

template <typename T>
static int sheet_rows_launch(const vrg_sheet_panel* panels, int64_t n, const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes,
                             int32_t max_segments, int32_t max_rows, void* stream) {
    if (n < 0 || table_ints < 0 || tmp_bytes < 0 || max_segments < 0 || max_rows < 0) return VRG_ERR_BAD_ARG;
    if (n == 0 || max_segments == 0 || max_rows == 0) return VRG_OK;
    if (!panels || !tmp || (table_ints > 0 && !tables) || (reinterpret_cast<uintptr_t>(panels) & 7u) || (reinterpret_cast<uintptr_t>(tables) & 3u) ||
        (const void*)tmp == (const void*)panels || (const void*)tmp == (const void*)tables)
        return VRG_ERR_BAD_ARG;
    if (max_segments > SHEET_MAX_SIDE || max_rows > SHEET_MAX_SIDE) return VRG_ERR_UNSUPPORTED;
    const dim3 grid((uint32_t)max_segments, (uint32_t)((max_rows + SHEET_ROWS - 1) / SHEET_ROWS), 1);
    return launch_chunks(n, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL((k_sheet_rows<T>), dim3(grid.x, grid.y, (uint32_t)count), dim3(SHEET_THREADS), 0, (hipStream_t)stream, panels + first,
                           tables, table_ints, tmp, tmp_bytes);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

template <typename O>
static int sheet_compose_launch(const vrg_sheet_panel* panels, int64_t n, int32_t bytes, const int32_t* tables, int64_t table_ints,
                                const int32_t* spans, int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, O* out, int32_t width, int32_t height,
                                uint32_t background, void* stream) {
    if (n < 0 || table_ints < 0 || n_spans < 0 || tmp_bytes < 0) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!panels || !tmp || !out || width < 1 || height < 1 || (table_ints > 0 && !tables) || (n_spans > 0 && !spans)) return VRG_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & (sizeof(O) - 1)) || (reinterpret_cast<uintptr_t>(panels) & 7u) || (reinterpret_cast<uintptr_t>(tables) & 3u) ||
        (reinterpret_cast<uintptr_t>(spans) & 3u))
        return VRG_ERR_BAD_ARG;
    const void* o = out;
    if (o == (const void*)tmp || o == (const void*)tables || o == (const void*)spans || o == (const void*)panels) return VRG_ERR_BAD_ARG;
    if (width > SHEET_MAX_SIDE || height > SHEET_MAX_SIDE) return VRG_ERR_UNSUPPORTED;
    SheetCanvas g{n, table_ints, n_spans, tmp_bytes, (int64_t)width * height * 3, width, bytes, background & 0xffffffu};
    PilFlat f;
    if (!pil_flat_plan(out, sizeof(O), g.total, SHEET_THREADS, f)) return VRG_ERR_UNSUPPORTED;       // (never with SHEET_MAX_SIDE)
    hipLaunchKernelGGL((k_sheet_compose<O>), dim3((uint32_t)f.blocks), dim3(SHEET_THREADS), 0, (hipStream_t)stream, panels, tables, spans, tmp, out, g,
                       f.lead, f.pieces);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_sheet_fit(int32_t src_w, int32_t src_h, int32_t w, int32_t h, int32_t cover, int32_t* fit_host) {
    if (!fit_host || src_w < 1 || src_h < 1 || w < 1 || h < 1) return VRG_ERR_BAD_ARG;
    if (src_w > SHEET_MAX_SIDE || src_h > SHEET_MAX_SIDE || w > SHEET_MAX_SIDE || h > SHEET_MAX_SIDE) return VRG_ERR_UNSUPPORTED;
    sheet_fit(src_w, src_h, w, h, cover != 0, fit_host);
    return VRG_OK;
}

int vrg_sheet_plan(vrg_sheet_panel* panels_host, int64_t n, const int32_t* tables_host, int64_t table_ints) {
    if (n < 0 || table_ints < 0 || (n > 0 && !panels_host) || (table_ints > 0 && !tables_host)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; ++i) {
        vrg_sheet_panel q = panels_host[i];                                    // the fields the plan reads, judged before a table is read
        q.cps = 1;
        q.tmp_offset = 0;
        q.span_offset = -1;
        q.row0 = q.src_h != q.new_h ? 0 : q.win_y;
        q.rows = q.src_h != q.new_h ? 1 : q.pic_h;
        if (!q.src) q.src = panels_host;                                       // the plan does not need the source
        if (!sheet_panel_ok(q, true, table_ints, 0, 0x7fffffffffffffffll)) return VRG_ERR_BAD_ARG;
        if (!sheet_plan(panels_host[i], tables_host)) return VRG_ERR_UNSUPPORTED;
    }
    return VRG_OK;
}

int vrg_sheet_check(const vrg_sheet_panel* panels_host, int64_t n, int32_t bytes, const int32_t* tables_host, int64_t table_ints, int64_t n_spans,
                    int64_t tmp_bytes) {
    return sheet_check(panels_host, n, bytes != 0, tables_host, table_ints, n_spans, tmp_bytes);
}

int vrg_sheet_rows_f32(const vrg_sheet_panel* panels, int64_t n, const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes,
                       int32_t max_segments, int32_t max_rows, void* stream) {
    return sheet_rows_launch<float>(panels, n, tables, table_ints, tmp, tmp_bytes, max_segments, max_rows, stream);
}

int vrg_sheet_rows_u8(const vrg_sheet_panel* panels, int64_t n, const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes,
                      int32_t max_segments, int32_t max_rows, void* stream) {
    return sheet_rows_launch<uint8_t>(panels, n, tables, table_ints, tmp, tmp_bytes, max_segments, max_rows, stream);
}

int vrg_sheet_compose_f32(const vrg_sheet_panel* panels, int64_t n, int32_t bytes, const int32_t* tables, int64_t table_ints, const int32_t* spans,
                          int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, float* out, int32_t width, int32_t height, uint32_t background,
                          void* stream) {
    return sheet_compose_launch<float>(panels, n, bytes, tables, table_ints, spans, n_spans, tmp, tmp_bytes, out, width, height, background, stream);
}

int vrg_sheet_compose_u8(const vrg_sheet_panel* panels, int64_t n, int32_t bytes, const int32_t* tables, int64_t table_ints, const int32_t* spans,
                         int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, uint8_t* out, int32_t width, int32_t height, uint32_t background,
                         void* stream) {
    return sheet_compose_launch<uint8_t>(panels, n, bytes, tables, table_ints, spans, n_spans, tmp, tmp_bytes, out, width, height, background, stream);
}

}  // extern "C"
