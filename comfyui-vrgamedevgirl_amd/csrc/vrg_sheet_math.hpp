// vrg_sheet_math.hpp -- arithmetic of the reference sheets (csrc/vrg_sheet.hip), host and device.
//
// What is restated: VRGDG_LTXICIngredientsGrid.build of the reference (VRGDG_LTXICIngredientsGrid.py:37-95, :337-400) and the three sheet
// builders of the AI Video Builder (VRGDG_MusicVideoBuilderNodes.py:7169-7238) -- numpy and Pillow, no cv2.  Nothing of
// vrg_pil_resample.hpp (Pillow's 22-bit LANCZOS tables, its tap records and its two byte passes) or vrg_grid_math.hpp (the truncating
// quantiser, byte / 255) is stated again; this header holds the glue between them.
//   source -> bytes   C == 1 is repeated to three channels, C == 3 is taken as is, C > 3 gives its first three; C == 2 is refused (so does
//                     Image.fromarray).  byte = grid_quant(x) = trunc(clip(fl(x * 255.0f), 0, 255)).  NaN has no defined result in numpy;
//                     here it gives 0, as in the grid plot.  A byte source is its own quantisation.
//   panel picture     scale = max(w / sw, h / sh) for cover_crop, min for contain_pad, in double; new = max(1, round(src * scale)) with
//                     Python's round (half to even: nearbyint).  The picture is Image.resize((new_w, new_h), LANCZOS) of the whole source:
//                     horizontal pass, rounded clipped bytes, vertical pass; a pass whose size does not change is skipped.  cover_crop
//                     keeps the window at (max(0, (new_w - w) // 2), max(0, (new_h - h) // 2)); contain_pad centres the picture at
//                     ((w - new_w) // 2, (h - new_h) // 2) on the cell colour.  Only the window's columns and the source rows its taps
//                     touch are computed (`tmp`: [rows][pic_w][3] bytes, row r = source row row0 + r, or window row r when the vertical
//                     pass is skipped).
//   canvas            panels are pasted in order, so for a pixel the LAST panel that covers it decides: covered = inside the panel's
//                     rectangle and, where the panel has a mask, inside the row's span (the 0 / 255 mask of ImageDraw.rounded_rectangle,
//                     its first and last set column per row taken from Pillow on the host; first > last: none -- a 1 x 1 panel's mask is
//                     all zero and pastes nothing).  A covered pixel is the picture's where the window lies, else the cell colour; an
//                     uncovered one is the background.  Image.paste clips to the canvas: so does the walk over the canvas.
//   output            (float)byte / 255.0f (grid_unit), or the byte.
#pragma once
#include "vrg_common.hpp"
#include "vrg_grid_math.hpp"
#include "vrg_pil_resample.hpp"

namespace vrg {

constexpr int SHEET_MAX_SIDE = VRG_SHEET_MAX_SIDE;            // source, resized picture, panel and canvas sides
constexpr int SHEET_STAGE_VALUES = VRG_SHEET_STAGE_VALUES;    // source values (pixels x channels) of one staged row segment
constexpr int SHEET_ROWS = 4;                                 // source rows one workgroup of the horizontal pass takes
constexpr int SHEET_FIT_WORDS = 8;                            // new_w, new_h, win_x, win_y, pic_w, pic_h, pic_x, pic_y

// the source channel output channel c reads
VRG_HD int32_t sheet_channel(int32_t channels, int32_t c) { return channels == 1 ? 0 : c; }

VRG_HD bool sheet_channels_ok(int32_t channels) { return channels == 1 || channels >= 3; }

// HOST.  _resize_to_panel: the size of the resized picture, the window of it that is kept and where the window lies in the panel
inline void sheet_fit(int32_t src_w, int32_t src_h, int32_t w, int32_t h, bool cover, int32_t* fit) {
    const double sx = (double)w / (double)src_w, sy = (double)h / (double)src_h;
    const double scale = cover ? (sx > sy ? sx : sy) : (sx < sy ? sx : sy);
    const double rw = nearbyint((double)src_w * scale), rh = nearbyint((double)src_h * scale);
    const int32_t new_w = rw < 1.0 ? 1 : (rw > 2147483647.0 ? 2147483647 : (int32_t)rw);
    const int32_t new_h = rh < 1.0 ? 1 : (rh > 2147483647.0 ? 2147483647 : (int32_t)rh);
    int32_t win_x = 0, win_y = 0, pic_x = 0, pic_y = 0;
    if (cover) {
        win_x = new_w > w ? (new_w - w) / 2 : 0;
        win_y = new_h > h ? (new_h - h) / 2 : 0;
    } else {                                                  // floor division, as Python's //
        pic_x = (w - new_w) >= 0 ? (w - new_w) / 2 : -((new_w - w + 1) / 2);
        pic_y = (h - new_h) >= 0 ? (h - new_h) / 2 : -((new_h - h + 1) / 2);
    }
    fit[0] = new_w;
    fit[1] = new_h;
    fit[2] = win_x;
    fit[3] = win_y;
    fit[4] = cover ? w : new_w;
    fit[5] = cover ? h : new_h;
    fit[6] = pic_x;
    fit[7] = pic_y;
}

// what the kernels need to hold before they follow a record: every offset inside its buffer, every size in range (no table is read here)
VRG_HD bool sheet_panel_ok(const vrg_sheet_panel& p, bool bytes, int64_t table_ints, int64_t n_spans, int64_t tmp_bytes) {
    if (!p.src || !sheet_channels_ok(p.channels) || p.channels > SHEET_STAGE_VALUES) return false;
    if (!bytes && (reinterpret_cast<uintptr_t>(p.src) & 3u)) return false;
    if (p.src_w < 1 || p.src_h < 1 || p.new_w < 1 || p.new_h < 1 || p.w < 1 || p.h < 1 || p.pic_w < 1 || p.pic_h < 1) return false;
    if (p.src_w > SHEET_MAX_SIDE || p.src_h > SHEET_MAX_SIDE || p.new_w > SHEET_MAX_SIDE || p.new_h > SHEET_MAX_SIDE || p.w > SHEET_MAX_SIDE ||
        p.h > SHEET_MAX_SIDE)
        return false;
    if (p.win_x < 0 || p.win_y < 0 || p.win_x > p.new_w - p.pic_w || p.win_y > p.new_h - p.pic_h) return false;      // the window inside the picture
    if (p.pic_x < 0 || p.pic_y < 0 || p.pic_x > p.w - p.pic_w || p.pic_y > p.h - p.pic_h) return false;              // and inside the panel
    const bool hp = p.src_w != p.new_w, vp = p.src_h != p.new_h;
    if (hp && (p.h_ksize < 1 || !span_fits(p.h_table, (int64_t)p.new_w * (2 + p.h_ksize), table_ints))) return false;
    if (vp && (p.v_ksize < 1 || !span_fits(p.v_table, (int64_t)p.new_h * (2 + p.v_ksize), table_ints))) return false;
    if (p.rows < 1 || p.row0 < 0 || p.row0 > (vp ? p.src_h : p.new_h) - p.rows) return false;
    if (!vp && (p.row0 != p.win_y || p.rows != p.pic_h)) return false;
    if (p.cps < 1 || p.cps > p.pic_w) return false;
    if (p.span_offset != -1 && !span_fits(p.span_offset, p.h, n_spans)) return false;
    return span_fits(p.tmp_offset, (int64_t)p.rows * p.pic_w * 3, tmp_bytes);
}

// the source pixels [lo, hi) the window columns [c0, c1) read
VRG_HD void sheet_source_range(const vrg_sheet_panel& p, const int32_t* tables, int32_t c0, int32_t c1, int32_t& lo, int32_t& hi) {
    if (p.src_w != p.new_w) {
        const int32_t* hb = tables + p.h_table;
        lo = hb[2 * (p.win_x + c0)];
        hi = hb[2 * (p.win_x + c1 - 1)] + hb[2 * (p.win_x + c1 - 1) + 1];
    } else {
        lo = p.win_x + c0;
        hi = p.win_x + c1;
    }
    lo = lo < 0 ? 0 : (lo > p.src_w ? p.src_w : lo);
    hi = hi < lo ? lo : (hi > p.src_w ? p.src_w : hi);
}

// one pixel of `tmp`: window column col of one source row.  load(x, c) = the quantised channel c (of the source) of source pixel x, which
// is asked only for lo <= x < hi; a column whose taps leave that range gives 0 (never taken with the tables and the cps of sheet_plan)
template <class Load>
VRG_HD void sheet_row_pixel(const vrg_sheet_panel& p, const int32_t* tables, int32_t col, int32_t lo, int32_t hi, Load load, uint8_t* out) {
    const int32_t c1 = sheet_channel(p.channels, 1), c2 = sheet_channel(p.channels, 2);
    const int32_t xx = p.win_x + col;
    if (p.src_w == p.new_w) {                                                  // skipped: the quantised window itself
        const bool in = xx >= lo && xx < hi;
        out[0] = in ? load(xx, 0) : 0;
        out[1] = in ? load(xx, c1) : 0;
        out[2] = in ? load(xx, c2) : 0;
        return;
    }
    const PilRecord t = pil_record(tables + p.h_table, p.new_w, xx, p.h_ksize, lo, hi);
    if (!t.ok) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    pil_taps<3>(t.w, t.n, [&](int32_t i, int c) { return load(t.first + i, c == 0 ? 0 : (c == 1 ? c1 : c2)); }, out);
}

// channel c of window pixel (cx, cy): the vertical pass over `tmp`
VRG_HD uint8_t sheet_picture_byte(const vrg_sheet_panel& p, const int32_t* tables, const uint8_t* tmp, int32_t cx, int32_t cy, int32_t c) {
    const uint8_t* t = tmp + p.tmp_offset;
    const int64_t pitch = (int64_t)p.pic_w * 3;
    if (p.src_h == p.new_h) return t[(int64_t)cy * pitch + cx * 3 + c];
    const PilRecord v = pil_record(tables + p.v_table, p.new_h, p.win_y + cy, p.v_ksize, p.row0, p.row0 + p.rows);
    if (!v.ok) return 0;                                                      // (never taken with sheet_plan's rows)
    return pil_walk_byte(v.w, v.n, t + (int64_t)(v.first - p.row0) * pitch + cx * 3 + c, pitch);
}

// which panel decides canvas pixel (x, y): its index, or -1 for the background
VRG_HD int64_t sheet_panel_at(const vrg_sheet_panel* panels, int64_t n, const int32_t* spans, int64_t n_spans, bool bytes, int64_t table_ints,
                              int64_t tmp_bytes, int32_t x, int32_t y) {
    for (int64_t i = n - 1; i >= 0; --i) {
        const vrg_sheet_panel& p = panels[i];
        const int64_t lx = (int64_t)x - p.left, ly = (int64_t)y - p.top;
        if (lx < 0 || ly < 0 || lx >= p.w || ly >= p.h) continue;
        if (!sheet_panel_ok(p, bytes, table_ints, n_spans, tmp_bytes)) continue;                // a record the kernels do not follow pastes nothing
        if (p.span_offset != -1) {
            const int32_t* sp = spans + 2 * (p.span_offset + ly);
            if (lx < sp[0] || lx > sp[1]) continue;
        }
        return i;
    }
    return -1;
}

// channel c of canvas pixel (x, y) under panel `at` (sheet_panel_at); background = R | G << 8 | B << 16
VRG_HD uint8_t sheet_canvas_byte(const vrg_sheet_panel* panels, int64_t at, const int32_t* tables, const uint8_t* tmp, uint32_t background,
                                 int32_t x, int32_t y, int32_t c) {
    if (at < 0) return (uint8_t)(background >> (8 * c));
    const vrg_sheet_panel& p = panels[at];
    const int32_t cx = x - p.left - p.pic_x, cy = y - p.top - p.pic_y;
    if (cx < 0 || cy < 0 || cx >= p.pic_w || cy >= p.pic_h) return p.cell[c];
    return sheet_picture_byte(p, tables, tmp, cx, cy, c);
}

VRG_HD float sheet_unit(uint8_t b) { return grid_unit((int32_t)b); }

// ---- HOST ----

// row0, rows and cps of a record whose other fields are filled in: the source rows the window's vertical taps touch, and the most window
// columns per segment whose source values fit the staging buffer.  false: the taps of one column do not fit.
inline bool sheet_plan(vrg_sheet_panel& p, const int32_t* tables) {
    if (p.src_h != p.new_h) {
        const int32_t* vb = tables + p.v_table;
        const int32_t last = p.win_y + p.pic_h - 1;
        p.row0 = vb[2 * p.win_y];
        p.rows = vb[2 * last] + vb[2 * last + 1] - p.row0;
    } else {
        p.row0 = p.win_y;
        p.rows = p.pic_h;
    }
    for (int32_t cps = p.pic_w;; cps = (cps + 1) / 2) {
        int64_t longest = 0;
        for (int32_t c0 = 0; c0 < p.pic_w; c0 += cps) {
            int32_t lo, hi;
            sheet_source_range(p, tables, c0, c0 + cps < p.pic_w ? c0 + cps : p.pic_w, lo, hi);
            longest = hi - lo > longest ? hi - lo : longest;
        }
        if (longest * p.channels <= SHEET_STAGE_VALUES) {
            p.cps = cps;
            return true;
        }
        if (cps == 1) return false;
    }
}

// are the tables of the record the whole-axis LANCZOS tables for its sizes (vrg_pil_lanczos_table), and row0 / rows / cps sheet_plan's
inline bool sheet_tables_ok(const vrg_sheet_panel& p, const int32_t* tables) {
    for (int axis = 0; axis < 2; ++axis) {
        const int32_t n_in = axis ? p.src_h : p.src_w, n_out = axis ? p.new_h : p.new_w, ksize = axis ? p.v_ksize : p.h_ksize;
        if (n_in == n_out) continue;
        if (ksize != pil_lanczos_ksize(n_in, n_out)) return false;
        const size_t n = (size_t)n_out * (2 + (size_t)ksize);
        int32_t* want = new int32_t[n];
        pil_lanczos_table(n_in, n_out, want, want + 2 * (size_t)n_out);
        const int32_t* got = tables + (axis ? p.v_table : p.h_table);
        bool same = true;
        for (size_t i = 0; i < n && same; ++i) same = got[i] == want[i];
        delete[] want;
        if (!same) return false;
    }
    vrg_sheet_panel q = p;
    return sheet_plan(q, tables) && q.row0 == p.row0 && q.rows == p.rows && q.cps == p.cps;
}

// VRG_OK, or why a list of records is refused (vrg_sheet_check; the `src` of a record is only compared with null)
inline int sheet_check(const vrg_sheet_panel* panels, int64_t n, bool bytes, const int32_t* tables, int64_t table_ints, int64_t n_spans,
                       int64_t tmp_bytes) {
    if (n < 0 || table_ints < 0 || n_spans < 0 || tmp_bytes < 0 || (n > 0 && !panels) || (table_ints > 0 && !tables)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const vrg_sheet_panel& p = panels[i];
        if (p.src_w > SHEET_MAX_SIDE || p.src_h > SHEET_MAX_SIDE || p.new_w > SHEET_MAX_SIDE || p.new_h > SHEET_MAX_SIDE || p.w > SHEET_MAX_SIDE ||
            p.h > SHEET_MAX_SIDE)
            return VRG_ERR_UNSUPPORTED;
        vrg_sheet_panel q = p;                                                 // row0 / rows / cps are judged against the tables below
        q.cps = 1;
        if (p.src_h != p.new_h) {
            q.row0 = 0;
            q.rows = 1;
        }
        if (!sheet_panel_ok(q, bytes, table_ints, n_spans, 0x7fffffffffffffffll)) return VRG_ERR_BAD_ARG;
        q = p;
        if (!sheet_plan(q, tables)) return VRG_ERR_UNSUPPORTED;                // the taps of one column pass the staging buffer
        if (!sheet_tables_ok(p, tables) || !sheet_panel_ok(p, bytes, table_ints, n_spans, tmp_bytes)) return VRG_ERR_BAD_ARG;
    }
    return VRG_OK;
}

// the horizontal pass of one record straight from the definition (tests/host_math/sheet_check.cpp; the kernel stages the same bytes in LDS)
template <typename T>
inline void sheet_rows_host(const vrg_sheet_panel& p, const int32_t* tables, uint8_t* tmp) {
    const T* src = reinterpret_cast<const T*>(p.src);
    int32_t lo, hi;
    sheet_source_range(p, tables, 0, p.pic_w, lo, hi);
    for (int32_t r = 0; r < p.rows; ++r) {
        const T* row = src + (int64_t)(p.row0 + r) * p.src_w * p.channels;
        for (int32_t col = 0; col < p.pic_w; ++col)
            sheet_row_pixel(p, tables, col, lo, hi, [&](int32_t x, int32_t c) { return grid_quant(row[(int64_t)x * p.channels + c]); },
                            tmp + p.tmp_offset + ((int64_t)r * p.pic_w + col) * 3);
    }
}

// the canvas [height][width][3], as bytes and as floats (either may be null)
inline void sheet_compose_host(const vrg_sheet_panel* panels, int64_t n, bool bytes, const int32_t* tables, int64_t table_ints, const int32_t* spans,
                               int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, uint32_t background, int32_t width, int32_t height,
                               uint8_t* out_u8, float* out_f32) {
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) {
            const int64_t at = sheet_panel_at(panels, n, spans, n_spans, bytes, table_ints, tmp_bytes, x, y);
            for (int32_t c = 0; c < 3; ++c) {
                const uint8_t b = sheet_canvas_byte(panels, at, tables, tmp, background, x, y, c);
                const int64_t e = ((int64_t)y * width + x) * 3 + c;
                if (out_u8) out_u8[e] = b;
                if (out_f32) out_f32[e] = sheet_unit(b);
            }
        }
}

}  // namespace vrg
