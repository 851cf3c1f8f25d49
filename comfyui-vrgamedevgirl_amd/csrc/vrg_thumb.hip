// vrg_thumb.hip -- the contact sheet of the far-face repair backend (reference scripts/far_face_repair_backend.py: contact_sheet :374-408)
// on decoded bytes: original and fixed frame side by side, Image.thumbnail (Image.reduce, then a BICUBIC resize over the fractional source
// box) and the paste into the cells of the sheet, byte for byte.  gfx950 only.  Arithmetic, byte staging and the flat piece writer:
// csrc/vrg_pil_resample.hpp.  The resize is over the box (0, 0, w / fx, h / fy) of the reduced picture; one more than PIL_TALL_RATIO times
// as tall as wide resizes vertically first in Pillow: not restated, refused.  The sheet (:398-406): cols = max(1, columns),
// rows = ceil(n / cols), the cell is the largest thumbnail, thumbnail i is pasted at ((i % cols) cell_w, (i / cols) cell_h) on (24, 24, 24).
//
// k_thumb_rows     the pair, the reduce and the horizontal pass.  One workgroup = ONE reduced row (fy source rows) of a segment of `cps`
//                  output columns of one entry.  Per source row the 256 threads read the bytes the segment's taps touch ONCE with 16-byte
//                  non-temporal loads into LDS -- the run out of the original and the run out of the fixed frame each at the phase of its
//                  own address, black where the fixed frame ends -- and add the fx bytes of every cell to a uint32 per reduced value in
//                  LDS.  After the last row a value becomes Pillow's byte (pil_reduce_byte with the cell's own pixel count: the partial
//                  last column, row and corner and a cell that straddles the seam of the pair are nothing special), and a thread owns
//                  output columns and walks their taps over the reduced bytes (pil_taps) into tmp.  Neither the pair nor the reduced
//                  picture reaches memory.  Factors (1, 1): the staged bytes are the reduced row; no table: they are the output row.
//                  LDS: 8.1 KB of source bytes, 16 KB of sums, 8 KB of reduced bytes -- 32 KB, four workgroups (16 waves) on a CU.
// k_thumb_compose  one pass over the sheet as a flat run of bytes, one 16-byte piece per thread: a byte inside a thumbnail is the vertical
//                  pass over tmp (one channel's taps), every other byte the canvas colour; ThumbCursor gives pil_flat_write the bytes.
#include "vrg_common.hpp"
#include "vrg_pil_resample.hpp"

namespace vrg {

constexpr int PT_THREADS = 256;
constexpr int PT_STAGE = VRG_THUMB_STAGE_BYTES;
constexpr int PT_VALUES = VRG_THUMB_STAGE_VALUES;
constexpr int PT_STAGE_LDS = PT_STAGE + 64;                                    // two runs, each at its phase behind a 16-byte boundary

struct ThumbGeom {
    int64_t src_bytes, table_ints, tmp_bytes;
};

VRG_HD int32_t thumb_pair_w(const vrg_thumb_entry& e) { return e.right_offset >= 0 ? 2 * e.left_w : e.left_w; }

// reduced values a segment may hold: the sums are kept only where cells are folded
VRG_HD int32_t thumb_value_cap(const vrg_thumb_entry& e) { return e.fx * e.fy > 1 ? PT_VALUES : PT_STAGE; }

// everything of an entry that needs no table; the kernels follow no entry that fails it
VRG_HD bool thumb_entry_ok(const vrg_thumb_entry& e, const ThumbGeom& g) {
    if (e.left_w < 1 || e.left_h < 1 || e.left_w > VRG_THUMB_MAX_SOURCE || e.left_h > VRG_THUMB_MAX_SOURCE) return false;
    if (e.fx < 1 || e.fy < 1 || e.fx > VRG_THUMB_MAX_FACTOR || e.fy > VRG_THUMB_MAX_FACTOR || e.cps < 1) return false;
    if (e.red_w != pil_reduced_size(thumb_pair_w(e), e.fx) || e.red_h != pil_reduced_size(e.left_h, e.fy)) return false;
    if (e.out_w < 1 || e.out_h < 1 || e.out_w > VRG_THUMB_MAX_SOURCE || e.out_h > VRG_THUMB_MAX_SOURCE) return false;
    if (e.h_ksize < 0 || e.v_ksize < 0 || (e.h_ksize == 0 && e.out_w != e.red_w) || (e.v_ksize == 0 && e.out_h != e.red_h)) return false;
    if (!span_fits(e.left_offset, (int64_t)e.left_h * e.left_w * 3, g.src_bytes)) return false;
    if (e.right_offset >= 0 && (e.right_w < 1 || e.right_h < 1 || e.right_w > VRG_THUMB_MAX_SOURCE || e.right_h > VRG_THUMB_MAX_SOURCE ||
                                !span_fits(e.right_offset, (int64_t)e.right_h * e.right_w * 3, g.src_bytes)))
        return false;
    if (e.right_offset < -1) return false;
    if (!span_fits(e.tmp_offset, (int64_t)e.red_h * e.out_w * 3, g.tmp_bytes)) return false;
    if (e.h_ksize && !span_fits(e.h_table, (int64_t)e.out_w * (2 + e.h_ksize), g.table_ints)) return false;
    if (e.v_ksize && !span_fits(e.v_table, (int64_t)e.out_h * (2 + e.v_ksize), g.table_ints)) return false;
    return true;
}

// the reduced columns [lo, hi) that the output columns [c0, c1) of an entry read; false: the table does not fit the entry
VRG_HD bool thumb_source_range(const vrg_thumb_entry& e, const int32_t* tables, int32_t c0, int32_t c1, int32_t& lo, int32_t& hi) {
    if (!e.h_ksize) {
        lo = c0;
        hi = c1;
        return true;
    }
    const int32_t* table = tables + e.h_table;
    lo = table[2 * c0];
    if (lo < 0 || table[2 * c0 + 1] < 0) return false;
    const PilRecord last = pil_record(table, e.out_w, c1 - 1, e.h_ksize, lo, e.red_w);
    if (!last.ok) return false;
    hi = last.first + last.n;
    return hi > lo;
}

// does the segment [lo, hi) of reduced columns fit the staging buffers?
VRG_HD bool thumb_segment_fits(const vrg_thumb_entry& e, int32_t lo, int32_t hi) {
    const int64_t p1 = (int64_t)hi * e.fx < thumb_pair_w(e) ? (int64_t)hi * e.fx : thumb_pair_w(e);
    return (p1 - (int64_t)lo * e.fx) * 3 <= PT_STAGE && (int64_t)(hi - lo) * 3 <= thumb_value_cap(e);
}

__global__ __launch_bounds__(PT_THREADS) void k_thumb_rows(const uint8_t* __restrict__ src, const vrg_thumb_entry* __restrict__ entries,
                                                            const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp, ThumbGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[PT_STAGE_LDS];
    __shared__ uint32_t acc[PT_VALUES];
    __shared__ uint8_t red[PT_STAGE];
    const vrg_thumb_entry e = entries[blockIdx.z];                             // workgroup-uniform, as is every return below
    if (!thumb_entry_ok(e, g)) return;
    const int tid = (int)threadIdx.x;
    const int32_t r = (int32_t)blockIdx.y;
    const int64_t c0l = (int64_t)blockIdx.x * e.cps;
    if (r >= e.red_h || c0l >= e.out_w) return;
    const int32_t c0 = (int32_t)c0l, c1 = (int32_t)(c0l + e.cps < e.out_w ? c0l + e.cps : e.out_w);
    int32_t lo, hi;
    if (!thumb_source_range(e, tables, c0, c1, lo, hi) || !thumb_segment_fits(e, lo, hi)) return;   // (never with vrg_thumb_check)
    const int32_t pair_w = thumb_pair_w(e), Wl = e.left_w, fx = e.fx;
    const int32_t p0 = lo * fx, p1 = hi * fx < pair_w ? hi * fx : pair_w;     // the pair columns of the segment
    const int32_t l0 = p0 < Wl ? p0 : Wl, l1 = p1 < Wl ? p1 : Wl;             // of them the original's ...
    const int32_t q0 = (p0 > Wl ? p0 : Wl) - Wl, q1 = (p1 > Wl ? p1 : Wl) - Wl;   // ... and the fixed frame's own columns
    const int nl = (l1 - l0) * 3, nr = (q1 - q0) * 3, nvals = (hi - lo) * 3;
    const bool fold = fx * e.fy > 1;
    const int32_t y0 = r * e.fy, y1 = y0 + e.fy < e.left_h ? y0 + e.fy : e.left_h;
    uint8_t* rb = stage + 16 + ((nl + 15) & ~15);                              // the right run's 16-byte boundary, behind the left run
    if (fold)
        for (int j = tid; j < nvals; j += PT_THREADS) acc[j] = 0u;
    for (int32_t y = y0; y < y1; ++y) {
        int phl = 0, offr = 0;
        if (nl > 0) phl = pil_stage_bytes(src + e.left_offset + ((int64_t)y * Wl + l0) * 3, nl, stage, tid, PT_THREADS);
        if (nr > 0) {
            int32_t have = (y < e.right_h ? (q1 < e.right_w ? q1 : e.right_w) : 0) - q0;   // columns the fixed frame has in this row
            have = have > 0 ? have : 0;
            int phr = 0;
            if (have > 0) phr = pil_stage_bytes(src + e.right_offset + ((int64_t)y * e.right_w + q0) * 3, have * 3, rb, tid, PT_THREADS);
            for (int j = have * 3 + tid; j < nr; j += PT_THREADS) rb[phr + j] = 0;                 // Image.new(.., (0, 0, 0)) shows
            offr = (int)(rb - stage) + phr;
        }
        __syncthreads();
        const uint8_t* left = stage + phl;
        const uint8_t* right = stage + offr;                                   // byte b >= nl of the segment is right[b - nl]
        if (fold) {
            for (int j = tid; j < nvals; j += PT_THREADS) {
                const int v = j / 3, c = j - v * 3;
                const int32_t a = (lo + v) * fx, z = a + fx < pair_w ? a + fx : pair_w;
                uint32_t s = 0;
                for (int32_t p = a; p < z; ++p) {
                    const int b = (p - p0) * 3 + c;
                    s += b < nl ? left[b] : right[b - nl];
                }
                acc[j] += s;
            }
        } else {
            for (int j = tid; j < nvals; j += PT_THREADS) red[j] = j < nl ? left[j] : right[j - nl];
        }
        __syncthreads();                                                       // the next row overwrites the buffer
    }
    if (fold) {
        for (int j = tid; j < nvals; j += PT_THREADS) {
            const int32_t a = (lo + j / 3) * fx, z = a + fx < pair_w ? a + fx : pair_w;
            red[j] = pil_reduce_byte(acc[j], (uint32_t)((z - a) * (y1 - y0)));
        }
        __syncthreads();
    }
    uint8_t* row = tmp + e.tmp_offset + (int64_t)r * e.out_w * 3;
    for (int32_t col = c0 + tid; col < c1; col += PT_THREADS) {
        uint8_t o[3] = {0, 0, 0};
        if (!e.h_ksize) {
            for (int c = 0; c < 3; ++c) o[c] = red[(col - lo) * 3 + c];
        } else {
            const PilRecord t = pil_record(tables + e.h_table, e.out_w, col, e.h_ksize, lo, hi);
            if (t.ok) {
                const uint8_t* at = red + (t.first - lo) * 3;
                pil_taps<3>(t.w, t.n, [&](int32_t i, int c) { return at[i * 3 + c]; }, o);
            }
        }
        row[col * 3 + 0] = o[0];
        row[col * 3 + 1] = o[1];
        row[col * 3 + 2] = o[2];
    }
}

struct ThumbSheet {
    int64_t n, total;                                                          // total: bytes of the sheet
    ThumbGeom g;
    int32_t width, columns, cell_w, cell_h;
    uint32_t background;
};

// the entry whose cell holds a pixel, loaded once per run of bytes that share it
struct ThumbAt {
    int64_t i;
    bool ok;
    vrg_thumb_entry e;
};

// the bytes of the sheet for pil_flat_write: channel c of pixel (x, y); the 64-bit divisions are made once per seek, the bytes that follow
// are stepped to
struct ThumbCursor {
    const vrg_thumb_entry* __restrict__ entries;
    const int32_t* __restrict__ tables;
    const uint8_t* __restrict__ tmp;
    const ThumbSheet& s;
    ThumbAt at;
    int32_t x, y, c;

    __device__ __forceinline__ void seek(int64_t b) {
        const int64_t pixel = b / 3;
        c = (int32_t)(b - pixel * 3);
        y = (int32_t)(pixel / s.width);
        x = (int32_t)(pixel - (int64_t)y * s.width);
    }
    __device__ __forceinline__ uint8_t next() {
        const uint8_t v = element();
        if (++c == 3) {
            c = 0;
            if (++x == s.width) {
                x = 0;
                ++y;
            }
        }
        return v;
    }
    __device__ __forceinline__ uint8_t element() {
        const uint8_t ground = (uint8_t)(s.background >> (8 * c));
        const int32_t cx = x / s.cell_w, cy = y / s.cell_h;
        const int64_t i = (int64_t)cy * s.columns + cx;
        if (cx >= s.columns || i >= s.n) return ground;
        if (i != at.i) {
            at.i = i;
            at.e = entries[i];
            at.ok = thumb_entry_ok(at.e, s.g);
        }
        if (!at.ok) return ground;
        const vrg_thumb_entry& e = at.e;
        const int64_t lx = (int64_t)x - e.dst_x, ly = (int64_t)y - e.dst_y;
        if (lx < 0 || ly < 0 || lx >= e.out_w || ly >= e.out_h) return ground;
        const int64_t pitch = (int64_t)e.out_w * 3;
        const uint8_t* col = tmp + e.tmp_offset + lx * 3 + c;                  // [red_h][out_w][3]
        if (!e.v_ksize) return col[ly * pitch];
        const PilRecord v = pil_record(tables + e.v_table, e.out_h, (int32_t)ly, e.v_ksize, 0, e.red_h);
        if (!v.ok) return ground;                                             // (never with vrg_thumb_check) pastes nothing
        return pil_walk_byte(v.w, v.n, col + v.first * pitch, pitch);
    }
};

__global__ __launch_bounds__(PT_THREADS) void k_thumb_compose(const vrg_thumb_entry* __restrict__ entries, const int32_t* __restrict__ tables,
                                                               const uint8_t* __restrict__ tmp, uint8_t* __restrict__ out, ThumbSheet s,
                                                               int64_t lead, int64_t pieces) {
    ThumbCursor cur{entries, tables, tmp, s};
    cur.at.i = -1;
    cur.at.ok = false;
    pil_flat_write(out, s.total, lead, pieces, (int64_t)blockIdx.x * PT_THREADS + threadIdx.x, cur);
}

// HOST.  cps of an entry whose sizes, factors and h_ksize are set: `k` output columns read at most (k - 1) scale + 2 support + 3 reduced
// columns (k where the axis is copied), and a segment's source bytes and reduced values must fit the staging buffers; false: not even one
inline bool thumb_plan_cps(vrg_thumb_entry& e, int32_t filter, float in1) {
    const int64_t most = thumb_value_cap(e) / 3 < PT_STAGE / (3 * e.fx) ? thumb_value_cap(e) / 3 : PT_STAGE / (3 * e.fx);
    int64_t cps = most;
    if (e.h_ksize) {
        const double scale = (double)in1 / e.out_w, support = pil_filter_support(filter) * (scale < 1.0 ? 1.0 : scale);
        const double room = (double)most - 3.0 - 2.0 * support;
        cps = room < 0.0 ? 0 : (int64_t)(room / scale) + 1;
    }
    if (cps < 1) return false;
    e.cps = (int32_t)(cps < e.out_w ? cps : e.out_w);
    return true;
}

// HOST.  the plan of one entry
inline int thumb_plan_entry(vrg_thumb_entry& e, double req_w, double req_h, int32_t filter, double gap) {
    if (e.left_w < 1 || e.left_h < 1 || e.right_offset < -1 || !(req_w >= 1.0) || !(req_h >= 1.0) || !(req_w <= 2147483647.0) ||
        !(req_h <= 2147483647.0))
        return VRG_ERR_BAD_ARG;
    if (e.left_w > VRG_THUMB_MAX_SOURCE || e.left_h > VRG_THUMB_MAX_SOURCE) return VRG_ERR_UNSUPPORTED;
    const int32_t pw = thumb_pair_w(e), ph = e.left_h;
    e.fx = e.fy = 1;
    e.h_ksize = e.v_ksize = 0;
    e.out_w = pw;
    e.out_h = ph;
    float in1[2] = {(float)pw, (float)ph};
    if (pil_thumbnail_size(pw, ph, req_w, req_h, &e.out_w, &e.out_h) && (e.out_w != pw || e.out_h != ph)) {
        if (gap > 0.0) {
            e.fx = pil_reduce_factor(pw, e.out_w, gap);
            e.fy = pil_reduce_factor(ph, e.out_h, gap);
        }
        if (e.fx > VRG_THUMB_MAX_FACTOR || e.fy > VRG_THUMB_MAX_FACTOR) return VRG_ERR_UNSUPPORTED;
        if (e.fx > 1 || e.fy > 1) {
            in1[0] = (float)((double)pw / e.fx);
            in1[1] = (float)((double)ph / e.fy);
        }
    }
    e.red_w = pil_reduced_size(pw, e.fx);
    e.red_h = pil_reduced_size(ph, e.fy);
    if (e.out_w != e.red_w || in1[0] != (float)e.red_w) e.h_ksize = pil_filter_ksize(filter, pil_box_span(0.0f, in1[0]), e.out_w);
    if (e.out_h != e.red_h || in1[1] != (float)e.red_h) e.v_ksize = pil_filter_ksize(filter, pil_box_span(0.0f, in1[1]), e.out_h);
    if ((e.h_ksize || e.v_ksize) && e.red_h > (int64_t)e.red_w * PIL_TALL_RATIO && e.out_h < e.red_h) return VRG_ERR_UNSUPPORTED;
    return thumb_plan_cps(e, filter, in1[0]) ? VRG_OK : VRG_ERR_UNSUPPORTED;
}

// HOST.  the entries planned by `plan_one` one after the other, their temp images packed and their cells laid out `columns` to a row
template <class PlanOne>
inline int thumb_plan_sheet(vrg_thumb_entry* entries_host, int64_t n, int32_t columns, int64_t* sheet_host, PlanOne plan_one) {
    const int64_t cols = columns > 1 ? columns : 1;
    int64_t cell_w = 0, cell_h = 0, tmp_bytes = 0;
    for (int64_t i = 0; i < n; ++i) {
        vrg_thumb_entry& e = entries_host[i];
        const int rc = plan_one(e, i);
        if (rc != VRG_OK) return rc;
        e.tmp_offset = tmp_bytes;
        e.reserved = 0;
        tmp_bytes += (int64_t)e.red_h * e.out_w * 3;
        cell_w = e.out_w > cell_w ? e.out_w : cell_w;
        cell_h = e.out_h > cell_h ? e.out_h : cell_h;
    }
    const int64_t rows = (n + cols - 1) / cols;
    if (cols * cell_w > 0x7fffffffll || rows * cell_h > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < n; ++i) {
        entries_host[i].dst_x = (int32_t)((i % cols) * cell_w);
        entries_host[i].dst_y = (int32_t)((i / cols) * cell_h);
    }
    sheet_host[0] = cols;
    sheet_host[1] = rows;
    sheet_host[2] = cell_w;
    sheet_host[3] = cell_h;
    sheet_host[4] = tmp_bytes;
    return VRG_OK;
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_pil_reduce_host(const uint8_t* src_host, int32_t height, int32_t width, int32_t channels, int32_t fx, int32_t fy, uint8_t* dst_host) {
    if (!src_host || !dst_host || src_host == dst_host || height < 1 || width < 1 || channels < 1 || channels > 4 || fx < 1 || fy < 1)
        return VRG_ERR_BAD_ARG;
    if ((int64_t)fx * fy > 65536) return VRG_ERR_UNSUPPORTED;                  // the sums are uint32
    pil_reduce_image(src_host, height, width, channels, fx, fy, dst_host);
    return VRG_OK;
}

int vrg_thumb_plan(vrg_thumb_entry* entries_host, int64_t n, const double* req_host, int32_t filter, double reducing_gap, int32_t columns,
                   int64_t* sheet_host) {
    if (n < 0 || !sheet_host || (n > 0 && (!entries_host || !req_host)) || !pil_filter_known(filter) ||
        (reducing_gap > 0.0 && reducing_gap < 1.0) || reducing_gap != reducing_gap)
        return VRG_ERR_BAD_ARG;
    return thumb_plan_sheet(entries_host, n, columns, sheet_host, [&](vrg_thumb_entry& e, int64_t i) {
        return thumb_plan_entry(e, req_host[2 * i], req_host[2 * i + 1], filter, reducing_gap);
    });
}

int vrg_thumb_plan_reduce(vrg_thumb_entry* entries_host, int64_t n, int32_t fx, int32_t fy, int32_t columns, int64_t* sheet_host) {
    if (n < 0 || !sheet_host || (n > 0 && !entries_host) || fx < 1 || fy < 1) return VRG_ERR_BAD_ARG;
    if (fx > VRG_THUMB_MAX_FACTOR || fy > VRG_THUMB_MAX_FACTOR) return VRG_ERR_UNSUPPORTED;
    return thumb_plan_sheet(entries_host, n, columns, sheet_host, [&](vrg_thumb_entry& e, int64_t) {
        if (e.left_w < 1 || e.left_h < 1 || e.right_offset < -1) return (int)VRG_ERR_BAD_ARG;
        if (e.left_w > VRG_THUMB_MAX_SOURCE || e.left_h > VRG_THUMB_MAX_SOURCE) return (int)VRG_ERR_UNSUPPORTED;
        e.fx = fx;
        e.fy = fy;
        e.h_ksize = e.v_ksize = 0;
        e.red_w = e.out_w = pil_reduced_size(thumb_pair_w(e), fx);
        e.red_h = e.out_h = pil_reduced_size(e.left_h, fy);
        return thumb_plan_cps(e, PIL_FILTER_BICUBIC, 0.0f) ? (int)VRG_OK : (int)VRG_ERR_UNSUPPORTED;
    });
}

int vrg_thumb_check(const vrg_thumb_entry* entries_host, int64_t n, const int32_t* tables_host, int64_t table_ints, int64_t src_bytes,
                    int64_t tmp_bytes, int32_t width, int32_t height, int32_t columns, int32_t cell_w, int32_t cell_h) {
    if (n < 0 || table_ints < 0 || src_bytes < 0 || tmp_bytes < 0 || (n > 0 && !entries_host) || (table_ints > 0 && !tables_host))
        return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (columns < 1 || cell_w < 1 || cell_h < 1 || (int64_t)columns * cell_w != width || ((n + columns - 1) / columns) * cell_h != height)
        return VRG_ERR_BAD_ARG;
    const ThumbGeom g{src_bytes, table_ints, tmp_bytes};
    for (int64_t i = 0; i < n; ++i) {
        const vrg_thumb_entry& e = entries_host[i];
        if (e.fx > VRG_THUMB_MAX_FACTOR || e.fy > VRG_THUMB_MAX_FACTOR) return VRG_ERR_UNSUPPORTED;
        if (!thumb_entry_ok(e, g) || e.cps > e.out_w) return VRG_ERR_BAD_ARG;
        if (e.out_w > cell_w || e.out_h > cell_h || e.dst_x != (i % columns) * cell_w || e.dst_y != (i / columns) * cell_h) return VRG_ERR_BAD_ARG;
        for (int32_t y = 0; e.v_ksize && y < e.out_h; ++y)
            if (!pil_record(tables_host + e.v_table, e.out_h, y, e.v_ksize, 0, e.red_h).ok) return VRG_ERR_BAD_ARG;
        for (int64_t c0 = 0; c0 < e.out_w; c0 += e.cps) {
            const int32_t c1 = (int32_t)(c0 + e.cps < e.out_w ? c0 + e.cps : e.out_w);
            int32_t lo, hi;
            if (!thumb_source_range(e, tables_host, (int32_t)c0, c1, lo, hi)) return VRG_ERR_BAD_ARG;
            if (!thumb_segment_fits(e, lo, hi)) return VRG_ERR_UNSUPPORTED;
            for (int32_t c = (int32_t)c0; e.h_ksize && c < c1; ++c)
                if (!pil_record(tables_host + e.h_table, e.out_w, c, e.h_ksize, lo, hi).ok) return VRG_ERR_BAD_ARG;
        }
    }
    return VRG_OK;
}

int vrg_thumb_rows_u8(const uint8_t* src, int64_t src_bytes, const vrg_thumb_entry* entries, int64_t n, const int32_t* tables,
                      int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes, int32_t max_segments, int32_t max_rows, void* stream) {
    if (n < 0 || src_bytes < 0 || table_ints < 0 || tmp_bytes < 0 || max_segments < 0 || max_rows < 0) return VRG_ERR_BAD_ARG;
    if (n == 0 || max_segments == 0 || max_rows == 0) return VRG_OK;
    if (!src || !entries || !tmp || (table_ints > 0 && !tables) || (reinterpret_cast<uintptr_t>(entries) & 7u) ||
        (reinterpret_cast<uintptr_t>(tables) & 3u) || (const void*)tmp == (const void*)src || (const void*)tmp == (const void*)entries ||
        (const void*)tmp == (const void*)tables)
        return VRG_ERR_BAD_ARG;
    if (max_segments > VRG_THUMB_MAX_SOURCE || max_rows > VRG_THUMB_MAX_SOURCE) return VRG_ERR_UNSUPPORTED;
    const ThumbGeom g{src_bytes, table_ints, tmp_bytes};
    return launch_chunks(n, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL(k_thumb_rows, dim3((uint32_t)max_segments, (uint32_t)max_rows, (uint32_t)count), dim3(PT_THREADS), 0, (hipStream_t)stream,
                           src, entries + first, tables, tmp, g);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

int vrg_thumb_compose_u8(const vrg_thumb_entry* entries, int64_t n, const int32_t* tables, int64_t table_ints, const uint8_t* tmp,
                         int64_t tmp_bytes, uint8_t* out, int32_t width, int32_t height, int32_t columns, int32_t cell_w, int32_t cell_h,
                         uint32_t background, void* stream) {
    if (n < 0 || table_ints < 0 || tmp_bytes < 0) return VRG_ERR_BAD_ARG;
    if (n == 0) return VRG_OK;
    if (!entries || !tmp || !out || width < 1 || height < 1 || columns < 1 || cell_w < 1 || cell_h < 1 || (table_ints > 0 && !tables) ||
        (reinterpret_cast<uintptr_t>(entries) & 7u) || (reinterpret_cast<uintptr_t>(tables) & 3u))
        return VRG_ERR_BAD_ARG;
    const void* o = out;
    if (o == (const void*)tmp || o == (const void*)tables || o == (const void*)entries) return VRG_ERR_BAD_ARG;
    const ThumbSheet s{n, (int64_t)width * height * 3, ThumbGeom{0x7fffffffffffffffll, table_ints, tmp_bytes}, width, columns, cell_w, cell_h,
                       background & 0xffffffu};
    PilFlat f;
    if (!pil_flat_plan(out, 1, s.total, PT_THREADS, f)) return VRG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_thumb_compose, dim3((uint32_t)f.blocks), dim3(PT_THREADS), 0, (hipStream_t)stream, entries, tables, tmp, out, s, f.lead,
                       f.pieces);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
