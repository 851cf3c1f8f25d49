// vrg_area_walk.hpp -- the workgroup-level source walk of cv2.resize(..., INTER_AREA) on bytes, device only: k_cut_thumbs (csrc/vrg_cut.hip),
// k_grid_tiles (csrc/vrg_grid.hip) and k_face_thumbs (csrc/vrg_thumbs.hip) are built on it.  Arithmetic: csrc/vrg_grid_math.hpp.
//
// One workgroup (four waves) = up to 64 columns of one output row.  The order of the fp32 sums is the bit-exactness contract with OpenCV and
// fixes what may run in parallel: source rows are independent until the vertical combine, columns are independent along x, the terms of one
// column of one row are sequential.
//   The source rows of the output row go round the four waves.  A wave reads the samples its columns need once with 16-byte loads (from the
//   first 16-byte boundary on; the few values in front of and behind them go one by one), quantises them and keeps the BYTES in a row buffer
//   of its own in LDS, at the byte phase of the source (all C channels: the layout of the buffer is the layout of the row).  Then lane d
//   walks the taps of column d for three channels out of that buffer -- 64 lanes x 3 sequential sums -- and leaves the three words of its
//   (row, column) in LDS.  Samples that do not fit the row buffer go through it in segments of whole columns (`cps` columns each).
//   After every four rows the workgroup meets once and 192 threads fold the four rows' words into their running values in row order (two
//   sets of words, so one barrier per four rows); at the end they make the byte.
// One walk serves every rule (a GridMode), the words it leaves differ:
//     general   fp32 sums in cv2's order                         folded with the row weights, rounded
//     fast/copy integer sums (copy: cells of one sample)         added, scaled by 1 / (sx * sy), rounded (2 x 2: (sum + 2) >> 2)
//     linear    dt_hpass of the column's one or two samples      the one or two rows through dt_vpass
// The rule is workgroup-uniform; a caller that passes a constant (k_cut_thumbs) has the other rules folded away.
#pragma once
#include "vrg_common.hpp"
#include "vrg_grid_math.hpp"

namespace vrg {

constexpr int WALK_WAVES = 4, WALK_THREADS = WALK_WAVES * 64;
constexpr int WALK_VALUES = GRID_LANES * 3;                                    // the values of one workgroup
constexpr int WALK_PART_BYTES = 2 * WALK_WAVES * WALK_VALUES * 4;              // part[2][WALK_WAVES][WALK_VALUES]: two sets of four rows' words
constexpr int WALK_CELL_BYTES = GRID_LANES * (int)sizeof(AreaCell);            // the column table of one workgroup
static_assert(AREA_OUT == GRID_LANES, "a cut thumbnail row is one workgroup");

typedef float walk_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t walk_u4 __attribute__((ext_vector_type(4)));

struct WalkSums {                                                              // of thread tid < WALK_VALUES: fp32 bits (general) or integers
    uint32_t total, row0, row1;
};

// What one wave wrote to ITS row buffer is read by other lanes of the same wave only: a wave's LDS accesses execute in order, the fences
// keep the compiler from moving them across.
VRG_D void walk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <uint8_t (*QUANT)(float)>
VRG_D uint32_t walk_quant4(const walk_f4 v) {
    return (uint32_t)QUANT(v.x) | ((uint32_t)QUANT(v.y) << 8) | ((uint32_t)QUANT(v.z) << 16) | ((uint32_t)QUANT(v.w) << 24);
}

// n values from src as bytes into rb: value i lands at rb[ph + i], ph the returned phase (fp32: the float's index mod 4; bytes: the
// address mod 16), so that the 16-byte loads and the LDS words they fill are both aligned.  Nothing outside src[0 .. n) is read; rb holds
// n + 4 (fp32) or n + 16 (bytes).  A byte source is its own quantisation: QUANT is for fp32 alone.
template <uint8_t (*QUANT)(float)>
VRG_D int walk_stage(const float* src, int n, uint8_t* rb, int lane) {
    const int ph = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
    int head = (4 - ph) & 3;
    head = head < n ? head : n;
    const int nq = (n - head) >> 2;
    if (lane < head) rb[ph + lane] = QUANT(src[lane]);
    const walk_f4* body = reinterpret_cast<const walk_f4*>(src + head);
    uint32_t* dst = reinterpret_cast<uint32_t*>(rb + ph + head);
    int q = lane;
    for (; q + 192 < nq; q += 256) {                                           // four loads in flight per lane
        const walk_f4 v0 = __builtin_nontemporal_load(body + q), v1 = __builtin_nontemporal_load(body + q + 64);
        const walk_f4 v2 = __builtin_nontemporal_load(body + q + 128), v3 = __builtin_nontemporal_load(body + q + 192);
        dst[q] = walk_quant4<QUANT>(v0);
        dst[q + 64] = walk_quant4<QUANT>(v1);
        dst[q + 128] = walk_quant4<QUANT>(v2);
        dst[q + 192] = walk_quant4<QUANT>(v3);
    }
    for (; q < nq; q += 64) dst[q] = walk_quant4<QUANT>(__builtin_nontemporal_load(body + q));
    const int t = head + 4 * nq + lane;
    if (t < n) rb[ph + t] = QUANT(src[t]);
    return ph;
}

template <uint8_t (*QUANT)(float)>
VRG_D int walk_stage(const uint8_t* src, int n, uint8_t* rb, int lane) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    int head = (16 - ph) & 15;
    head = head < n ? head : n;
    const int nq = (n - head) >> 4;
    if (lane < head) rb[ph + lane] = src[lane];
    const walk_u4* body = reinterpret_cast<const walk_u4*>(src + head);
    walk_u4* dst = reinterpret_cast<walk_u4*>(rb + ph + head);
    for (int q = lane; q < nq; q += 64) dst[q] = __builtin_nontemporal_load(body + q);
    const int t = head + 16 * nq + lane;                                       // at most 15 bytes behind the last 16-byte piece
    if (t < n) rb[ph + t] = src[t];
    return ph;
}

VRG_D AreaCell walk_clamped(AreaCell c, int32_t n_in) {                        // a table made for another geometry reads nothing outside
    c.first = c.first < 0 ? 0 : (c.first > n_in - 1 ? n_in - 1 : c.first);
    c.count = c.count < 0 ? 0 : (c.count > n_in - c.first ? n_in - c.first : c.count);
    return c;
}

// One source row by one wave: `words` gets the lane's three words.  row: C values per sample, output channel c reads channel 2 - c with
// SWAP.  xc[0 .. nc): the clamped cells of the workgroup's columns; lane `lane` owns column cl = its index in xc (any other cl: none), m its
// cell.  rb: the wave's row buffer, cap the values a segment may stage.
template <uint8_t (*QUANT)(float), bool SWAP, typename T>
VRG_D void walk_row(const T* row, int C, int mode, const AreaCell* xc, int nc, int cl, const AreaCell& m, int cps, uint8_t* rb, int cap, int lane,
                    uint32_t* words) {
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    for (int c0 = 0; c0 < nc; c0 += cps) {
        const int cl_last = (c0 + cps < nc ? c0 + cps : nc) - 1;
        const int x0 = xc[c0].first;
        int n = (xc[cl_last].first + xc[cl_last].count - x0) * C;              // values of this segment; inside the row: the cells are clamped
        n = n < 0 ? 0 : (n > cap ? cap : n);                                   // (never taken: the host chose cps for this buffer)
        const int ph = walk_stage<QUANT>(row + (int64_t)x0 * C, n, rb, lane);
        walk_wave_sync();
        if (cl >= c0 && cl <= cl_last) {
            const int at = (m.first - x0) * C;
            int count = m.count;
            if (at < 0 || at + count * C > n) count = 0;                       // (never taken)
            const uint8_t* p = rb + ph + at;
            const int s0 = SWAP ? 2 : 0, s2 = SWAP ? 0 : 2;
            if (mode == GRID_GENERAL) {
                float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
                for (int k = 0; k < count; ++k, p += C) {
                    const float w = k == 0 ? m.w_first : (k == m.count - 1 ? m.w_last : m.w_mid);                   // area_weight
                    f0 = grid_term_general(f0, p[s0], w);
                    f1 = grid_term_general(f1, p[1], w);
                    f2 = grid_term_general(f2, p[s2], w);
                }
                a0 = __float_as_uint(f0); a1 = __float_as_uint(f1); a2 = __float_as_uint(f2);
            } else if (mode == GRID_LINEAR) {
                if (count > 0) {
                    const uint8_t* q = p + (count - 1) * C;
                    a0 = (uint32_t)grid_row_linear(p[s0], q[s0], m);
                    a1 = (uint32_t)grid_row_linear(p[1], q[1], m);
                    a2 = (uint32_t)grid_row_linear(p[s2], q[s2], m);
                }
            } else {
                int32_t i0 = 0, i1 = 0, i2 = 0;
                for (int k = 0; k < count; ++k, p += C) {
                    i0 = grid_term_fast(i0, p[s0]);
                    i1 = grid_term_fast(i1, p[1]);
                    i2 = grid_term_fast(i2, p[s2]);
                }
                a0 = (uint32_t)i0; a1 = (uint32_t)i1; a2 = (uint32_t)i2;
            }
        }
        walk_wave_sync();                                                      // the next segment overwrites the buffer
    }
    words[0] = a0; words[1] = a1; words[2] = a2;
}

// where the wave leaves the words of its row of batch b for lane `lane`
VRG_D uint32_t* walk_words(uint32_t* part, int b, int wave, int lane) { return part + ((b & 1) * WALK_WAVES + wave) * WALK_VALUES + lane * 3; }

// The workgroup meets; threads < WALK_VALUES fold the up to four rows of batch b (rows 4b .. 4b + 3 of the yc.count rows) in row order.
VRG_D void walk_fold(const uint32_t* part, int b, int tid, int mode, const AreaCell& yc, WalkSums& s) {
    const int rows = yc.count;
    const float w_first = yc.w_first, w_mid = yc.w_mid, w_last = yc.w_last;     // values, not places: yc stays in registers
    __syncthreads();
    if (tid < WALK_VALUES) {
#pragma unroll
        for (int w = 0; w < WALK_WAVES; ++w) {
            const int rr = b * WALK_WAVES + w;
            if (rr < rows) {
                const uint32_t v = part[((b & 1) * WALK_WAVES + w) * WALK_VALUES + tid];
                if (mode == GRID_GENERAL)
                    s.total = __float_as_uint(area_fold(__uint_as_float(s.total), __uint_as_float(v),
                                                        rr == 0 ? w_first : (rr == rows - 1 ? w_last : w_mid), rr == 0));
                else if (mode == GRID_LINEAR) {
                    if (rr == 0) s.row0 = s.row1 = v;
                    else if (rr == 1) s.row1 = v;
                } else
                    s.total += v;
            }
        }
    }
}

// the byte of a thread's folded values; inv = 1.0f / (sx * sy) of the integer rules
VRG_D uint8_t walk_byte(const WalkSums& s, int mode, const AreaCell& yc, float inv) {
    if (mode == GRID_GENERAL) return area_cast(__uint_as_float(s.total));
    if (mode == GRID_LINEAR) return grid_byte_linear((int32_t)s.row0, (int32_t)s.row1, yc);
    return area_fast_cast((int32_t)s.total, inv, mode == GRID_FAST_2X2);
}

}  // namespace vrg
