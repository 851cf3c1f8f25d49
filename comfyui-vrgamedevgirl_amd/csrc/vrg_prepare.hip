// vrg_prepare.hip -- the pixels of the Video Enhance Prepare node (VRGDGVideoEnhancePrepare.prepare, VRGDG_VideoEnhanceNodes.py:170-252 of
// the reference): source frames picked by an index list, resampled as vrg_resize_f32 resamples them, and left both as fp32 working
// frames and as the bytes _save_image_batch (:109-119) writes into its PNG files -- one pass, one launch per call.  gfx950 only.
// Arithmetic: vrg_resize_math.hpp, called, not restated: the fp32 output is bit-identical to vrg_resize_f32 for every method and
// geometry.  Plan: vrg_prepare_math.hpp.
//
// Shape of the work.  Prepare takes 4K frames DOWN (3840 x 2160 -> 960 x 544): 12 B are read per source pixel and under 1 B written, so
// the source read is everything.  k_resize_bicubic (one thread marches down an output column, source taps gathered from global memory)
// is built for the way up: at a 4x shrink neighbouring lanes' taps lie 48 B apart and every output row wants four source rows nobody
// else reads.  Here a workgroup owns a band of PREP_BAND output rows of one segment of one output frame, and
//   * walks the band's source rows in order: a row is brought through LDS ONCE with contiguous 16-byte non-temporal loads
//     (prep_stage: the frame is read once and never again, so it should not displace anything from L2), a thread takes the four x taps of its
//     column out of LDS and keeps the horizontally resampled row in a ring of four (h, 12 registers).  An output row then is
//     sum_y wy * h[y]: the same products and sums in the same order as rs_pixel.  The ring moves by as many rows as the y taps moved
//     (prep_ring_shift): four at a 4x shrink, one or none going up -- so no source row is staged twice inside a band, whatever the ratio,
//     and neighbouring bands share at most the four rows a band primes with;
//   * a source span wider than the stage buffer is walked in column segments of `cps` columns (prep_plan), as k_sheet_rows does.
// Band height and stage size.  LDS per workgroup = 16 KiB stage + 1.5 KiB bytes: nine fit the 160 KiB of a CU, so LDS never decides the
// occupancy; the registers do (90 VGPRs: five workgroups of four waves per CU, profiles/prepare_resources.txt) -- and several resident
// workgroups are what hides the load -> barrier -> taps latency of one behind its neighbours without a second buffer: a larger stage
// would buy fewer barriers per row at the price of that.  16 KiB is a 4x shrink of 256 columns of RGB (1027 px, 12.3 KB) or of
// 255 columns of RGBA: one column per thread at the node's default geometry.  Measured (profiles/prepare.json): 64 4K frames and 5
// anchors in 1.41 ms against 1.45 ms for the direct form of the same arithmetic (rs_pixel from global memory), ahead in six of seven
// alternated rounds: the stage wins at a 4x shrink, by 2.5 % -- neighbouring lanes' taps share L2 lines, so the direct form is closer
// than its 48 B stride suggests.  Band height and stage size themselves were reasoned as above, not swept.  The band: at shrinks of 4x and more no two output rows
// share a source row, so the band height buys no reuse there and is chosen for the grid: 8 rows give 68 x 4 workgroups per 960 x 544
// frame, enough to fill 256 CUs several workgroups deep from a handful of anchor frames, while the four rows a band primes with stay under a tenth
// of its reads down to a 1:1 copy.
// Bilinear, nearest and area run the direct form (rs_pixel from global memory), as in vrg_resize.hip, with the same frame pick and
// outputs.  Bytes: a row's bytes are collected in LDS and leave through pil_flat_write as whole 16-byte non-temporal pieces, the ragged
// head and tail of a run byte by byte.
#include "vrg_common.hpp"
#include "vrg_pil_resample.hpp"
#include "vrg_prepare_math.hpp"

namespace vrg {

struct PrepK {
    const float* in;                 // [frames][in_h][in_w][in_c]
    const int32_t* index;            // source frame of every output frame of this launch, or null: first + blockIdx.z
    float* out_f32;                  // [.][out_h][out_w][3] of this launch, or null
    uint8_t* out_u8;                 // the same as bytes, or null
    int64_t frames, first;
    int32_t cps;
};

// the bytes of one output row of a segment, in LDS, for pil_flat_write
struct PrepCursor {
    const uint8_t* bytes;
    int64_t e;
    __device__ __forceinline__ void seek(int64_t to) { e = to; }
    __device__ __forceinline__ uint8_t next() { return bytes[e++]; }
    static __device__ __forceinline__ float unit(uint8_t b) { return (float)b; }      // (never asked: the canvas is bytes)
};

// the source frame of output frame blockIdx.z of the launch, or -1: an index outside the batch is ignored
__device__ __forceinline__ int64_t prep_frame(const PrepK& k) {
    const int64_t f = k.index ? (int64_t)k.index[blockIdx.z] : k.first + (int64_t)blockIdx.z;
    return f >= 0 && f < k.frames ? f : -1;
}

// Output row oy, columns [c0, c1) of output frame blockIdx.z: thread tid holds column c0 + tid.  Every thread of the workgroup calls it
// (barrier); `bb` = PREP_THREADS * 3 bytes of LDS that nobody else touches before the workgroup's next barrier.
__device__ __forceinline__ void prep_emit_row(const PrepK& k, const ResizeGeom& g, int32_t oy, int32_t c0, int32_t c1, int tid, const float v[3],
                                              uint8_t* bb) {
    const bool mine = c0 + tid < c1;
    const int64_t run = (((int64_t)blockIdx.z * g.out_h + oy) * g.out_w + c0) * 3;      // first element of the row's run
    if (k.out_f32 && mine) {
        float* o = k.out_f32 + run + tid * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(v[c], o + c);
    }
    if (k.out_u8) {                                                                    // workgroup-uniform
        if (mine) {
#pragma unroll
            for (int c = 0; c < 3; ++c) bb[tid * 3 + c] = prep_byte(v[c]);
        }
        __syncthreads();
        const int64_t total = (int64_t)(c1 - c0) * 3;                                  // at most 768: 48 pieces and the ragged ends
        PilFlat f;
        pil_flat_plan(k.out_u8 + run, 1, total, PREP_THREADS, f);
        pil_flat_write(k.out_u8 + run, total, f.lead, f.pieces, (int64_t)tid, PrepCursor{bb, 0});
    }
}

// n <= PREP_STAGE_FLOATS floats from src into rb by the whole workgroup: value i lands at rb[ph + i], ph the returned phase (the float's
// index mod 4), so that the 16-byte non-temporal loads and the LDS words they fill are both aligned.  Four loads in flight per thread.
__device__ __forceinline__ int prep_stage(const float* src, int n, float* rb, int tid) {
    const int ph = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
    int head = (4 - ph) & 3;
    head = head < n ? head : n;
    const int nq = (n - head) >> 2;
    if (tid < head) rb[ph + tid] = __builtin_nontemporal_load(src + tid);
    const pil_f4* body = reinterpret_cast<const pil_f4*>(src + head);
    pil_f4* dst = reinterpret_cast<pil_f4*>(rb + ph + head);
    constexpr int DEPTH = PREP_STAGE_FLOATS / 4 / PREP_THREADS;
    pil_f4 v[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) {
        const int q = tid + i * PREP_THREADS;
        if (q < nq) v[i] = __builtin_nontemporal_load(body + q);
    }
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) {
        const int q = tid + i * PREP_THREADS;
        if (q < nq) dst[q] = v[i];
    }
    const int t = head + 4 * nq + tid;                                                  // at most 3 floats behind the last piece
    if (t < n) rb[ph + t] = __builtin_nontemporal_load(src + t);
    return ph;
}

__global__ __launch_bounds__(PREP_THREADS) void k_prepare_bicubic(PrepK k, ResizeGeom g) {
    constexpr int NT = 4;
    __shared__ __attribute__((aligned(16))) float rb[PREP_STAGE_FLOATS + 8];
    __shared__ __attribute__((aligned(16))) uint8_t bb[2][PREP_THREADS * 3];
    const int tid = (int)threadIdx.x;
    int32_t c0, c1, r0, r1;
    prep_segment(k.cps, g.out_w, (int32_t)blockIdx.x, c0, c1);
    prep_band(g.out_h, (int32_t)blockIdx.y, r0, r1);
    const int64_t f = prep_frame(k);
    if (c0 >= c1 || r0 >= r1 || f < 0) return;                                          // workgroup-uniform, as every branch around a barrier below
    int32_t lo, hi;
    const bool any = prep_source_span(g, c0, c1, lo, hi);
    const int n = (hi - lo) * g.in_c;
    if (n > PREP_STAGE_FLOATS) return;                                                  // (never with prep_plan's cps)
    const float* fin = k.in + f * (int64_t)g.in_h * g.in_w * g.in_c;

    const int32_t dx = c0 + tid - g.dx0;
    const bool in_x = c0 + tid < c1 && dx >= 0 && dx < g.dw;
    const float sx = rs_scale(g.sw, g.dw), sy = rs_scale(g.sh, g.dh);
    int32_t ix[NT];
    float wx[NT];
    rs_taps(in_x ? dx : 0, sx, g.sw, ix, wx);
#pragma unroll
    for (int i = 0; i < NT; ++i) ix[i] = (g.sx0 + ix[i] - lo) * g.in_c;                 // float offset inside the staged span (in_x only)

    float h[NT][3];
    int32_t hy[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        hy[j] = -1;
        h[j][0] = h[j][1] = h[j][2] = 0.0f;
    }
    for (int32_t oy = r0; oy < r1; ++oy) {
        const int32_t dy = oy - g.dy0;
        float val[3] = {0.0f, 0.0f, 0.0f};
        if (any && dy >= 0 && dy < g.dh) {
            int32_t iy[NT];
            float wy[NT];
            rs_taps(dy, sy, g.sh, iy, wy);
            const int s = prep_ring_shift(hy, iy);
#pragma unroll
            for (int S = 1; S < NT; ++S) {
                if (s == S) {
#pragma unroll
                    for (int j = 0; j + S < NT; ++j) {
                        h[j][0] = h[j + S][0]; h[j][1] = h[j + S][1]; h[j][2] = h[j + S][2];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (j >= NT - s) {
                    if (j > 0 && iy[j] == iy[j - 1]) {                                  // a tap clamped onto its neighbour: the same row
                        h[j][0] = h[j - 1][0]; h[j][1] = h[j - 1][1]; h[j][2] = h[j - 1][2];
                    } else {
                        const int ph = prep_stage(fin + ((int64_t)(g.sy0 + iy[j]) * g.in_w + lo) * g.in_c, n, rb, tid);
                        __syncthreads();
                        if (in_x) {
                            const float* row = rb + ph;
                            float v[3][NT];
#pragma unroll
                            for (int i = 0; i < NT; ++i) {
#pragma unroll
                                for (int c = 0; c < 3; ++c) v[c][i] = row[ix[i] + c];
                            }
#pragma unroll
                            for (int c = 0; c < 3; ++c) h[j][c] = rs_dot<NT>(wx, v[c]);
                        }
                        __syncthreads();                                                // the next row overwrites the buffer
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) hy[j] = iy[j];
            if (in_x) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float rows[NT];
#pragma unroll
                    for (int j = 0; j < NT; ++j) rows[j] = h[j][c];
                    val[c] = clamp01(rs_dot<NT>(wy, rows));
                }
            }
        }
        prep_emit_row(k, g, oy, c0, c1, tid, val, bb[oy & 1]);
    }
}

// bilinear / nearest / area: the direct form, one output pixel per thread and row
__global__ __launch_bounds__(PREP_THREADS) void k_prepare_direct(PrepK k, ResizeGeom g, int32_t method) {
    __shared__ __attribute__((aligned(16))) uint8_t bb[2][PREP_THREADS * 3];
    const int tid = (int)threadIdx.x;
    int32_t c0, c1, r0, r1;
    prep_segment(k.cps, g.out_w, (int32_t)blockIdx.x, c0, c1);
    prep_band(g.out_h, (int32_t)blockIdx.y, r0, r1);
    const int64_t f = prep_frame(k);
    if (c0 >= c1 || r0 >= r1 || f < 0) return;                                          // workgroup-uniform
    const float* fin = k.in + f * (int64_t)g.in_h * g.in_w * g.in_c;
    auto load = [&](int32_t y, int32_t x, int c) { return fin[((int64_t)y * g.in_w + x) * g.in_c + c]; };
    for (int32_t oy = r0; oy < r1; ++oy) {
        float val[3] = {0.0f, 0.0f, 0.0f};
        if (c0 + tid < c1) rs_pixel(g, method, c0 + tid, oy, load, val);
        prep_emit_row(k, g, oy, c0, c1, tid, val, bb[oy & 1]);
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" int vrg_prepare_frames_f32(const float* in, int64_t frames, int32_t in_h, int32_t in_w, int32_t in_channels,
                                      const int32_t* frame_index, int64_t n_out, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                                      int32_t out_h, int32_t out_w, int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h, int32_t method,
                                      float* out_f32, uint8_t* out_u8, void* stream) {
    const ResizeGeom g{in_h, in_w, in_channels, src_x0, src_y0, src_w, src_h, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h};
    const void *i = in, *a = out_f32, *b = out_u8, *x = frame_index;
    if (!in || (!out_f32 && !out_u8) || a == i || b == i || (a && a == b) || (x && (x == i || x == a || x == b))) return VRG_ERR_BAD_ARG;
    if (frames < 0 || n_out < 0 || method < 0 || method > 3 || !rs_geom_ok(g)) return VRG_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(in) & 3u) || (reinterpret_cast<uintptr_t>(out_f32) & 3u) || (reinterpret_cast<uintptr_t>(frame_index) & 3u))
        return VRG_ERR_BAD_ARG;
    if (n_out == 0) return VRG_OK;
    if (frames == 0 || (!frame_index && n_out > frames)) return VRG_ERR_BAD_ARG;       // no frame an output could come from
    if (!rs_sizes_ok(g)) return VRG_ERR_UNSUPPORTED;
    {   // no two of the four buffers may overlap anywhere, not only start at the same address
        const int64_t in_fe = (int64_t)in_h * in_w * in_channels, fe = (int64_t)out_h * out_w * 3;
        if (frames > 0x7fffffffffffffffll / 4 / in_fe || n_out > 0x7fffffffffffffffll / 4 / fe) return VRG_ERR_UNSUPPORTED;
        const void* at[4] = {in, out_f32, out_u8, frame_index};
        const int64_t bytes[4] = {frames * in_fe * 4, n_out * fe * 4, n_out * fe, n_out * 4};
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q)
                if (vrg_ranges_overlap(at[p], bytes[p], at[q], bytes[q])) return VRG_ERR_BAD_ARG;
    }
#if defined(VRG_LAB_VARIANT_SOURCE) && defined(LAB_PREPARE_DIRECT_BICUBIC)     /* tools/ab: bicubic through the direct form, the other side of the A/B of tools/measure_prepare.py */
    const bool staged = false;
#else
    const bool staged = method == RS_BICUBIC;
#endif
    PrepPlan p;
    if (!prep_plan(g, staged, p)) return VRG_ERR_UNSUPPORTED;
    const int64_t out_fe = (int64_t)out_h * out_w * 3;
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(n_out, [&](int64_t f0, int64_t nf) {
        const dim3 grid((uint32_t)p.segments, (uint32_t)p.bands, (uint32_t)nf);
        const PrepK k{in, frame_index ? frame_index + f0 : nullptr, out_f32 ? out_f32 + f0 * out_fe : nullptr,
                      out_u8 ? out_u8 + f0 * out_fe : nullptr, frames, f0, p.cps};
        if (staged) hipLaunchKernelGGL(k_prepare_bicubic, grid, dim3(PREP_THREADS), 0, st, k, g);
        else hipLaunchKernelGGL(k_prepare_direct, grid, dim3(PREP_THREADS), 0, st, k, g, method);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}
