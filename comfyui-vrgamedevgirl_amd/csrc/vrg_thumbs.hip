// vrg_thumbs.hip -- the input of the landmark estimator (VRGDGFaceFixCompositeLandmarkAligned._landmarks, VRGDG_StandaloneFaceFixNodes.py:
// 955-979 of the reference): the 320 x 320 B,G,R thumbnails cv2.cvtColor(cv2.resize(rgb, (320, 320), INTER_AREA), COLOR_RGB2BGR) makes of
// the packed face images of vrg_face_bytes_u8, for a list of descriptors in one launch.  gfx950 only.  Arithmetic: csrc/vrg_grid_math.hpp
// (nothing of its own: csrc/vrg_thumbs_math.hpp holds the descriptor's rules and the host loop).
//
// k_face_thumbs: one workgroup (four waves) = 64 columns of one row of one thumbnail, 5 x 320 workgroups per descriptor.  The walk is the
// one of k_grid_tiles (csrc/vrg_grid.hip) for byte sources with three channels, whose comment says why the order of the fp32 sums allows
// this much and no more: the source rows of the output row go round the four waves; a wave stages the bytes its 64 columns need once with
// 16-byte loads in a row buffer of its own in LDS (the image starts at any byte, so the buffer keeps the phase of the address mod 16);
// lane d walks the taps of column d for the three channels, reading channel 2 - c for output channel c; after every four rows the
// workgroup meets and 192 threads fold the rows' values in row order.  Columns whose samples do not fit the row buffer go through it
// desc.cps columns at a time.  The workgroup's 192 bytes are put together in LDS and leave as twelve 16-byte stores, always aligned: 192,
// 960 and 307,200 are multiples of 16 and `out` is 16-byte aligned.  Every byte of a thumbnail is written once.  When both axes shrink a
// source byte is read once, twice for the rows two output rows share; when an axis enlarges (a box below 320: at most 307 KB) the one or
// two source rows of an output row are read again by its neighbours, out of the cache.
#include "vrg_common.hpp"
#include "vrg_thumbs_math.hpp"

namespace vrg {

constexpr int TH_WAVES = 4, TH_THREADS = TH_WAVES * 64;
constexpr int TH_VALUES = GRID_LANES * 3;                                      // the values of one workgroup
constexpr int TH_PART_BYTES = 2 * TH_WAVES * TH_VALUES * 4;                    // two sets of four rows' words
constexpr int TH_CELL_BYTES = GRID_LANES * (int)sizeof(AreaCell);
constexpr int TH_OUT_BYTES = 256;                                              // the bytes of the workgroup (192 used)
constexpr int TH_HEAD_BYTES = TH_PART_BYTES + TH_CELL_BYTES + TH_OUT_BYTES;
constexpr int TH_ROWBUF = GRID_ROW_VALUES + 16;                                // a staged byte lies at the byte phase of its source
constexpr int TH_LDS_BYTES = TH_HEAD_BYTES + TH_WAVES * TH_ROWBUF;
static_assert(TH_HEAD_BYTES % 16 == 0 && TH_ROWBUF % 16 == 0 && (TH_PART_BYTES + TH_CELL_BYTES) % 16 == 0,
              "the row buffers and the output bytes start on a 16-byte boundary");

typedef uint32_t th_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void th_wave_sync() {                               // cut_wave_sync of vrg_cut.hip
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n bytes from src into rb: byte i lands at rb[ph + i], ph = the address mod 16 (returned), so that the 16-byte loads and the LDS words
// they fill are both aligned.  n <= GRID_ROW_VALUES.  Nothing outside src[0 .. n) is read.
__device__ __forceinline__ int th_stage(const uint8_t* src, int n, uint8_t* rb, int lane) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    int head = (16 - ph) & 15;
    head = head < n ? head : n;
    const int nq = (n - head) >> 4;
    if (lane < head) rb[ph + lane] = src[lane];
    const th_u4* body = reinterpret_cast<const th_u4*>(src + head);
    th_u4* dst = reinterpret_cast<th_u4*>(rb + ph + head);
    for (int q = lane; q < nq; q += 64) dst[q] = __builtin_nontemporal_load(body + q);
    const int t = head + 16 * nq + lane;                                       // at most 15 bytes behind the last 16-byte piece
    if (t < n) rb[ph + t] = src[t];
    return ph;
}

__device__ __forceinline__ AreaCell th_clamped(AreaCell c, int32_t n_in) {     // a table made for another geometry reads nothing outside
    c.first = c.first < 0 ? 0 : (c.first > n_in - 1 ? n_in - 1 : c.first);
    c.count = c.count < 0 ? 0 : (c.count > n_in - c.first ? n_in - c.first : c.count);
    return c;
}

__global__ __launch_bounds__(TH_THREADS) void k_face_thumbs(const uint8_t* __restrict__ generated, const uint8_t* __restrict__ source,
                                                            int64_t n_bytes, const vrg_thumb_desc* __restrict__ descs,
                                                            uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[TH_LDS_BYTES];
    uint32_t* part = reinterpret_cast<uint32_t*>(lds);                        // [2][TH_WAVES][TH_VALUES]
    AreaCell* xc = reinterpret_cast<AreaCell*>(lds + TH_PART_BYTES);          // [64]
    uint8_t* ob = lds + TH_PART_BYTES + TH_CELL_BYTES;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t* rb = lds + TH_HEAD_BYTES + wave * TH_ROWBUF;

    const vrg_thumb_desc d = descs[blockIdx.y];
    const int seg = (int)(blockIdx.x % (uint32_t)THUMB_SEGMENTS), ty = (int)(blockIdx.x / (uint32_t)THUMB_SEGMENTS);
    const int tx0 = seg * GRID_LANES;
    // a descriptor the host check refuses writes nothing (workgroup-uniform)
    const uint8_t* image = d.which == 0 ? generated : (d.which == 1 ? source : nullptr);
    if (!image || !d.xtab || !d.ytab || d.mode < GRID_COPY || d.mode > GRID_LINEAR || !thumb_image_fits(d.offset, d.box_w, d.box_h, n_bytes)) return;
    image += d.offset;
    const int mode = d.mode, W = d.box_w;

    xc[lane] = th_clamped(reinterpret_cast<const AreaCell*>(d.xtab)[tx0 + lane], W);        // the four waves write the same 64 records
    const AreaCell yc = th_clamped(reinterpret_cast<const AreaCell*>(d.ytab)[ty], d.box_h);
    __syncthreads();
    const AreaCell m = xc[lane];
    const int cps = d.cps < 1 ? 1 : (d.cps > GRID_LANES ? GRID_LANES : d.cps);

    uint32_t total = 0, row0 = 0, row1 = 0;
    const int batches = (yc.count + TH_WAVES - 1) / TH_WAVES;
    for (int b = 0; b < batches; ++b) {
        const int r = b * TH_WAVES + wave;
        if (r < yc.count) {                                                    // wave-uniform
            const uint8_t* row = image + (int64_t)(yc.first + r) * W * 3;
            uint32_t a0 = 0, a1 = 0, a2 = 0;
            for (int c0 = 0; c0 < GRID_LANES; c0 += cps) {
                const int cl_last = (c0 + cps < GRID_LANES ? c0 + cps : GRID_LANES) - 1;
                const int x0 = xc[c0].first;
                int n = (xc[cl_last].first + xc[cl_last].count - x0) * 3;      // bytes of this segment; inside the row: the cells are clamped
                n = n < 0 ? 0 : (n > GRID_ROW_VALUES ? GRID_ROW_VALUES : n);   // (never taken with the cps of vrg_grid_plan)
                const int ph = th_stage(row + (int64_t)x0 * 3, n, rb, lane);
                th_wave_sync();
                if (lane >= c0 && lane <= cl_last) {
                    const int at = (m.first - x0) * 3;
                    int count = m.count;
                    if (at < 0 || at + count * 3 > n) count = 0;               // (never taken)
                    const uint8_t* p = rb + ph + at;
                    if (mode == GRID_GENERAL) {
                        float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
                        for (int k = 0; k < count; ++k, p += 3) {
                            const float w = k == 0 ? m.w_first : (k == m.count - 1 ? m.w_last : m.w_mid);          // area_weight
                            f0 = grid_term_general(f0, p[2], w);
                            f1 = grid_term_general(f1, p[1], w);
                            f2 = grid_term_general(f2, p[0], w);
                        }
                        a0 = __float_as_uint(f0); a1 = __float_as_uint(f1); a2 = __float_as_uint(f2);
                    } else if (mode == GRID_LINEAR) {
                        if (count > 0) {
                            const uint8_t* q = p + (count - 1) * 3;
                            a0 = (uint32_t)grid_row_linear(p[2], q[2], m);
                            a1 = (uint32_t)grid_row_linear(p[1], q[1], m);
                            a2 = (uint32_t)grid_row_linear(p[0], q[0], m);
                        }
                    } else {
                        int32_t i0 = 0, i1 = 0, i2 = 0;
                        for (int k = 0; k < count; ++k, p += 3) {
                            i0 = grid_term_fast(i0, p[2]);
                            i1 = grid_term_fast(i1, p[1]);
                            i2 = grid_term_fast(i2, p[0]);
                        }
                        a0 = (uint32_t)i0; a1 = (uint32_t)i1; a2 = (uint32_t)i2;
                    }
                }
                th_wave_sync();                                                // the next segment overwrites the buffer
            }
            uint32_t* mine_out = part + ((b & 1) * TH_WAVES + wave) * TH_VALUES + lane * 3;
            mine_out[0] = a0; mine_out[1] = a1; mine_out[2] = a2;
        }
        __syncthreads();
        if (tid < TH_VALUES) {
#pragma unroll
            for (int w = 0; w < TH_WAVES; ++w) {
                const int rr = b * TH_WAVES + w;
                if (rr < yc.count) {
                    const uint32_t v = part[((b & 1) * TH_WAVES + w) * TH_VALUES + tid];
                    if (mode == GRID_GENERAL)
                        total = __float_as_uint(area_fold(__uint_as_float(total), __uint_as_float(v),
                                                          rr == 0 ? yc.w_first : (rr == yc.count - 1 ? yc.w_last : yc.w_mid), rr == 0));
                    else if (mode == GRID_LINEAR) {
                        if (rr == 0) row0 = row1 = v;
                        else if (rr == 1) row1 = v;
                    } else
                        total += v;
                }
            }
        }
    }

    // the 192 bytes of this workgroup: value tid = column tx0 + tid / 3, channel tid % 3 (B, G, R)
    if (tid < TH_VALUES) {
        uint8_t o;
        if (mode == GRID_GENERAL) o = area_cast(__uint_as_float(total));
        else if (mode == GRID_LINEAR) o = grid_byte_linear((int32_t)row0, (int32_t)row1, yc);
        else o = area_fast_cast((int32_t)total, d.inv, mode == GRID_FAST_2X2);
        ob[tid] = o;
    }
    __syncthreads();
    if (tid < TH_VALUES / 16) {
        uint8_t* dst = out + (int64_t)blockIdx.y * THUMB_BYTES + (int64_t)ty * THUMB_ROW_BYTES + tx0 * 3;
        reinterpret_cast<th_u4*>(dst)[tid] = reinterpret_cast<const th_u4*>(ob)[tid];
    }
}

static bool th_overlap(const uint8_t* a, int64_t a_bytes, const uint8_t* b, int64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    if (!a || !b) return false;
    return a0 == b0 || (a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes);
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_face_thumbs_check(const vrg_thumb_desc* desc_host, int64_t n_desc, int64_t n_bytes, int has_source) {
    if (n_desc < 0 || n_bytes < 0 || (n_desc > 0 && !desc_host)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_desc; ++i)
        if (!thumb_desc_ok(desc_host[i], n_bytes, has_source != 0)) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

int vrg_face_thumbs_u8(const uint8_t* generated, const uint8_t* source, int64_t n_bytes, const vrg_thumb_desc* desc, int64_t n_desc,
                       uint8_t* out, void* stream) {
    if (n_desc < 0 || n_bytes < 0) return VRG_ERR_BAD_ARG;
    if (n_desc == 0) return VRG_OK;
    if (!generated || !desc || !out || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0 || (reinterpret_cast<uintptr_t>(out) & 15u) != 0) return VRG_ERR_BAD_ARG;
    if (n_desc > INT64_MAX / THUMB_BYTES) return VRG_ERR_BAD_ARG;
    if (th_overlap(out, n_desc * THUMB_BYTES, generated, n_bytes) || th_overlap(out, n_desc * THUMB_BYTES, source, n_bytes)) return VRG_ERR_BAD_ARG;
    return launch_chunks(n_desc, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL(k_face_thumbs, dim3((uint32_t)(THUMB_SEGMENTS * THUMB_SIDE), (uint32_t)count), dim3(TH_THREADS), 0, (hipStream_t)stream,
                           generated, source, n_bytes, desc + first, out + first * THUMB_BYTES);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // extern "C"
