// vrg_cut.hip -- the hard-cut score of the shot-aware Face Fix Prepare nodes (VRGDGFaceFixPrepareShotAware._cut_score,
// VRGDG_StandaloneFaceFixNodes.py:421-435, and the quantisation of :456) for a whole video: 64 x 64 INTER_AREA thumbnails of the quantised
// frames, their 32 x 32 hue / saturation histograms, and per consecutive pair the four integers the score is made of.  gfx950 only.
// Arithmetic: csrc/vrg_area_math.hpp.
//
// k_cut_thumbs: one workgroup (four waves) = one output row of one frame.  The order of the fp32 sums fixes what may run in parallel: source
// rows are independent until the vertical combine, cells are independent along x, the terms of one cell of one row are sequential.
//   The source rows of the output row go round the four waves.  A wave reads its row once with 16-byte loads (lane i takes floats 4i ..
//   4i + 3 from the first 16-byte boundary on; the few floats in front of and behind it go one by one), quantises them and keeps the BYTES in
//   a row buffer of its own in LDS, at the byte position of the float (all C channels: the layout of the buffer is the layout of the row).
//   Then lane d walks the taps of cell d for the three channels out of that buffer -- 64 lanes x 3 sequential sums -- and leaves the three
//   `buf` values of its (row, cell) in LDS.  A row wider than the buffer goes through in segments of whole cells (g.cps cells each).
//   After every four rows the workgroup meets once and 192 threads fold the four rows' values into their running sums in row order (two
//   sets of values, so one barrier per four rows); at the end they round and store the 192 bytes of the output row.
//   The fast path (both ratios integers) is the same walk with integer sums and no weights.
// The input is read once (rows that two output rows share are read by both: 1 row in 34 at 4K); 12 B/px with C = 3.
//
// k_cut_hist: one workgroup = one thumbnail: HSV per pixel from two small division tables made in LDS, integer histogram in LDS.
// k_cut_pair: one workgroup = one consecutive pair: D over the bytes, S11, S22, S12 over the histograms, integer adds in LDS.
#include "vrg_common.hpp"
#include "vrg_area_math.hpp"

#include <type_traits>

namespace vrg {

constexpr int CUT_WAVES = 4, CUT_THREADS = CUT_WAVES * 64;
constexpr int CUT_VALUES = AREA_OUT * 3;                                      // the values of one output row
constexpr int CUT_PART_BYTES = 2 * CUT_WAVES * CUT_VALUES * 4;                // two sets of four rows' values
constexpr int CUT_CELL_BYTES = AREA_OUT * (int)sizeof(AreaCell);
constexpr int CUT_HEAD_BYTES = CUT_PART_BYTES + CUT_CELL_BYTES;               // 7424: a multiple of 16
constexpr int CUT_ROW_MAX = ((65536 - CUT_HEAD_BYTES) / CUT_WAVES) & ~15;     // bytes of one wave's row buffer at most
static_assert(CUT_HEAD_BYTES % 16 == 0, "the row buffers start on a 16-byte boundary");

struct CutGeom {
    int32_t H, W, C, mode;
    int32_t cps;          // cells per segment: 64, 32, .. 1
    int32_t rowbuf;       // bytes of one wave's row buffer: a multiple of 16, >= the longest segment + 4
    float inv;            // fast path: 1.0f / (sx * sy)
};

typedef float cut_f4 __attribute__((ext_vector_type(4)));

// What one wave wrote to ITS row buffer is read by other lanes of the same wave only: a wave's LDS accesses execute in order, the fences
// keep the compiler from moving them across.
__device__ __forceinline__ void cut_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t cut_quant4(const cut_f4 v) {
    return (uint32_t)area_quant(v.x) | ((uint32_t)area_quant(v.y) << 8) | ((uint32_t)area_quant(v.z) << 16) | ((uint32_t)area_quant(v.w) << 24);
}

template <bool FAST>
__global__ __launch_bounds__(CUT_THREADS) void k_cut_thumbs(const float* __restrict__ in, uint8_t* __restrict__ out, const AreaCell* __restrict__ taps,
                                                            CutGeom g) {
    typedef typename std::conditional<FAST, int32_t, float>::type acc_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t cut_lds[];
    acc_t* part = reinterpret_cast<acc_t*>(cut_lds);                          // [2][CUT_WAVES][CUT_VALUES]
    AreaCell* xc = reinterpret_cast<AreaCell*>(cut_lds + CUT_PART_BYTES);     // [64]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t* rb = cut_lds + CUT_HEAD_BYTES + wave * g.rowbuf;
    const int64_t frame = (int64_t)(blockIdx.x >> 6);
    const int dy = (int)(blockIdx.x & 63u);

    for (int i = tid; i < AREA_OUT * 5; i += CUT_THREADS)
        reinterpret_cast<uint32_t*>(xc)[i] = reinterpret_cast<const uint32_t*>(taps)[i];
    AreaCell yc = taps[AREA_OUT + dy];
    // a table made for another geometry must not carry a read outside the frame: never taken with the table of vrg_area_taps
    yc.first = yc.first < 0 ? 0 : (yc.first > g.H - 1 ? g.H - 1 : yc.first);
    yc.count = yc.count < 0 ? 0 : (yc.count > g.H - yc.first ? g.H - yc.first : yc.count);
    __syncthreads();
    if (tid < AREA_OUT) {
        AreaCell c = xc[tid];
        c.first = c.first < 0 ? 0 : (c.first > g.W - 1 ? g.W - 1 : c.first);
        c.count = c.count < 0 ? 0 : (c.count > g.W - c.first ? g.W - c.first : c.count);
        xc[tid] = c;
    }
    __syncthreads();

    const int C = g.C;
    const float* fin = in + frame * (int64_t)g.H * g.W * C;
    const int m_first = xc[lane].first, m_count = xc[lane].count;
    const float m_wf = xc[lane].w_first, m_wm = xc[lane].w_mid, m_wl = xc[lane].w_last;
    const int y_count = yc.count;
    const float y_wf = yc.w_first, y_wm = yc.w_mid, y_wl = yc.w_last;
    acc_t total = 0;
    const int batches = (yc.count + CUT_WAVES - 1) / CUT_WAVES;
    for (int b = 0; b < batches; ++b) {
        const int r = b * CUT_WAVES + wave;
        if (r < yc.count) {                                                    // wave-uniform
            const float* row = fin + (int64_t)(yc.first + r) * g.W * C;
            acc_t acc0 = 0, acc1 = 0, acc2 = 0;
            for (int d0 = 0; d0 < AREA_OUT; d0 += g.cps) {
                const int dl = (d0 + g.cps < AREA_OUT ? d0 + g.cps : AREA_OUT) - 1;
                const int x0 = xc[d0].first;
                int n = (xc[dl].first + xc[dl].count - x0) * C;                // floats of this segment
                n = n < 0 ? 0 : (n > g.rowbuf - 4 ? g.rowbuf - 4 : n);          // (never taken: the entry point sized the buffer)
                const float* src = row + (int64_t)x0 * C;
                const int ph = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);       // float i of the segment -> byte ph + i of the buffer
                int head = (4 - ph) & 3;
                head = head < n ? head : n;
                const int nq = (n - head) >> 2;
                if (lane < head) rb[ph + lane] = area_quant(src[lane]);
                const cut_f4* body = reinterpret_cast<const cut_f4*>(src + head);
                uint32_t* dst = reinterpret_cast<uint32_t*>(rb + ph + head);
                int q = lane;
                for (; q + 192 < nq; q += 256) {                               // four loads in flight per lane
                    const cut_f4 v0 = __builtin_nontemporal_load(body + q), v1 = __builtin_nontemporal_load(body + q + 64);
                    const cut_f4 v2 = __builtin_nontemporal_load(body + q + 128), v3 = __builtin_nontemporal_load(body + q + 192);
                    dst[q] = cut_quant4(v0);
                    dst[q + 64] = cut_quant4(v1);
                    dst[q + 128] = cut_quant4(v2);
                    dst[q + 192] = cut_quant4(v3);
                }
                for (; q < nq; q += 64) dst[q] = cut_quant4(__builtin_nontemporal_load(body + q));
                const int t = head + 4 * nq + lane;
                if (t < n) rb[ph + t] = area_quant(src[t]);
                cut_wave_sync();
                if (lane >= d0 && lane <= dl) {
                    const int at = (m_first - x0) * C;
                    int count = m_count;
                    if (at < 0 || at + count * C > n) count = 0;               // (never taken)
                    const uint8_t* p = rb + ph + at;
                    for (int k = 0; k < count; ++k, p += C) {
                        if (FAST) {
                            acc0 += (acc_t)p[0];
                            acc1 += (acc_t)p[1];
                            acc2 += (acc_t)p[2];
                        } else {
                            const float w = k == 0 ? m_wf : (k == m_count - 1 ? m_wl : m_wm);      // area_weight
                            acc0 = (acc_t)area_add((float)acc0, p[0], w);
                            acc1 = (acc_t)area_add((float)acc1, p[1], w);
                            acc2 = (acc_t)area_add((float)acc2, p[2], w);
                        }
                    }
                }
                cut_wave_sync();                                               // the next segment overwrites the buffer
            }
            acc_t* mine_out = part + ((b & 1) * CUT_WAVES + wave) * CUT_VALUES + lane * 3;
            mine_out[0] = acc0; mine_out[1] = acc1; mine_out[2] = acc2;
        }
        __syncthreads();
        if (tid < CUT_VALUES) {
#pragma unroll
            for (int w = 0; w < CUT_WAVES; ++w) {
                const int rr = b * CUT_WAVES + w;
                if (rr < yc.count) {
                    const acc_t v = part[((b & 1) * CUT_WAVES + w) * CUT_VALUES + tid];
                    if (FAST) total += v;
                    else total = (acc_t)area_fold((float)total, (float)v, rr == 0 ? y_wf : (rr == y_count - 1 ? y_wl : y_wm), rr == 0);
                }
            }
        }
    }
    if (tid < CUT_VALUES) {
        uint8_t o;
        if (FAST) o = area_fast_cast((int32_t)total, g.inv, g.mode == AREA_FAST_2X2);
        else o = area_cast((float)total);
        out[(frame * AREA_OUT + dy) * CUT_VALUES + tid] = o;
    }
}

__global__ __launch_bounds__(256) void k_cut_hist(const uint8_t* __restrict__ thumbs, int32_t* __restrict__ hist) {
    __shared__ int32_t h[AREA_HIST_BINS], sdiv[256], hdiv[256];
    const int tid = (int)threadIdx.x;
    const uint8_t* t = thumbs + (int64_t)blockIdx.x * AREA_THUMB_BYTES;
    sdiv[tid] = area_sdiv(tid);
    hdiv[tid] = area_hdiv(tid);
#pragma unroll
    for (int i = 0; i < AREA_HIST_BINS / 256; ++i) h[tid + 256 * i] = 0;
    __syncthreads();
    for (int p = tid; p < AREA_OUT * AREA_OUT; p += 256) {
        const int bin = area_hsv_bin(t[3 * p], t[3 * p + 1], t[3 * p + 2], [&](int32_t v) { return sdiv[v]; }, [&](int32_t d) { return hdiv[d]; });
        atomicAdd(&h[bin], 1);
    }
    __syncthreads();
    int32_t* o = hist + (int64_t)blockIdx.x * AREA_HIST_BINS;
#pragma unroll
    for (int i = 0; i < AREA_HIST_BINS / 256; ++i) o[tid + 256 * i] = h[tid + 256 * i];
}

// every sum fits int32: D <= 255 * 12288, S11, S22, S12 <= 4096^2
__global__ __launch_bounds__(256) void k_cut_pair(const uint8_t* __restrict__ thumbs, const int32_t* __restrict__ hist, int64_t* __restrict__ sums) {
    __shared__ int32_t acc[4];
    const int tid = (int)threadIdx.x;
    const uint8_t* a = thumbs + (int64_t)blockIdx.x * AREA_THUMB_BYTES;
    const uint8_t* b = a + AREA_THUMB_BYTES;
    const int32_t* ha = hist + (int64_t)blockIdx.x * AREA_HIST_BINS;
    const int32_t* hb = ha + AREA_HIST_BINS;
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    int32_t d = 0, s11 = 0, s22 = 0, s12 = 0;
    for (int i = tid; i < AREA_THUMB_BYTES; i += 256) {
        const int32_t x = (int32_t)a[i] - (int32_t)b[i];
        d += x < 0 ? -x : x;
    }
    for (int i = tid; i < AREA_HIST_BINS; i += 256) {
        const int32_t p = ha[i], q = hb[i];
        s11 += p * p;
        s22 += q * q;
        s12 += p * q;
    }
    atomicAdd(&acc[0], d);
    atomicAdd(&acc[1], s11);
    atomicAdd(&acc[2], s22);
    atomicAdd(&acc[3], s12);
    __syncthreads();
    if (tid < 4) sums[(int64_t)blockIdx.x * 4 + tid] = (int64_t)acc[tid];
}

// cells per segment and the row buffer for this geometry; false: even one cell does not fit
static bool cut_segments(const AreaCell* xc, int32_t C, int32_t& cps, int32_t& rowbuf) {
    for (cps = AREA_OUT; cps >= 1; cps >>= 1) {
        int64_t longest = 0;
        for (int d0 = 0; d0 < AREA_OUT; d0 += cps) {
            const int dl = d0 + cps - 1;
            const int64_t n = (int64_t)(xc[dl].first + xc[dl].count - xc[d0].first) * C;
            longest = n > longest ? n : longest;
        }
        if (longest + 4 <= CUT_ROW_MAX) {
            rowbuf = (int32_t)((longest + 4 + 15) & ~(int64_t)15);
            return true;
        }
    }
    return false;
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_area_taps(int32_t in_h, int32_t in_w, void* taps_host) {
    if (!taps_host || in_h < AREA_OUT || in_w < AREA_OUT) return VRG_ERR_BAD_ARG;
    area_fill_cells(in_h, in_w, reinterpret_cast<AreaCell*>(taps_host));
    return VRG_OK;
}

int vrg_cut_thumbs_f32(const float* in, uint8_t* out, int64_t frames, int32_t height, int32_t width, int32_t channels, const void* taps,
                       void* stream) {
    if (!in || !out || !taps || (reinterpret_cast<uintptr_t>(in) & 3u) != 0 || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || frames < 0 ||
        height < AREA_OUT || width < AREA_OUT || channels < 3 || channels > 4 || reinterpret_cast<const void*>(in) == reinterpret_cast<const void*>(out))
        return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if ((int64_t)height * width * channels > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    AreaCell cells[2 * AREA_OUT];
    area_fill_cells(height, width, cells);
    CutGeom g{height, width, channels, area_mode(height, width), 0, 0, 1.0f / (float)((width / AREA_OUT) * (height / AREA_OUT))};
    if (!cut_segments(cells, channels, g.cps, g.rowbuf)) return VRG_ERR_UNSUPPORTED;
    const size_t lds = (size_t)CUT_HEAD_BYTES + (size_t)CUT_WAVES * (size_t)g.rowbuf;
    const int64_t fe = (int64_t)height * width * channels;
    const int64_t step = 0x7fffffffll / AREA_OUT;                              // frames per launch
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        const dim3 grid((uint32_t)(nf * AREA_OUT));
        const AreaCell* t = reinterpret_cast<const AreaCell*>(taps);
        if (g.mode == AREA_GENERAL)
            hipLaunchKernelGGL((k_cut_thumbs<false>), grid, dim3(CUT_THREADS), lds, (hipStream_t)stream, in + f0 * fe, out + f0 * AREA_THUMB_BYTES, t, g);
        else
            hipLaunchKernelGGL((k_cut_thumbs<true>), grid, dim3(CUT_THREADS), lds, (hipStream_t)stream, in + f0 * fe, out + f0 * AREA_THUMB_BYTES, t, g);
        VRG_CHECK_LAUNCH();
    }
    return VRG_OK;
}

int vrg_cut_hist_u8(const uint8_t* thumbs, int32_t* hist, int64_t frames, void* stream) {
    if (!thumbs || !hist || (reinterpret_cast<uintptr_t>(hist) & 3u) != 0 || frames < 0 || frames > 0x7fffffffll) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    hipLaunchKernelGGL(k_cut_hist, dim3((uint32_t)frames), dim3(256), 0, (hipStream_t)stream, thumbs, hist);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_cut_pair_sums(const uint8_t* thumbs, const int32_t* hist, int64_t* sums, int64_t frames, void* stream) {
    if (!thumbs || !hist || !sums || (reinterpret_cast<uintptr_t>(hist) & 3u) != 0 || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0 || frames < 0 ||
        frames > 0x7fffffffll)
        return VRG_ERR_BAD_ARG;
    if (frames < 2) return VRG_OK;
    hipLaunchKernelGGL(k_cut_pair, dim3((uint32_t)(frames - 1)), dim3(256), 0, (hipStream_t)stream, thumbs, hist, sums);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
