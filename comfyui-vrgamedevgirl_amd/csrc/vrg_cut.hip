// vrg_cut.hip -- the hard-cut score of the shot-aware Face Fix Prepare nodes (VRGDGFaceFixPrepareShotAware._cut_score,
// VRGDG_StandaloneFaceFixNodes.py:421-435, and the quantisation of :456) for a whole video: 64 x 64 INTER_AREA thumbnails of the quantised
// frames, their 32 x 32 hue / saturation histograms, and per consecutive pair the four integers the score is made of.  gfx950 only.
// Arithmetic: csrc/vrg_area_math.hpp.
//
// k_cut_thumbs: one workgroup (four waves) = one output row of one frame, on the source walk of csrc/vrg_area_walk.hpp, whose comment says why
// the order of the fp32 sums allows this much parallelism and no more.  The frames are fp32 and quantised by area_quant (round half to
// even) as they are staged; the rule is a compile-time constant, general or integer sums, so the walk's other rules fold away.  The row
// buffers are dynamic LDS sized by cut_segments for the geometry; the 192 bytes of the output row are stored as bytes.
// The input is read once (rows that two output rows share are read by both: 1 row in 34 at 4K); 12 B/px with C = 3.
//
// k_cut_hist: one workgroup = one thumbnail: HSV per pixel from two small division tables made in LDS, integer histogram in LDS.
// k_cut_pair: one workgroup = one consecutive pair: D over the bytes, S11, S22, S12 over the histograms, integer adds in LDS.
#include "vrg_common.hpp"
#include "vrg_area_walk.hpp"

namespace vrg {

constexpr int CUT_HEAD_BYTES = WALK_PART_BYTES + WALK_CELL_BYTES;             // 7424: a multiple of 16
constexpr int CUT_ROW_MAX = ((65536 - CUT_HEAD_BYTES) / WALK_WAVES) & ~15;    // bytes of one wave's row buffer at most
static_assert(CUT_HEAD_BYTES % 16 == 0, "the row buffers start on a 16-byte boundary");

struct CutGeom {
    int32_t H, W, C, mode;
    int32_t cps;          // cells per segment: 64, 32, .. 1
    int32_t rowbuf;       // bytes of one wave's row buffer: a multiple of 16, >= the longest segment + 4
    float inv;            // fast path: 1.0f / (sx * sy)
};

template <bool FAST>
__global__ __launch_bounds__(WALK_THREADS) void k_cut_thumbs(const float* __restrict__ in, uint8_t* __restrict__ out, const AreaCell* __restrict__ taps,
                                                             CutGeom g) {
    constexpr int RULE = FAST ? GRID_FAST : GRID_GENERAL;                      // of the walk and the fold: 2 x 2 differs in the last step alone
    extern __shared__ __attribute__((aligned(16))) uint8_t cut_lds[];
    uint32_t* part = reinterpret_cast<uint32_t*>(cut_lds);                    // [2][WALK_WAVES][WALK_VALUES]
    AreaCell* xc = reinterpret_cast<AreaCell*>(cut_lds + WALK_PART_BYTES);    // [64]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t* rb = cut_lds + CUT_HEAD_BYTES + wave * g.rowbuf;
    const int64_t frame = (int64_t)(blockIdx.x >> 6);
    const int dy = (int)(blockIdx.x & 63u);

    for (int i = tid; i < AREA_OUT * 5; i += WALK_THREADS)
        reinterpret_cast<uint32_t*>(xc)[i] = reinterpret_cast<const uint32_t*>(taps)[i];
    const AreaCell yc = walk_clamped(taps[AREA_OUT + dy], g.H);                // never changes the table of vrg_area_taps
    __syncthreads();
    if (tid < AREA_OUT) xc[tid] = walk_clamped(xc[tid], g.W);
    __syncthreads();

    const int C = g.C;
    const float* fin = in + frame * (int64_t)g.H * g.W * C;
    const AreaCell m = xc[lane];
    WalkSums s{0, 0, 0};
    const int batches = (yc.count + WALK_WAVES - 1) / WALK_WAVES;
    for (int b = 0; b < batches; ++b) {
        const int r = b * WALK_WAVES + wave;
        if (r < yc.count)                                                      // wave-uniform
            walk_row<area_quant, false>(fin + (int64_t)(yc.first + r) * g.W * C, C, RULE, xc, AREA_OUT, lane, m, g.cps, rb, g.rowbuf - 4, lane,
                                        walk_words(part, b, wave, lane));
        walk_fold(part, b, tid, RULE, yc, s);
    }
    if (tid < WALK_VALUES)
        out[(frame * AREA_OUT + dy) * WALK_VALUES + tid] = walk_byte(s, FAST && g.mode == AREA_FAST_2X2 ? GRID_FAST_2X2 : RULE, yc, g.inv);
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
    const size_t lds = (size_t)CUT_HEAD_BYTES + (size_t)WALK_WAVES * (size_t)g.rowbuf;
    const int64_t fe = (int64_t)height * width * channels;
    const int64_t step = 0x7fffffffll / AREA_OUT;                              // frames per launch
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        const dim3 grid((uint32_t)(nf * AREA_OUT));
        const AreaCell* t = reinterpret_cast<const AreaCell*>(taps);
        if (g.mode == AREA_GENERAL)
            hipLaunchKernelGGL((k_cut_thumbs<false>), grid, dim3(WALK_THREADS), lds, (hipStream_t)stream, in + f0 * fe, out + f0 * AREA_THUMB_BYTES, t, g);
        else
            hipLaunchKernelGGL((k_cut_thumbs<true>), grid, dim3(WALK_THREADS), lds, (hipStream_t)stream, in + f0 * fe, out + f0 * AREA_THUMB_BYTES, t, g);
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
