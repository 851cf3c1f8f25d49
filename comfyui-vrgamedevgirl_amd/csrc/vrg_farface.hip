// vrg_farface.hip -- the pixels of the far-face repair composite (reference scripts/far_face_repair_backend.py: composite :339-371) on
// decoded bytes: Pillow's LANCZOS resize, its GaussianBlur of the soft-ellipse mask, numpy's fp32 mean shift and Image.paste under an L
// mask, each byte for byte.  gfx950 only.  Arithmetic: csrc/vrg_pil_math.hpp; the resize's tables, tap records and passes:
// csrc/vrg_pil_resample.hpp, whose four HOST table functions (vrg_pil_lanczos_*, vrg_pil_filter_*) are exported below.
//
// Shape of the work.  A job is a batch of byte frames, at most one box per frame, and one repaired crop (of any size) per box.
//   k_pil_resize_h / _v   Image.resize: blockIdx.y = the output image, so its record is wave-uniform; one thread = one pixel of the pass,
//                         its taps and bounds out of the host-made integer tables.  The horizontal pass writes the rounded byte image the
//                         vertical pass reads (`tmp`); a pass whose size does not change is skipped.
//   k_pil_mask_h / _v     the masks, one per distinct (w, h, feather): one workgroup = one row (then one column) held in LDS through its
//                         three box passes; every pass is a block-wide prefix sum and then one independent pixel per lane
//                         (pil_box_pixel) -- nothing walks along a line.
//   k_np_means            numpy's sequential fp32 means: one workgroup per frame walks its box in chunks of NP_CHUNK pixels; a lane folds
//                         NP_RUN consecutive pixels into six maps, the maps are reduced pairwise in order through LDS, and the chunk is
//                         applied at once unless a sum would reach its next power of two -- then one lane per sum walks the chunk with
//                         real fp32 adds (np_means_block of csrc/vrg_farface_body.hpp, shared with csrc/vrg_farface_packed.hip).
//   k_pil_paste           ONE pass over the output batch as a flat run of bytes, 16 per thread: a piece that misses the box is one 16-byte
//                         non-temporal load and store, a piece that touches it is rebuilt byte by byte (move_bytes of
//                         csrc/vrg_byte_mover.hpp, shared with vrg_ff_composite_u8).
#include "vrg_byte_mover.hpp"
#include "vrg_farface_body.hpp"

namespace vrg {

struct PilResizeGeom {
    int64_t src_bytes, table_ints, tmp_bytes, dst_bytes;
    int32_t C;
};

__device__ __forceinline__ bool pil_resize_ok(const vrg_pil_resize_desc& d, const PilResizeGeom& g) {
    if (d.in_w < 1 || d.in_h < 1 || d.out_w < 1 || d.out_h < 1) return false;
    const bool hp = d.in_w != d.out_w, vp = d.in_h != d.out_h;
    if (!span_fits(d.src_offset, (int64_t)d.in_h * d.in_w * g.C, g.src_bytes)) return false;
    if (!span_fits(d.dst_offset, (int64_t)d.out_h * d.out_w * g.C, g.dst_bytes)) return false;
    if (hp && (d.h_ksize < 1 || !span_fits(d.h_table, (int64_t)d.out_w * (2 + d.h_ksize), g.table_ints))) return false;
    if (vp && (d.v_ksize < 1 || !span_fits(d.v_table, (int64_t)d.out_h * (2 + d.v_ksize), g.table_ints))) return false;
    if (hp && vp && !span_fits(d.tmp_offset, (int64_t)d.in_h * d.out_w * g.C, g.tmp_bytes)) return false;
    return true;
}

template <int C>
__global__ __launch_bounds__(256) void k_pil_resize_h(const uint8_t* __restrict__ src, const vrg_pil_resize_desc* __restrict__ desc,
                                                       const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst,
                                                       PilResizeGeom g) {
    const vrg_pil_resize_desc d = desc[blockIdx.y];                      // wave-uniform
    if (!pil_resize_ok(d, g) || d.in_w == d.out_w) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)d.in_h * d.out_w) return;
    const int32_t y = (int32_t)(p / d.out_w), x = (int32_t)(p - (int64_t)y * d.out_w);
    uint8_t* out = (d.in_h != d.out_h ? tmp + d.tmp_offset : dst + d.dst_offset) + p * C;
    uint8_t o[C];
    const PilRecord t = pil_record(tables + d.h_table, d.out_w, x, d.h_ksize, 0, d.in_w);
    if (t.ok) {
        const uint8_t* row = src + d.src_offset + ((int64_t)y * d.in_w + t.first) * C;
        pil_taps<C>(t.w, t.n, [&](int32_t i, int c) { return row[i * C + c]; }, o);
    } else {
        for (int c = 0; c < C; ++c) o[c] = 0;
    }
    for (int c = 0; c < C; ++c) out[c] = o[c];
}

template <int C>
__global__ __launch_bounds__(256) void k_pil_resize_v(const uint8_t* __restrict__ src, const vrg_pil_resize_desc* __restrict__ desc,
                                                       const int32_t* __restrict__ tables, const uint8_t* __restrict__ tmp,
                                                       uint8_t* __restrict__ dst, PilResizeGeom g) {
    const vrg_pil_resize_desc d = desc[blockIdx.y];
    if (!pil_resize_ok(d, g)) return;
    const bool hp = d.in_w != d.out_w, vp = d.in_h != d.out_h;
    if (hp && !vp) return;                                               // the horizontal pass wrote the result
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)d.out_h * d.out_w) return;
    const uint8_t* from = hp ? tmp + d.tmp_offset : src + d.src_offset;  // [in_h][out_w][C]
    uint8_t* out = dst + d.dst_offset + p * C;
    uint8_t o[C];
    if (!vp) {                                                           // the size itself: a copy
        for (int c = 0; c < C; ++c) o[c] = from[p * C + c];
    } else {
        const int32_t y = (int32_t)(p / d.out_w), x = (int32_t)(p - (int64_t)y * d.out_w);
        const PilRecord t = pil_record(tables + d.v_table, d.out_h, y, d.v_ksize, 0, d.in_h);
        if (t.ok) {
            pil_walk<C>(t.w, t.n, from + ((int64_t)t.first * d.out_w + x) * C, (int64_t)d.out_w * C, o);
        } else {
            for (int c = 0; c < C; ++c) o[c] = 0;
        }
    }
    for (int c = 0; c < C; ++c) out[c] = o[c];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// masks
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pil_mask_ok(const vrg_pil_mask_desc& d, int64_t n_spans, int64_t mask_bytes) {
    if (d.width < 1 || d.height < 1 || d.width > PIL_MAX_LINE || d.height > PIL_MAX_LINE || d.radius > (1 << 20)) return false;
    return span_fits(d.span_offset, d.height, n_spans) && span_fits(d.mask_offset, (int64_t)d.width * d.height, mask_bytes);
}

struct PilLineLds {
    uint32_t pre[PIL_MAX_LINE + 1];
    uint8_t line[2][PIL_MAX_LINE];
    uint32_t wave_total[4];
};

// three box passes over the n bytes of s.line[0], all 256 threads; the result is in s.line[1] (3 is odd); ends synchronised
__device__ __forceinline__ void pil_blur_line(PilLineLds& s, int32_t n, const PilBox& b) {
    const int32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t per = (n + 255) / 256, i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
    for (int pass = 0; pass < 3; ++pass) {
        const uint8_t* in = s.line[pass & 1];
        uint8_t* out = s.line[(pass & 1) ^ 1];
        uint32_t own = 0;
        for (int32_t i = i0; i < i1; ++i) own += in[i];
        uint32_t scan = own;                                             // inclusive over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)scan, off, 64);
            if (lane >= off) scan += v;
        }
        if (lane == 63) s.wave_total[wave] = scan;
        __syncthreads();
        uint32_t run = scan - own;
        for (int w = 0; w < wave; ++w) run += s.wave_total[w];
        if (t == 0) s.pre[0] = 0u;
        for (int32_t i = i0; i < i1; ++i) {
            run += in[i];
            s.pre[i + 1] = run;
        }
        __syncthreads();
        for (int32_t x = t; x < n; x += 256)
            out[x] = pil_box_pixel(x, n, b, [&](int32_t i) { return s.pre[i]; }, [&](int32_t i) { return in[i]; });
        __syncthreads();
    }
}

// rows: the spans, blurred along x into `scratch`; radius < 0: the 0 / 255 spans straight into `masks`
__global__ __launch_bounds__(256) void k_pil_mask_h(const PilSpan* __restrict__ spans, int64_t n_spans, const vrg_pil_mask_desc* __restrict__ desc,
                                                     uint8_t* __restrict__ scratch, uint8_t* __restrict__ masks, int64_t mask_bytes) {
    __shared__ PilLineLds s;
    const vrg_pil_mask_desc d = desc[blockIdx.y];
    if (!pil_mask_ok(d, n_spans, mask_bytes) || (int32_t)blockIdx.x >= d.height) return;     // uniform
    const int32_t y = (int32_t)blockIdx.x, n = d.width;
    const PilSpan sp = spans[d.span_offset + y];
    uint8_t* row = (d.radius < 0 ? masks : scratch) + d.mask_offset + (int64_t)y * n;
    if (d.radius < 0) {
        for (int32_t x = threadIdx.x; x < n; x += 256) row[x] = (x >= sp.x0 && x <= sp.x1) ? 255 : 0;
        return;
    }
    for (int32_t x = threadIdx.x; x < n; x += 256) s.line[0][x] = (x >= sp.x0 && x <= sp.x1) ? 255 : 0;
    __syncthreads();
    const PilBox b{d.radius, d.ww, d.fw};
    pil_blur_line(s, n, b);
    for (int32_t x = threadIdx.x; x < n; x += 256) row[x] = s.line[1][x];
}

// columns: `plane` blurred along y into `masks`
__global__ __launch_bounds__(256) void k_pil_mask_v(int64_t n_spans, const vrg_pil_mask_desc* __restrict__ desc, const uint8_t* __restrict__ plane,
                                                     uint8_t* __restrict__ masks, int64_t mask_bytes) {
    __shared__ PilLineLds s;
    const vrg_pil_mask_desc d = desc[blockIdx.y];
    if (!pil_mask_ok(d, n_spans, mask_bytes) || d.radius < 0 || (int32_t)blockIdx.x >= d.width) return;
    const int32_t x = (int32_t)blockIdx.x, n = d.height;
    const uint8_t* col = plane + d.mask_offset + x;
    for (int32_t y = threadIdx.x; y < n; y += 256) s.line[0][y] = col[(int64_t)y * d.width];
    __syncthreads();
    const PilBox b{d.radius, d.ww, d.fw};
    pil_blur_line(s, n, b);
    uint8_t* to = masks + d.mask_offset + x;
    for (int32_t y = threadIdx.x; y < n; y += 256) to[(int64_t)y * d.width] = s.line[1][y];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// means and paste
// ---------------------------------------------------------------------------------------------------------------------------------
struct PilGeom {
    int64_t frames, rep_bytes, mask_bytes;
    int32_t H, W;
};

__device__ __forceinline__ bool pil_box_ok(const vrg_pil_box_desc& d, const PilGeom& g) {
    if (d.left < 0 || d.top < 0 || d.box_w < 1 || d.box_h < 1) return false;
    if ((int64_t)d.left + d.box_w > g.W || (int64_t)d.top + d.box_h > g.H) return false;
    const int64_t px = (int64_t)d.box_w * d.box_h;
    return span_fits(d.mask_offset, px, g.mask_bytes) && span_fits(d.rep_offset, px * 3, g.rep_bytes);
}

__global__ __launch_bounds__(256) void k_np_means(const uint8_t* __restrict__ originals, const uint8_t* __restrict__ repaired,
                                                   const uint8_t* __restrict__ masks, const vrg_pil_box_desc* __restrict__ desc,
                                                   uint32_t* __restrict__ stats, PilGeom g, float strength) {
    const int64_t f = blockIdx.x;
    const vrg_pil_box_desc d = desc[f];                                  // uniform
    uint32_t* rec = stats + f * PIL_STATS_WORDS;
    if (!pil_box_ok(d, g) || !d.color_match) {
        if (threadIdx.x < PIL_STATS_WORDS) rec[threadIdx.x] = 0u;
        return;
    }
    const PilFrameOrig orig{originals + ((f * g.H + d.top) * (int64_t)g.W + d.left) * 3, d.box_w, g.W};
    np_means_block(orig, repaired + d.rep_offset, masks + d.mask_offset, (int64_t)d.box_w * d.box_h, strength, rec);
}

// the paste as a policy of move_bytes: the repaired bytes, shifted where the box asked for the colour match, pasted under the byte mask
struct PilMover {
    typedef MoverFrame<vrg_pil_box_desc> Frame;
    const uint8_t* __restrict__ repaired;
    const uint8_t* __restrict__ masks;
    const vrg_pil_box_desc* __restrict__ desc;
    const uint32_t* __restrict__ stats;
    PilGeom g;

    __device__ __forceinline__ void load(Frame& fr, int64_t f) const {
        fr.d = desc[f];
        fr.ok = pil_box_ok(fr.d, g);
        fr.matched = false;
        fr.shift[0] = fr.shift[1] = fr.shift[2] = 0.0f;
    }
    __device__ __forceinline__ void load_stats(Frame& fr, int64_t f) const {
        if (fr.d.color_match) fr.matched = pil_read_shift(stats + f * PIL_STATS_WORDS, fr.shift);
    }
    __device__ __forceinline__ ByteBox box(const Frame& fr) const { return ByteBox{fr.d.left, fr.d.top, fr.d.box_w, fr.d.box_h, g.W}; }
    __device__ __forceinline__ uint8_t byte(const Frame& fr, int32_t r, uint8_t v) const {
        int64_t i;
        int32_t c;
        if (!byte_in_box(box(fr), r, i, c)) return v;
        return pil_face_byte(v, repaired[fr.d.rep_offset + i * 3 + c], fr.matched, fr.shift[c], masks[fr.d.mask_offset + i]);
    }
};

__global__ __launch_bounds__(256) void k_pil_paste(const uint8_t* __restrict__ originals, const uint8_t* __restrict__ repaired,
                                                    const uint8_t* __restrict__ masks, const vrg_pil_box_desc* __restrict__ desc,
                                                    const uint32_t* __restrict__ stats, uint8_t* __restrict__ out, PilGeom g,
                                                    int64_t frame_bytes, int64_t total, int32_t aligned) {
    move_bytes(PilMover{repaired, masks, desc, stats, g}, originals, out, frame_bytes, total, aligned);
}

}  // namespace vrg

using namespace vrg;

extern "C" {

// the whole axis: the one builder over (0, n_in), which no float passes through
int32_t vrg_pil_lanczos_ksize(int32_t n_in, int32_t n_out) {
    return (n_in < 1 || n_out < 1) ? 0 : pil_lanczos_ksize(n_in, n_out);
}

int vrg_pil_lanczos_table(int32_t n_in, int32_t n_out, int32_t* bounds_host, int32_t* weights_host) {
    if (!bounds_host || !weights_host || n_in < 1 || n_out < 1) return VRG_ERR_BAD_ARG;
    pil_lanczos_table(n_in, n_out, bounds_host, weights_host);
    return VRG_OK;
}

// a box, as Pillow's C takes it
int32_t vrg_pil_filter_ksize(int32_t filter, float in0, float in1, int32_t n_out) {
    if (!pil_filter_known(filter) || n_out < 1 || !(in0 >= 0.0f) || !(in1 >= in0) || !(in1 <= 2147483520.0f)) return 0;
    const double k = ceil(pil_filter_support(filter) * fmax(pil_box_span(in0, in1) / n_out, 1.0)) * 2 + 1;
    return k > 2147483647.0 ? 0 : (int32_t)k;
}

int vrg_pil_filter_table(int32_t filter, int32_t n_in, float in0, float in1, int32_t n_out, int32_t* bounds_host, int32_t* weights_host) {
    if (!bounds_host || !weights_host || !pil_filter_known(filter) || n_in < 1 || n_out < 1 || !(in0 >= 0.0f) || !(in1 >= in0) ||
        !(in1 <= (float)n_in) || vrg_pil_filter_ksize(filter, in0, in1, n_out) < 1)
        return VRG_ERR_BAD_ARG;
    pil_filter_table(filter, n_in, in0, pil_box_span(in0, in1), n_out, bounds_host, weights_host);
    return VRG_OK;
}

int vrg_pil_box_parameters(float sigma, int32_t* out_host) {
    if (!out_host || !(sigma > 0.0f) || !(sigma <= 4096.0f)) return VRG_ERR_BAD_ARG;
    const PilBox b = pil_box_parameters(sigma);
    out_host[0] = b.r;
    out_host[1] = (int32_t)b.ww;
    out_host[2] = (int32_t)b.fw;
    return VRG_OK;
}

int vrg_pil_resize_u8(const uint8_t* src, int64_t src_bytes, const vrg_pil_resize_desc* desc, int64_t n_out, int32_t channels,
                      const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes, uint8_t* dst, int64_t dst_bytes,
                      int64_t max_pixels, void* stream) {
    if ((channels != 1 && channels != 3) || n_out < 0 || src_bytes < 0 || table_ints < 0 || tmp_bytes < 0 || dst_bytes < 0 || max_pixels < 0)
        return VRG_ERR_BAD_ARG;
    if (n_out == 0 || max_pixels == 0) return VRG_OK;
    if (!src || !desc || !dst || dst == src || (table_ints > 0 && !tables) || (tmp_bytes > 0 && (!tmp || tmp == src || tmp == dst)))
        return VRG_ERR_BAD_ARG;
    if (max_pixels > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const uint32_t parts = (uint32_t)((max_pixels + 255) / 256);
    const PilResizeGeom g{src_bytes, table_ints, tmp_bytes, dst_bytes, channels};
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(n_out, [&](int64_t i0, int64_t count) {
        const uint32_t ni = (uint32_t)count;
        if (channels == 3) {
            hipLaunchKernelGGL(k_pil_resize_h<3>, dim3(parts, ni), dim3(256), 0, st, src, desc + i0, tables, tmp, dst, g);
            VRG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_pil_resize_v<3>, dim3(parts, ni), dim3(256), 0, st, src, desc + i0, tables, (const uint8_t*)tmp, dst, g);
        } else {
            hipLaunchKernelGGL(k_pil_resize_h<1>, dim3(parts, ni), dim3(256), 0, st, src, desc + i0, tables, tmp, dst, g);
            VRG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_pil_resize_v<1>, dim3(parts, ni), dim3(256), 0, st, src, desc + i0, tables, (const uint8_t*)tmp, dst, g);
        }
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

int vrg_pil_mask_u8(const int32_t* spans, int64_t n_spans, const vrg_pil_mask_desc* desc, int64_t n_masks, int32_t max_width,
                    int32_t max_height, uint8_t* scratch, uint8_t* masks, int64_t mask_bytes, void* stream) {
    if (n_masks < 0 || n_spans < 0 || mask_bytes < 0 || max_width < 0 || max_height < 0) return VRG_ERR_BAD_ARG;
    if (n_masks == 0 || max_width == 0 || max_height == 0) return VRG_OK;
    if (!spans || !desc || !masks || !scratch || scratch == masks) return VRG_ERR_BAD_ARG;
    if (max_width > PIL_MAX_LINE || max_height > PIL_MAX_LINE) return VRG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(n_masks, [&](int64_t m0, int64_t count) {
        const uint32_t nm = (uint32_t)count;
        // a record without a blur (radius < 0) writes its spans to `masks` in the first launch and sits out the second
        hipLaunchKernelGGL(k_pil_mask_h, dim3((uint32_t)max_height, nm), dim3(256), 0, st, reinterpret_cast<const PilSpan*>(spans), n_spans,
                           desc + m0, scratch, masks, mask_bytes);
        VRG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_pil_mask_v, dim3((uint32_t)max_width, nm), dim3(256), 0, st, n_spans, desc + m0, (const uint8_t*)scratch, masks,
                           mask_bytes);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

int vrg_np_masked_means_f32(const uint8_t* originals, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks, int64_t mask_bytes,
                            const vrg_pil_box_desc* desc, uint32_t* stats, int64_t frames, int32_t height, int32_t width, float strength,
                            void* stream) {
    if (frames < 0 || rep_bytes < 0 || mask_bytes < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!originals || !repaired || !masks || !desc || !stats || (reinterpret_cast<uintptr_t>(stats) & 3u) != 0 || height < 1 || width < 1)
        return VRG_ERR_BAD_ARG;
    if ((int64_t)height * width * 3 > 0x7fffffffll || frames > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const PilGeom g{frames, rep_bytes, mask_bytes, height, width};
    hipLaunchKernelGGL(k_np_means, dim3((uint32_t)frames), dim3(256), 0, (hipStream_t)stream, originals, repaired, masks, desc, stats, g, strength);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_pil_paste_u8(const uint8_t* originals, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks, int64_t mask_bytes,
                     const vrg_pil_box_desc* desc, const uint32_t* stats, uint8_t* out, int64_t frames, int32_t height, int32_t width,
                     void* stream) {
    if (frames < 0 || rep_bytes < 0 || mask_bytes < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!originals || !repaired || !masks || !desc || !stats || (reinterpret_cast<uintptr_t>(stats) & 3u) != 0 || !out || out == originals ||
        out == repaired || height < 1 || width < 1)
        return VRG_ERR_BAD_ARG;
    ByteMoverLaunch l;
    const int rc = byte_mover_launch(originals, out, frames, height, width, l);
    if (rc != VRG_OK) return rc;
    const PilGeom g{frames, rep_bytes, mask_bytes, height, width};
    hipLaunchKernelGGL(k_pil_paste, dim3(l.blocks), dim3(256), 0, (hipStream_t)stream, originals, repaired, masks, desc, stats, out, g,
                       l.frame_bytes, l.total, l.aligned);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
