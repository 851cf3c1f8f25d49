// vrg_facefix.hip -- the pixels of the AI Video Builder's Face Fix (reference VRGDG_FaceFix.py: prepare_face_fix :473-476,
// finalize_face_fix :937-957) on decoded B,G,R bytes.  gfx950 only.  Arithmetic: csrc/vrg_facefix_math.hpp, csrc/vrg_lanczos_math.hpp; the
// body of a pixel, a byte, a record check and a workgroup's sums is csrc/vrg_facefix_body.hpp, shared with csrc/vrg_facefix_packed.hip.
//
// Shape of the work.  A job is a batch of byte frames and one square box per frame, a few per cent of a 4K frame up to all of its height.
//   k_lanczos4_boxes     prepare: one launch, blockIdx.y = the output frame, so its record (source frame, box, where its Lanczos records
//                        start) is wave-uniform; one thread = one output pixel straight from the definition (lz_pixel: 64 byte taps per
//                        channel out of L1 / L2, clamped to the BOX).  The box sizes differ per frame, so the tiles of k_lanczos4_tile
//                        (one geometry per launch) do not apply.
//   k_ff_mask_h / _v     the soft-ellipse masks, one per distinct (w, h) of the batch: the 0 / 1 spans blurred through a scratch plane.
//                        The horizontal pass adds the coefficients of the taps inside the row's span; the vertical pass reads the plane
//                        column-wise (consecutive lanes, consecutive floats).
//   k_ff_resize_stats    finalize, first half: the repaired frame resized to its box (lz_pixel again) into a packed byte scratch, and in
//                        the same launch the selected count and six byte sums of the frame: lane values -> wave butterfly -> LDS -> one
//                        64-bit integer atomic per sum and workgroup (integer addition: the same bits in any order).
//   k_ff_finish          the means and shifts of every record, on the device: the host never waits.  Both routes launch it (ff_stats_end).
//   k_ff_composite       finalize, second half: ONE pass over the output batch as a flat run of bytes, 16 per thread.  A piece that
//                        misses the box (nearly all of a frame) is one 16-byte non-temporal load and store; a piece that touches it is
//                        rebuilt byte by byte in registers; pieces that cross a frame boundary or are not 16-byte aligned go byte by byte
//                        (move_bytes of csrc/vrg_byte_mover.hpp, shared with the far-face paste).
#include "vrg_byte_mover.hpp"
#include "vrg_facefix_body.hpp"

namespace vrg {

struct FfGeom {
    int64_t frames, enhanced_frames, mask_floats, n_taps, capacity;
    int32_t H, W, enh_h, enh_w;
};

__device__ __forceinline__ bool ff_box_ok(const vrg_ff_box_desc& d, int64_t in_frames, int32_t H, int32_t W, int64_t n_taps, int32_t out_h,
                                          int32_t out_w) {
    if (d.frame < 0 || d.frame >= in_frames || d.left < 0 || d.top < 0 || d.box_w < 1 || d.box_h < 1) return false;
    if ((int64_t)d.left + d.box_w > W || (int64_t)d.top + d.box_h > H) return false;
    return span_fits(d.taps_offset, (int64_t)out_w + out_h, n_taps);
}

// the record of the composite: the box inside the frame, and ff_blend_ok
__device__ __forceinline__ bool ff_desc_ok(const vrg_ff_desc& d, const FfGeom& g, bool resized) {
    if (d.left < 0 || d.top < 0 || d.box_w < 1 || d.box_h < 1) return false;
    if ((int64_t)d.left + d.box_w > g.W || (int64_t)d.top + d.box_h > g.H) return false;
    return ff_blend_ok(d, g, (int64_t)d.box_w * d.box_h, resized);
}

__global__ __launch_bounds__(256) void k_lanczos4_boxes(const uint8_t* __restrict__ in, int64_t in_frames, int32_t H, int32_t W,
                                                         uint8_t* __restrict__ out, const vrg_ff_box_desc* __restrict__ desc, int32_t out_h,
                                                         int32_t out_w, const LzTap* __restrict__ taps, int64_t n_taps) {
    const int32_t n = out_h * out_w;
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n) return;
    const vrg_ff_box_desc d = desc[blockIdx.y];                          // wave-uniform
    uint8_t* dst = out + ((int64_t)blockIdx.y * n + p) * 3;
    uint8_t o[3] = {0, 0, 0};
    if (ff_box_ok(d, in_frames, H, W, n_taps, out_h, out_w)) {
        const int32_t y = p / out_w, x = p - y * out_w;
        ff_crop_pixel(in + (((int64_t)d.frame * H + d.top) * W + d.left) * 3, W, d.box_w, d.box_h, taps[d.taps_offset + x],
                      taps[d.taps_offset + out_w + y], o);
    }
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

__device__ __forceinline__ bool ff_mask_ok(const vrg_ff_mask_desc& d, int64_t n_spans, int64_t mask_floats) {
    if (d.width < 1 || d.height < 1) return false;
    return span_fits(d.span_offset, d.height, n_spans) && span_fits(d.mask_offset, (int64_t)d.width * d.height, mask_floats);
}

// n == 0: the 0 / 1 spans go straight to `plane` (the masks); otherwise the horizontal plane (the scratch)
__global__ __launch_bounds__(256) void k_ff_mask_h(const FfSpan* __restrict__ spans, int64_t n_spans, const float* __restrict__ coeffs, int32_t n,
                                                    const vrg_ff_mask_desc* __restrict__ desc, float* __restrict__ plane, int64_t mask_floats) {
    const vrg_ff_mask_desc d = desc[blockIdx.y];
    if (!ff_mask_ok(d, n_spans, mask_floats)) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)d.width * d.height) return;
    const int32_t y = (int32_t)(p / d.width), x = (int32_t)(p - (int64_t)y * d.width);
    const FfSpan s = spans[d.span_offset + y];
    plane[d.mask_offset + p] = n == 0 ? ((x >= s.x0 && x <= s.x1) ? 1.0f : 0.0f) : ff_blur_h(coeffs, n, s, d.width, x);
}

__global__ __launch_bounds__(256) void k_ff_mask_v(int64_t n_spans, const float* __restrict__ coeffs, int32_t n,
                                                    const vrg_ff_mask_desc* __restrict__ desc, const float* __restrict__ plane,
                                                    float* __restrict__ masks, int64_t mask_floats) {
    const vrg_ff_mask_desc d = desc[blockIdx.y];
    if (!ff_mask_ok(d, n_spans, mask_floats)) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)d.width * d.height) return;
    const int32_t y = (int32_t)(p / d.width), x = (int32_t)(p - (int64_t)y * d.width);
    const float* col = plane + d.mask_offset + x;
    masks[d.mask_offset + p] = ff_blur_v(coeffs, n, d.height, y, [&](int32_t row) { return col[(int64_t)row * d.width]; });
}

__global__ __launch_bounds__(256) void k_ff_resize_stats(const uint8_t* __restrict__ originals, const uint8_t* __restrict__ enhanced,
                                                          const float* __restrict__ masks, const vrg_ff_desc* __restrict__ desc,
                                                          const LzTap* __restrict__ taps, uint8_t* __restrict__ bytes,
                                                          unsigned long long* __restrict__ stats, FfGeom g, int64_t f0, int32_t measure) {
    const int64_t f = f0 + blockIdx.y;
    const vrg_ff_desc d = desc[f];                                       // wave-uniform
    if (!ff_desc_ok(d, g, true)) return;                                 // the whole workgroup leaves
    const int64_t n = (int64_t)d.box_w * d.box_h;
    if ((int64_t)blockIdx.x * 256 >= n) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t acc[FF_STAT_SUMS] = {};
    if (p < n) {
        const int32_t dy = (int32_t)(p / d.box_w), dx = (int32_t)(p - (int64_t)dy * d.box_w);
        ff_resize_pixel(enhanced + (int64_t)d.enhanced_index * g.enh_h * g.enh_w * 3, g.enh_h, g.enh_w, taps[d.taps_offset + dx],
                        taps[d.taps_offset + d.box_w + dy], bytes + d.bytes_offset + p * 3, masks + d.mask_offset + p,
                        originals + ((f * g.H + d.top + dy) * (int64_t)g.W + d.left + dx) * 3, measure, acc);
    }
    if (measure) ff_block_stats(acc, stats + f * FF_STATS_WORDS);       // uniform
}

__global__ __launch_bounds__(256) void k_ff_finish(unsigned long long* __restrict__ stats, int64_t frames, float color_match) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    ff_finish_record(stats + f * FF_STATS_WORDS, color_match);
}

// the composite as a policy of move_bytes: the face bytes of the resize scratch, shifted, blended under the float mask and the strength
struct FfMover {
    typedef MoverFrame<vrg_ff_desc> Frame;
    const float* __restrict__ masks;
    const vrg_ff_desc* __restrict__ desc;
    const uint8_t* __restrict__ bytes;
    const unsigned long long* __restrict__ stats;
    FfGeom g;

    __device__ __forceinline__ void load(Frame& fr, int64_t f) const {
        fr.d = desc[f];
        fr.ok = ff_desc_ok(fr.d, g, false);
        fr.matched = false;
        fr.shift[0] = fr.shift[1] = fr.shift[2] = 0.0f;
    }
    __device__ __forceinline__ void load_stats(Frame& fr, int64_t f) const {
        fr.matched = ff_read_record(stats + f * FF_STATS_WORDS, fr.shift);
    }
    __device__ __forceinline__ ByteBox box(const Frame& fr) const { return ByteBox{fr.d.left, fr.d.top, fr.d.box_w, fr.d.box_h, g.W}; }
    __device__ __forceinline__ uint8_t byte(const Frame& fr, int32_t r, uint8_t v) const {
        int64_t i;
        int32_t c;
        if (!byte_in_box(box(fr), r, i, c)) return v;
        return ff_composite_byte(v, bytes[fr.d.bytes_offset + i * 3 + c], fr.matched, fr.shift[c], masks[fr.d.mask_offset + i], fr.d.strength);
    }
};

__global__ __launch_bounds__(256) void k_ff_composite(const uint8_t* __restrict__ originals, const float* __restrict__ masks,
                                                       const vrg_ff_desc* __restrict__ desc, const uint8_t* __restrict__ bytes,
                                                       const unsigned long long* __restrict__ stats, uint8_t* __restrict__ out, FfGeom g,
                                                       int64_t frame_bytes, int64_t total, int32_t aligned) {
    move_bytes(FfMover{masks, desc, bytes, stats, g}, originals, out, frame_bytes, total, aligned);
}

int ff_stats_begin(void* stats, int64_t n, void* stream) {
    return hipMemsetAsync(stats, 0, (size_t)n * FF_STATS_WORDS * sizeof(uint64_t), (hipStream_t)stream) == hipSuccess ? VRG_OK : VRG_ERR_LAUNCH;
}

int ff_stats_end(void* stats, int64_t n, float color_match, void* stream) {
    if (!(color_match > 0.0f)) return VRG_OK;
    hipLaunchKernelGGL(k_ff_finish, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)stats, n, color_match);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_ff_ellipse_spans(int32_t width, int32_t height, int32_t* spans_host) {
    if (!spans_host || width < 1 || height < 1) return VRG_ERR_BAD_ARG;
    ff_ellipse_spans(width, height, reinterpret_cast<FfSpan*>(spans_host));
    return VRG_OK;
}

int vrg_ff_gauss_coeffs(int32_t feather, float* coeffs_host) {
    if (!coeffs_host || feather < 0 || feather > 256) return VRG_ERR_BAD_ARG;
    ff_gauss_coeffs(feather, coeffs_host);
    return VRG_OK;
}

int vrg_lanczos4_boxes_u8(const uint8_t* in, int64_t in_frames, int32_t height, int32_t width, uint8_t* out, const vrg_ff_box_desc* desc,
                          int64_t n_out, int32_t out_h, int32_t out_w, const void* taps, int64_t n_taps, void* stream) {
    if (!in || !out || in == out || !desc || !taps || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || in_frames < 0 || n_out < 0 || n_taps < 0 ||
        height < 1 || width < 1 || out_h < 1 || out_w < 1)
        return VRG_ERR_BAD_ARG;
    if (n_out == 0) return VRG_OK;
    if ((int64_t)out_h * out_w * 3 > 0x7fffffffll || (int64_t)height * width * 3 > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const uint32_t parts = (uint32_t)(((int64_t)out_h * out_w + 255) / 256);
    const int64_t out_fe = (int64_t)out_h * out_w * 3;
    return launch_chunks(n_out, [&](int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(k_lanczos4_boxes, dim3(parts, (uint32_t)nf), dim3(256), 0, (hipStream_t)stream, in, in_frames, height, width,
                           out + f0 * out_fe, desc + f0, out_h, out_w, reinterpret_cast<const LzTap*>(taps), n_taps);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

int vrg_ff_masks_f32(const int32_t* spans, int64_t n_spans, const float* coeffs, int32_t n_coeffs, const vrg_ff_mask_desc* desc,
                     int64_t n_masks, int64_t max_mask_pixels, float* scratch, float* masks, int64_t mask_floats, void* stream) {
    if (n_masks < 0 || n_spans < 0 || max_mask_pixels < 0 || mask_floats < 0 || n_coeffs < 0 || n_coeffs > 4 * 256 + 1) return VRG_ERR_BAD_ARG;
    if (n_masks == 0) return VRG_OK;
    if (!spans || !desc || !masks || (n_coeffs > 0 && (!coeffs || !scratch || scratch == masks || (n_coeffs & 1) == 0))) return VRG_ERR_BAD_ARG;
    if (max_mask_pixels > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    if (max_mask_pixels == 0) return VRG_OK;
    const uint32_t parts = (uint32_t)((max_mask_pixels + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(n_masks, [&](int64_t m0, int64_t nm) {
        hipLaunchKernelGGL(k_ff_mask_h, dim3(parts, (uint32_t)nm), dim3(256), 0, st, reinterpret_cast<const FfSpan*>(spans), n_spans, coeffs,
                           n_coeffs, desc + m0, n_coeffs ? scratch : masks, mask_floats);
        VRG_CHECK_LAUNCH();
        if (n_coeffs) {
            hipLaunchKernelGGL(k_ff_mask_v, dim3(parts, (uint32_t)nm), dim3(256), 0, st, n_spans, coeffs, n_coeffs, desc + m0,
                               (const float*)scratch, masks, mask_floats);
            VRG_CHECK_LAUNCH();
        }
        return VRG_OK;
    });
}

int vrg_ff_resize_stats_u8(const uint8_t* originals, const uint8_t* enhanced, const float* masks, int64_t mask_floats,
                           const vrg_ff_desc* desc, const void* taps, int64_t n_taps, uint8_t* bytes, int64_t capacity, void* stats,
                           int64_t frames, int64_t enhanced_frames, int32_t height, int32_t width, int32_t enh_h, int32_t enh_w,
                           int64_t max_box_pixels, float color_match, void* stream) {
    if (frames < 0 || enhanced_frames < 0 || mask_floats < 0 || n_taps < 0 || capacity < 0 || max_box_pixels < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!originals || !enhanced || !masks || !desc || !taps || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || !bytes || !stats ||
        (reinterpret_cast<uintptr_t>(stats) & 7u) != 0 || bytes == originals || bytes == enhanced || height < 1 || width < 1 || enh_h < 1 || enh_w < 1)
        return VRG_ERR_BAD_ARG;
    if ((int64_t)height * width * 3 > 0x7fffffffll || (int64_t)enh_h * enh_w * 3 > 0x7fffffffll || max_box_pixels > 0x7fffffffll)
        return VRG_ERR_UNSUPPORTED;
    int rc = ff_stats_begin(stats, frames, stream);
    if (rc != VRG_OK) return rc;
    const FfGeom g{frames, enhanced_frames, mask_floats, n_taps, capacity, height, width, enh_h, enh_w};
    const int32_t measure = color_match > 0.0f ? 1 : 0;
    if (max_box_pixels > 0) {
        const uint32_t parts = (uint32_t)((max_box_pixels + 255) / 256);
        rc = launch_chunks(frames, [&](int64_t f0, int64_t nf) {
            hipLaunchKernelGGL(k_ff_resize_stats, dim3(parts, (uint32_t)nf), dim3(256), 0, (hipStream_t)stream, originals, enhanced, masks, desc,
                               reinterpret_cast<const LzTap*>(taps), bytes, (unsigned long long*)stats, g, f0, measure);
            VRG_CHECK_LAUNCH();
            return VRG_OK;
        });
        if (rc != VRG_OK) return rc;
    }
    return ff_stats_end(stats, frames, color_match, stream);
}

int vrg_ff_composite_u8(const uint8_t* originals, const float* masks, int64_t mask_floats, const vrg_ff_desc* desc, const uint8_t* bytes,
                        int64_t capacity, const void* stats, uint8_t* out, int64_t frames, int32_t height, int32_t width, void* stream) {
    if (frames < 0 || mask_floats < 0 || capacity < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!originals || !masks || !desc || !bytes || !stats || (reinterpret_cast<uintptr_t>(stats) & 7u) != 0 || !out || out == originals ||
        out == bytes || height < 1 || width < 1)
        return VRG_ERR_BAD_ARG;
    ByteMoverLaunch l;
    const int rc = byte_mover_launch(originals, out, frames, height, width, l);
    if (rc != VRG_OK) return rc;
    const FfGeom g{frames, 0, mask_floats, 0, capacity, height, width, 0, 0};
    hipLaunchKernelGGL(k_ff_composite, dim3(l.blocks), dim3(256), 0, (hipStream_t)stream, originals, masks, desc, bytes,
                       (const unsigned long long*)stats, out, g, l.frame_bytes, l.total, l.aligned);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
