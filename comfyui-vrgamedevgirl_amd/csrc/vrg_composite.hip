// vrg_composite.hip -- the feathered crop composite of Image Paste Back and the two Face Fix composite nodes: a crop / work frame is
// bicubic-resized into a box of the frame, blended in under an analytic alpha, optionally after a mean-shift colour match.
// Reference: VRGDG_ImagePasteBack.py:11-41, 224-260; VRGDG_StandaloneFaceFixNodes.py:827-849, 891-916; arithmetic: vrg_composite_math.hpp.
//
// Shape of the work.  The output is every pixel of every frame (24 or 32 B/px of frame traffic plus 4 B/px of mask); the box is a
// small part of it (a 1024^2 face box is one 4K pixel in eight), and the crop it is resampled from is smaller again and stays in L2.
//   k_composite_stats        the first masked reduction of this library: per measured frame, over the box pixels with
//                            alpha > threshold, the count and the fp64 sums of the resampled crop and of the original under it.
//                            One workgroup per CP_TILE box pixels; lane sums -> wave butterfly -> four waves through LDS -> one
//                            partial per workgroup, written with ordinary stores.  No atomics: every addition has a fixed place.
//   k_composite_stats_final  adds a frame's partials in index order, forms the fp32 means, the shifts and the `matched` decision
//                            (count >= 16) on the device: the host never waits for a frame.
//   k_composite_apply        one flat pass over the output batch, four consecutive pixels per thread: the batch is addressed as one
//                            run of pixels, so a thread's 12 or 16 floats of frame data and its 4 mask floats are 16-byte pieces
//                            whatever the frame size; non-temporal, read once and written once.  Outside the box that is a clamped
//                            copy; inside, alpha and the resampled crop are recomputed (not read back from a temporary).
// The landmark-aligned composite (VRGDG_StandaloneFaceFixNodes.py:1015-1054; arithmetic: vrg_warp_math.hpp) is the same apply pass with a
// side table of warp records: a frame whose record is set takes warped byte / 255 as its face (k_composite_apply<C, true>), 64 integer
// taps per box pixel against the 16 float taps of the bicubic face.  The bytes it warps come from k_face_bytes (resize + quantise, one
// launch for all listed frames); k_warp_affine is the warp alone.  The 128 KB phase table is read through L1 / L2 (a pixel reads the 128
// contiguous bytes of its phase as eight 16-byte pieces, one per tap row); it is not staged in LDS, where it would leave one workgroup per CU.
#include "vrg_common.hpp"
#include "vrg_composite_math.hpp"
#include "vrg_warp_math.hpp"

namespace vrg {

constexpr int CP_TILE = 4096;            // box pixels per workgroup of the measuring pass (16 per thread)

struct CompositeGeom {
    int64_t frames, n_orig, n_crop, n_mask;
    int32_t crop_h, crop_w, crop_c, H, W, C, mask_h, mask_w, mask_stride, nc;
    int32_t aligned;                     // originals, out and mask_out all start on 16 bytes: the apply pass may move 16-byte pieces
};

typedef float cv4 __attribute__((ext_vector_type(4)));

// A record is used only if everything it names exists: the tables are filled by the caller and read here through raw pointers.
__device__ __forceinline__ bool cp_desc_ok(const vrg_composite_desc& d, const CompositeGeom& g, bool has_mask) {
    if (d.rule < VRG_COMPOSITE_ELLIPSE || d.rule > VRG_COMPOSITE_OPAQUE) return false;
    if (d.original_index < 0 || d.original_index >= g.n_orig || d.crop_index < 0 || d.crop_index >= g.n_crop) return false;
    if ((d.flags & VRG_COMPOSITE_USER_MASK) && (!has_mask || d.mask_index < 0 || d.mask_index >= g.n_mask)) return false;
    if (d.left < 0 || d.top < 0 || d.box_w <= 0 || d.box_h <= 0 || d.paste_w <= 0 || d.paste_h <= 0) return false;
    if (d.paste_w > d.box_w || d.paste_h > d.box_h) return false;
    if ((int64_t)d.left + d.paste_w > g.W || (int64_t)d.top + d.paste_h > g.H) return false;
    return true;
}

// alpha and the resampled crop of box pixel (dx, dy)
__device__ __forceinline__ float cp_eval(const vrg_composite_desc& d, const CompositeGeom& g, const float* __restrict__ crops,
                                         const float* __restrict__ user_mask, int32_t dx, int32_t dy, bool want_crop, float v[4]) {
    const float* um = (d.flags & VRG_COMPOSITE_USER_MASK) ? user_mask + (int64_t)d.mask_index * g.mask_h * g.mask_w * g.mask_stride : nullptr;
    auto load_mask = [&](int32_t y, int32_t x) { return um[((int64_t)y * g.mask_w + x) * g.mask_stride]; };
    const float alpha = cp_alpha_masked(d, g.mask_h, g.mask_w, dx, dy, load_mask);
    if (want_crop) {
        const float* cf = crops + (int64_t)d.crop_index * g.crop_h * g.crop_w * g.crop_c;
        auto load = [&](int32_t y, int32_t x, int c) { return cf[(y * g.crop_w + x) * g.crop_c + c]; };
        cp_crop(d, g.crop_h, g.crop_w, g.nc, dx, dy, load, v);
    }
    return alpha;
}

__global__ __launch_bounds__(256) void k_composite_stats(const float* __restrict__ crops, const float* __restrict__ originals,
                                                         const float* __restrict__ user_mask, const vrg_composite_desc* __restrict__ desc,
                                                         const int32_t* __restrict__ match_frames, CompositeGeom g, int32_t parts,
                                                         double* __restrict__ scratch) {
    const int64_t m = blockIdx.y;
    const int32_t f = match_frames[m];
    double acc[CP_PART_DOUBLES];
#pragma unroll
    for (int i = 0; i < CP_PART_DOUBLES; ++i) acc[i] = 0.0;
    bool ok = f >= 0 && f < g.frames;
    vrg_composite_desc d;
    if (ok) {
        d = desc[f];
        ok = cp_desc_ok(d, g, user_mask != nullptr) && (d.flags & VRG_COMPOSITE_MATCH);
    }
    if (ok) {
        const int64_t n = (int64_t)d.paste_w * d.paste_h;                 // <= max_box_pixels < 2^31 (checked by the entry point's caller contract)
        const float* of = originals + (int64_t)d.original_index * g.H * g.W * g.C;
        for (int k = 0; k < CP_TILE / 256; ++k) {
            const int64_t p = (int64_t)blockIdx.x * CP_TILE + k * 256 + threadIdx.x;
            if (p < n) {
                const int32_t dy = (int32_t)((uint32_t)p / (uint32_t)d.paste_w), dx = (int32_t)p - dy * d.paste_w;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                const float alpha = cp_eval(d, g, crops, user_mask, dx, dy, true, v);
                if (cp_selected(d, alpha)) {
                    const float* t = of + ((int64_t)(d.top + dy) * g.W + d.left + dx) * g.C;
                    acc[0] += 1.0;
                    for (int c = 0; c < g.nc; ++c) {
                        acc[1 + c] += (double)v[c];
                        acc[5 + c] += (double)t[c];
                    }
                }
            }
        }
    }
    // every thread of the workgroup arrives here
    __shared__ double part[4][CP_PART_DOUBLES];
    block_sum_4waves(acc, part);
    if (threadIdx.x < CP_PART_DOUBLES) {
        const int t = threadIdx.x;
        scratch[(m * parts + blockIdx.x) * CP_PART_DOUBLES + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    }
}

__global__ __launch_bounds__(64) void k_composite_stats_final(const vrg_composite_desc* __restrict__ desc, const int32_t* __restrict__ match_frames,
                                                              CompositeGeom g, int32_t parts, const double* __restrict__ scratch,
                                                              uint32_t* __restrict__ stats) {
    const int64_t m = blockIdx.x;
    const int32_t f = match_frames[m];
    __shared__ double sums[CP_PART_DOUBLES];
    const int t = threadIdx.x;
    if (t < CP_PART_DOUBLES) {
        double a = 0.0;
        for (int32_t j = 0; j < parts; ++j) a += scratch[(m * parts + j) * CP_PART_DOUBLES + t];
        sums[t] = a;
    }
    __syncthreads();
    if (t == 0 && f >= 0 && f < g.frames) {
        const vrg_composite_desc d = desc[f];
        double s[CP_PART_DOUBLES];
        for (int i = 0; i < CP_PART_DOUBLES; ++i) s[i] = sums[i];
        uint32_t rec[CP_STATS_WORDS];
        cp_finalize(d, s, g.nc, rec);
        for (int i = 0; i < CP_STATS_WORDS; ++i) stats[(int64_t)f * CP_STATS_WORDS + i] = rec[i];
    }
}

// One output pixel: `in` = the original's C values, (x, y) its position in the frame.
// what the warping passes read besides the composite's own arguments
struct WarpSrc {
    const vrg_warp_desc* rec;            // one per output frame
    const uint8_t* bytes;                // the packed [h][w][3] images
    int64_t n_bytes;
    const int16_t* table;                // WP_PHASES x WP_KERNEL
};

// a record is used only if its image lies inside the byte buffer
__device__ __forceinline__ bool wp_rec_ok(const vrg_warp_desc& r, int64_t n_bytes) {
    if (!r.set || r.src_w < 1 || r.src_h < 1) return false;
    return span_fits(r.src_offset, (int64_t)r.src_w * r.src_h * 3, n_bytes);
}

// the warped byte pixel (x, y) of a record's image; the weights of the phase are read row by row, eight int16 = 16 bytes at a time
__device__ __forceinline__ void wp_eval(const vrg_warp_desc& r, const WarpSrc& ws, int32_t x, int32_t y, uint8_t o[3]) {
    int32_t sx, sy, phase;
    wp_source(r.m, x, y, sx, sy, phase);
    const uint8_t* img = ws.bytes + r.src_offset;
    const int32_t w = r.src_w;
    wp_pixel(ws.table + (int64_t)phase * WP_KERNEL, sx, sy, r.src_w, r.src_h,
             [&](int32_t yy, int32_t xx, int c) { return img[((int64_t)yy * w + xx) * 3 + c]; }, o);
}

template <int C, bool WARP>
__device__ __forceinline__ void cp_pixel(const vrg_composite_desc& d, bool ok, const CompositeGeom& g, const float* __restrict__ crops,
                                         const float* __restrict__ user_mask, const uint32_t* __restrict__ stats, int64_t f, int32_t x, int32_t y,
                                         const float in[C], float o[C], float& m, const vrg_warp_desc& wr, bool warped, const WarpSrc& ws) {
    const bool raw = d.rule == VRG_COMPOSITE_NONE && (d.flags & VRG_COMPOSITE_RAW_COPY);
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = raw ? in[c] : clamp01(in[c]);
    m = 0.0f;
    if (!ok) return;
    const int32_t dx = x - d.left, dy = y - d.top;
    if (dx < 0 || dx >= d.paste_w || dy < 0 || dy >= d.paste_h) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float alpha = cp_eval(d, g, crops, user_mask, dx, dy, !(WARP && warped), v);
    if (WARP && warped) {
        uint8_t b[3];
        wp_eval(wr, ws, dx, dy, b);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)b[c] / 255.0f;                 // astype(float32) / 255.0: the IEEE quotient
    }
    const uint32_t* rec = stats + f * CP_STATS_WORDS;
    const bool matched = (d.flags & VRG_COMPOSITE_MATCH) && rec[1] != 0u;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c < g.nc) o[c] = cp_blend(in[c], v[c], alpha, matched, matched ? f32_from_bits(rec[10 + c]) : 0.0f);
    }
    m = alpha;
}

template <int C, bool WARP>
__global__ __launch_bounds__(256) void k_composite_apply(const float* __restrict__ crops, const float* __restrict__ originals,
                                                         const float* __restrict__ user_mask, const vrg_composite_desc* __restrict__ desc,
                                                         const uint32_t* __restrict__ stats, float* __restrict__ out, float* __restrict__ mask_out,
                                                         CompositeGeom g, int64_t total_px, WarpSrc ws) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= total_px) return;
    const int32_t HW = g.H * g.W;
    const int64_t f0 = p0 / HW;
    const int32_t i0 = (int32_t)(p0 - f0 * HW);
    const bool has_mask = user_mask != nullptr;
    vrg_composite_desc d = desc[f0];
    bool ok = cp_desc_ok(d, g, has_mask);
    vrg_warp_desc wr = {};
    bool warped = false;
    if (WARP && ok) {
        wr = ws.rec[f0];
        warped = wp_rec_ok(wr, ws.n_bytes) && wr.src_w == d.box_w && wr.src_h == d.box_h;
    }
    const bool src_ok = d.original_index >= 0 && d.original_index < g.n_orig;
    if (g.aligned && p0 + 4 <= total_px && i0 + 3 < HW && src_ok && d.original_index == f0) {
        // the usual case: four pixels of one frame whose original is the frame of the same index -- 16-byte pieces in and out
        const cv4* src = reinterpret_cast<const cv4*>(originals + p0 * C);
        float in[4 * C], o[4 * C], mk[4];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const cv4 q = __builtin_nontemporal_load(src + j);
            in[4 * j] = q.x; in[4 * j + 1] = q.y; in[4 * j + 2] = q.z; in[4 * j + 3] = q.w;
        }
        int32_t y = (int32_t)((uint32_t)i0 / (uint32_t)g.W), x = i0 - y * g.W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cp_pixel<C, WARP>(d, ok, g, crops, user_mask, stats, f0, x, y, in + k * C, o + k * C, mk[k], wr, warped, ws);
            if (++x == g.W) { x = 0; ++y; }
        }
        cv4* dst = reinterpret_cast<cv4*>(out + p0 * C);
#pragma unroll
        for (int j = 0; j < C; ++j) __builtin_nontemporal_store(cv4{o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]}, dst + j);
        __builtin_nontemporal_store(cv4{mk[0], mk[1], mk[2], mk[3]}, reinterpret_cast<cv4*>(mask_out + p0));
        return;
    }
    // a group that crosses a frame boundary, ends the batch, or reads another frame's original (broadcast): pixel by pixel
    int64_t f = f0;
    int32_t i = i0;
    for (int k = 0; k < 4 && p0 + k < total_px; ++k) {
        if (i >= HW) {
            i = 0;
            ++f;
            d = desc[f];
            ok = cp_desc_ok(d, g, has_mask);
            warped = false;
            if (WARP && ok) {
                wr = ws.rec[f];
                warped = wp_rec_ok(wr, ws.n_bytes) && wr.src_w == d.box_w && wr.src_h == d.box_h;
            }
        }
        float in[C], o[C], mk;
        const bool have = d.original_index >= 0 && d.original_index < g.n_orig;
        const float* s = originals + ((int64_t)(have ? d.original_index : 0) * HW + i) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) in[c] = have ? __builtin_nontemporal_load(s + c) : 0.0f;
        const int32_t y = (int32_t)((uint32_t)i / (uint32_t)g.W), x = i - y * g.W;
        cp_pixel<C, WARP>(d, ok, g, crops, user_mask, stats, f, x, y, in, o, mk, wr, warped, ws);
        float* t = out + (p0 + k) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) __builtin_nontemporal_store(o[c], t + c);
        __builtin_nontemporal_store(mk, mask_out + p0 + k);
        ++i;
    }
}

// Steps 1-2 of the landmark-aligned node: the clamped bicubic face of every listed frame as bytes, and on request the original under the box.
__global__ __launch_bounds__(256) void k_face_bytes(const float* __restrict__ crops, const float* __restrict__ originals,
                                                    const vrg_composite_desc* __restrict__ desc, const int64_t* __restrict__ offsets,
                                                    uint8_t* __restrict__ generated, uint8_t* __restrict__ source, int64_t capacity,
                                                    CompositeGeom g, int64_t f0) {
    const int64_t f = f0 + blockIdx.y;
    const int64_t off = offsets[f];
    if (off < 0) return;
    const vrg_composite_desc d = desc[f];
    if (!cp_desc_ok(d, g, false) || d.paste_w != d.box_w || d.paste_h != d.box_h) return;
    const int64_t n = (int64_t)d.box_w * d.box_h;
    if (!span_fits(off, n * 3, capacity)) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int32_t dy = (int32_t)((uint32_t)p / (uint32_t)d.box_w), dx = (int32_t)p - dy * d.box_w;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* cf = crops + (int64_t)d.crop_index * g.crop_h * g.crop_w * g.crop_c;
    cp_crop(d, g.crop_h, g.crop_w, 3, dx, dy, [&](int32_t y, int32_t x, int c) { return cf[(y * g.crop_w + x) * g.crop_c + c]; }, v);
    uint8_t* o = generated + off + p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = wp_quantise(v[c]);
    if (source) {
        const float* t = originals + (((int64_t)d.original_index * g.H + d.top + dy) * g.W + d.left + dx) * g.C;
        uint8_t* s = source + off + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = wp_quantise(t[c]);
    }
}

// The warp alone: frame f0 + blockIdx.y, 256 result pixels per workgroup.
__global__ __launch_bounds__(256) void k_warp_affine(WarpSrc ws, uint8_t* __restrict__ out, int32_t out_h, int32_t out_w, int64_t f0) {
    const int64_t f = f0 + blockIdx.y;
    const int32_t n = out_h * out_w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const vrg_warp_desc r = ws.rec[f];
    uint8_t b[3] = {0, 0, 0};
    if (wp_rec_ok(r, ws.n_bytes)) {
        const int32_t y = (int32_t)((uint32_t)p / (uint32_t)out_w), x = (int32_t)p - y * out_w;
        wp_eval(r, ws, x, y, b);
    }
    uint8_t* o = out + (f * n + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = b[c];
}

static bool composite_geom_ok(const CompositeGeom& g, const float* user_mask) {
    if (g.frames < 0 || g.n_orig < 1 || g.n_crop < 1 || g.n_mask < 0) return false;
    if (g.crop_h <= 0 || g.crop_w <= 0 || g.crop_c < 3 || g.H <= 0 || g.W <= 0 || (g.C != 3 && g.C != 4)) return false;
    if ((g.nc != 3 && g.nc != 4) || g.nc > g.C || g.nc > g.crop_c) return false;
    if (user_mask && (g.n_mask < 1 || g.mask_h <= 0 || g.mask_w <= 0 || g.mask_stride < 1)) return false;
    return true;
}

// in-frame offsets are 32-bit; frames are addressed with 64 bits
static bool composite_geom_supported(const CompositeGeom& g, const float* user_mask) {
    if ((int64_t)g.H * g.W > 0x7fffffff / 4 || (int64_t)g.crop_h * g.crop_w * g.crop_c > 0x7fffffff) return false;
    if (user_mask && (int64_t)g.mask_h * g.mask_w * g.mask_stride > 0x7fffffff) return false;
    return true;
}

static int64_t composite_parts(int64_t max_box_pixels) {
    const int64_t parts = (max_box_pixels + CP_TILE - 1) / CP_TILE;
    return parts < 1 ? 1 : parts;
}

}  // namespace vrg

using namespace vrg;

extern "C" int64_t vrg_composite_scratch_bytes(int64_t frames, int64_t max_box_pixels) {
    if (frames < 0 || max_box_pixels < 0) return -1;
    return frames * composite_parts(max_box_pixels) * CP_PART_DOUBLES * (int64_t)sizeof(double);
}

extern "C" int vrg_composite_stats_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                                       const int32_t* match_frames, int64_t n_match, int64_t max_box_pixels,
                                       int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                                       int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                                       int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels,
                                       void* scratch, void* stats, void* stream) {
    const CompositeGeom g{frames, original_frames, crop_frames, mask_frames, crop_h, crop_w, crop_channels, height, width, channels,
                          mask_h, mask_w, mask_stride, match_channels, 0};
    if (n_match < 0 || max_box_pixels < 0 || n_match > frames) return VRG_ERR_BAD_ARG;
    if (n_match == 0) return VRG_OK;
    if (!crops || !originals || !desc || !match_frames || !scratch || !stats || !composite_geom_ok(g, user_mask)) return VRG_ERR_BAD_ARG;
    if (!composite_geom_supported(g, user_mask) || max_box_pixels > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    const int64_t parts = composite_parts(max_box_pixels);
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(n_match, [&](int64_t m0, int64_t nm) {
        double* sc = (double*)scratch + m0 * parts * CP_PART_DOUBLES;
        hipLaunchKernelGGL(k_composite_stats, dim3((uint32_t)parts, (uint32_t)nm), dim3(256), 0, st, crops, originals, user_mask, desc,
                           match_frames + m0, g, (int32_t)parts, sc);
        VRG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_composite_stats_final, dim3((uint32_t)nm), dim3(64), 0, st, desc, match_frames + m0, g, (int32_t)parts,
                           (const double*)sc, (uint32_t*)stats);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

// out and mask_out are both written, every other operand is read: no written operand may share a byte with another operand
static bool composite_operands_overlap(const CompositeGeom& g, const float* crops, const float* originals, const float* user_mask,
                                       const uint8_t* bytes, int64_t n_bytes, const float* out, const float* mask_out) {
    const int64_t px = (int64_t)g.H * g.W;
    const int64_t out_bytes = vrg_operand_bytes(g.frames, px * g.C * 4), mask_out_bytes = vrg_operand_bytes(g.frames, px * 4);
    const void* reads[4] = {crops, originals, user_mask, bytes};
    const int64_t read_bytes[4] = {vrg_operand_bytes(g.n_crop, (int64_t)g.crop_h * g.crop_w * g.crop_c * 4),
                                   vrg_operand_bytes(g.n_orig, px * g.C * 4),
                                   vrg_operand_bytes(g.n_mask, (int64_t)g.mask_h * g.mask_w * g.mask_stride * 4), n_bytes};
    if (vrg_ranges_overlap(out, out_bytes, mask_out, mask_out_bytes)) return true;
    for (int i = 0; i < 4; ++i)
        if (vrg_ranges_overlap(out, out_bytes, reads[i], read_bytes[i]) || vrg_ranges_overlap(mask_out, mask_out_bytes, reads[i], read_bytes[i]))
            return true;
    return false;
}

extern "C" int vrg_composite_apply_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                                       const void* stats, float* out, float* mask_out,
                                       int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                                       int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                                       int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels, void* stream) {
    const CompositeGeom g{frames, original_frames, crop_frames, mask_frames, crop_h, crop_w, crop_channels, height, width, channels,
                          mask_h, mask_w, mask_stride, match_channels,
                          ((((uintptr_t)originals | (uintptr_t)out | (uintptr_t)mask_out) & 15) == 0) ? 1 : 0};
    if (frames < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!crops || !originals || !desc || !stats || !out || !mask_out || out == originals || out == crops || !composite_geom_ok(g, user_mask))
        return VRG_ERR_BAD_ARG;
    if (composite_operands_overlap(g, crops, originals, user_mask, nullptr, 0, out, mask_out)) return VRG_ERR_BAD_ARG;
    if (!composite_geom_supported(g, user_mask)) return VRG_ERR_UNSUPPORTED;
    const int64_t total_px = frames * (int64_t)height * width;
    const int64_t blocks = ((total_px + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const WarpSrc none{nullptr, nullptr, 0, nullptr};
    if (channels == 3)
        hipLaunchKernelGGL((k_composite_apply<3, false>), dim3((uint32_t)blocks), dim3(256), 0, st, crops, originals, user_mask, desc,
                           (const uint32_t*)stats, out, mask_out, g, total_px, none);
    else
        hipLaunchKernelGGL((k_composite_apply<4, false>), dim3((uint32_t)blocks), dim3(256), 0, st, crops, originals, user_mask, desc,
                           (const uint32_t*)stats, out, mask_out, g, total_px, none);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

extern "C" int vrg_composite_warp_apply_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                                            const void* stats, const vrg_warp_desc* rec, const uint8_t* bytes, int64_t n_bytes, const void* table,
                                            float* out, float* mask_out,
                                            int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                                            int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                                            int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels, void* stream) {
    const CompositeGeom g{frames, original_frames, crop_frames, mask_frames, crop_h, crop_w, crop_channels, height, width, channels,
                          mask_h, mask_w, mask_stride, match_channels,
                          ((((uintptr_t)originals | (uintptr_t)out | (uintptr_t)mask_out) & 15) == 0) ? 1 : 0};
    if (frames < 0 || n_bytes < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!crops || !originals || !desc || !stats || !rec || !bytes || !table || !out || !mask_out || out == originals || out == crops ||
        ((uintptr_t)table & 15) || !composite_geom_ok(g, user_mask))
        return VRG_ERR_BAD_ARG;
    if (composite_operands_overlap(g, crops, originals, user_mask, bytes, n_bytes, out, mask_out)) return VRG_ERR_BAD_ARG;
    if (!composite_geom_supported(g, user_mask)) return VRG_ERR_UNSUPPORTED;
    const int64_t total_px = frames * (int64_t)height * width;
    const int64_t blocks = ((total_px + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const WarpSrc ws{rec, bytes, n_bytes, (const int16_t*)table};
    if (channels == 3)
        hipLaunchKernelGGL((k_composite_apply<3, true>), dim3((uint32_t)blocks), dim3(256), 0, st, crops, originals, user_mask, desc,
                           (const uint32_t*)stats, out, mask_out, g, total_px, ws);
    else
        hipLaunchKernelGGL((k_composite_apply<4, true>), dim3((uint32_t)blocks), dim3(256), 0, st, crops, originals, user_mask, desc,
                           (const uint32_t*)stats, out, mask_out, g, total_px, ws);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

extern "C" int vrg_warp_phase_table(void* table_host) {
    if (!table_host) return VRG_ERR_BAD_ARG;
    wp_phase_table(reinterpret_cast<int16_t*>(table_host));
    return VRG_OK;
}

extern "C" int vrg_warp_record(const float* transform, int32_t out_w, int32_t out_h, int32_t src_w, int32_t src_h, int64_t src_offset,
                               vrg_warp_desc* record_host) {
    if (!transform || !record_host) return VRG_ERR_BAD_ARG;
    return wp_record(transform, out_w, out_h, src_w, src_h, src_offset, record_host) ? VRG_OK : VRG_ERR_BAD_ARG;
}

extern "C" int vrg_face_bytes_u8(const float* crops, const float* originals, const vrg_composite_desc* desc, const int64_t* offsets,
                                 uint8_t* generated, uint8_t* source, int64_t capacity, int64_t max_box_pixels,
                                 int64_t frames, int64_t original_frames, int64_t crop_frames,
                                 int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                                 void* stream) {
    const CompositeGeom g{frames, original_frames, crop_frames, 0, crop_h, crop_w, crop_channels, height, width, channels, 0, 0, 0, 3, 0};
    if (frames < 0 || capacity < 0 || max_box_pixels < 0) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if (!crops || !desc || !offsets || !generated || (source && !originals) || source == generated || !composite_geom_ok(g, nullptr))
        return VRG_ERR_BAD_ARG;
    if (!composite_geom_supported(g, nullptr) || max_box_pixels > 0x7fffffff) return VRG_ERR_UNSUPPORTED;
    if (max_box_pixels == 0) return VRG_OK;
    const int64_t parts = (max_box_pixels + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    return launch_chunks(frames, [&](int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(k_face_bytes, dim3((uint32_t)parts, (uint32_t)nf), dim3(256), 0, st, crops, originals, desc, offsets, generated, source,
                           capacity, g, f0);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

extern "C" int vrg_warp_affine_u8(const uint8_t* in, int64_t in_bytes, uint8_t* out, const vrg_warp_desc* rec, const void* table, int64_t frames,
                                  int32_t out_h, int32_t out_w, void* stream) {
    if (frames < 0 || in_bytes < 0) return VRG_ERR_BAD_ARG;
    if (!in || !out || !rec || !table || in == out || ((uintptr_t)table & 15) || out_h < 1 || out_w < 1) return VRG_ERR_BAD_ARG;
    if (vrg_ranges_overlap(in, in_bytes, out, vrg_operand_bytes(frames, (int64_t)out_h * out_w * 3))) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    const int64_t px = (int64_t)out_h * out_w;
    if (px * 3 > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    const int64_t parts = (px + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    const WarpSrc ws{rec, in, in_bytes, (const int16_t*)table};
    return launch_chunks(frames, [&](int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(k_warp_affine, dim3((uint32_t)parts, (uint32_t)nf), dim3(256), 0, st, ws, out, out_h, out_w, f0);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}
