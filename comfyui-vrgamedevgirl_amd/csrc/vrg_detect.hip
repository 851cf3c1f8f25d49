// vrg_detect.hip -- what the face detector of the Face Fix Prepare nodes and of the Builder eats (`_detect_with_rotation` / `_detect`,
// VRGDG_StandaloneFaceFixNodes.py:95-185 and VRGDG_FaceFix.py:67-157 of the reference): the frame quantised to B,G,R bytes, rotated by the
// angles of `rotation_assist` (bilinear byte warpAffine, replicated border), cut into regions, each resized to 300 x 300 (bilinear byte
// resize) and turned into a mean-subtracted fp32 blob.  gfx950 only.  Arithmetic: csrc/vrg_detect_math.hpp.
//
// k_detect_blobs: one launch for every frame x angle x region of a call.  A thread owns one blob pixel and its three channel planes; x runs
//   fastest across the lanes, so a wave writes 64 consecutive floats of each plane.  Nothing between the source frame and the blob goes to
//   memory: a value without a transform reads the resize's 2 x 2 source pixels, one with a transform 16 -- each of the 2 x 2 taps is a
//   pixel of the rotated frame, itself a 2 x 2 warp sample clamped at the frame border.  Source bytes are quantised where they are read.
//   The coordinate arithmetic is IEEE double (v_mul_f64, v_add_f64, v_rndne_f64) per thread: 90,000 threads per blob, four roundings each.
// k_warp_linear: the rotated B,G,R byte frames themselves (the YuNet branch reads them whole).  A thread owns 16 consecutive pixels of the
//   flattened frame = 48 bytes = three 16-byte stores when the frame starts on a 16-byte boundary (bytewise otherwise and in the last,
//   partial group); the launch is bound by that write.
// A descriptor that names a frame, a transform or a region outside what the call states writes zeros (vrg_detect_check refuses it on the
// host before anything is uploaded).
#include "vrg_common.hpp"
#include "vrg_detect_math.hpp"

namespace vrg {

constexpr int DT_THREADS = 256;
constexpr int DT_BLOCKS_PER_BLOB = (DT_BLOB_PIXELS + DT_THREADS - 1) / DT_THREADS;      // 352
constexpr int DT_GROUP = 16;                                                            // pixels of one thread of k_warp_linear

typedef uint32_t dt_u4 __attribute__((ext_vector_type(4)));

// the three B,G,R bytes of source pixel (y, x) of one frame
template <bool F32>
struct DtSource {
    const void* base;        // the frame
    int32_t W, C;
    __device__ __forceinline__ void operator()(int32_t y, int32_t x, uint8_t b[3]) const {
        const int64_t at = ((int64_t)y * W + x) * C;
        if (F32) {
            const float* p = reinterpret_cast<const float*>(base) + at;
            b[0] = wp_quantise(p[2]);
            b[1] = wp_quantise(p[1]);
            b[2] = wp_quantise(p[0]);
        } else {
            const uint8_t* p = reinterpret_cast<const uint8_t*>(base) + at;
            b[0] = p[0];
            b[1] = p[1];
            b[2] = p[2];
        }
    }
};

template <bool F32>
__global__ __launch_bounds__(DT_THREADS) void k_detect_blobs(const void* __restrict__ frames, const double* __restrict__ transforms,
                                                            const vrg_detect_desc* __restrict__ desc, float* __restrict__ out, int64_t n_frames,
                                                            int64_t n_transforms, int32_t H, int32_t W, int32_t C) {
    const int64_t blob = (int64_t)(blockIdx.x / (uint32_t)DT_BLOCKS_PER_BLOB);
    const int p = (int)(blockIdx.x % (uint32_t)DT_BLOCKS_PER_BLOB) * DT_THREADS + (int)threadIdx.x;
    if (p >= DT_BLOB_PIXELS) return;
    const vrg_detect_desc d = desc[blob];
    float* o = out + blob * (int64_t)(3 * DT_BLOB_PIXELS) + p;
    if (!dt_desc_ok(d, n_frames, n_transforms, H, W)) {
        o[0] = 0.0f;
        o[DT_BLOB_PIXELS] = 0.0f;
        o[2 * DT_BLOB_PIXELS] = 0.0f;
        return;
    }
    const int64_t frame_elems = (int64_t)H * W * C;
    DtSource<F32> src;
    src.base = F32 ? (const void*)(reinterpret_cast<const float*>(frames) + (int64_t)d.frame * frame_elems)
                   : (const void*)(reinterpret_cast<const uint8_t*>(frames) + (int64_t)d.frame * frame_elems);
    src.W = W;
    src.C = C;
    const int dy = p / DT_BLOB, dx = p - dy * DT_BLOB;
    uint8_t b[3];
    if (d.transform < 0) {                                                       // uniform over the block
        dt_resize_pixel(dx, dy, d.right - d.left, d.bottom - d.top, DT_BLOB,
                        [&](int32_t y, int32_t x, uint8_t v[3]) { src(d.top + y, d.left + x, v); }, b);
    } else {
        double m[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = transforms[(int64_t)d.transform * 6 + i];
        dt_resize_pixel(dx, dy, d.right - d.left, d.bottom - d.top, DT_BLOB,
                        [&](int32_t y, int32_t x, uint8_t v[3]) { dt_warp_pixel(m, d.left + x, d.top + y, W, H, src, v); }, b);
    }
    o[0] = (float)b[0] - dt_mean(0);
    o[DT_BLOB_PIXELS] = (float)b[1] - dt_mean(1);
    o[2 * DT_BLOB_PIXELS] = (float)b[2] - dt_mean(2);
}

template <bool F32>
__global__ __launch_bounds__(DT_THREADS) void k_warp_linear(const void* __restrict__ frames, const double* __restrict__ transforms,
                                                           const vrg_detect_frame_desc* __restrict__ desc, uint8_t* __restrict__ out, int64_t n_frames,
                                                           int64_t n_transforms, int32_t H, int32_t W, int32_t C, uint32_t blocks_per_frame) {
    const int64_t n = (int64_t)(blockIdx.x / blocks_per_frame);
    const int64_t pixels = (int64_t)H * W;
    const int64_t p0 = ((int64_t)(blockIdx.x % blocks_per_frame) * DT_THREADS + (int64_t)threadIdx.x) * DT_GROUP;
    if (p0 >= pixels) return;
    const int count = pixels - p0 < DT_GROUP ? (int)(pixels - p0) : DT_GROUP;
    const vrg_detect_frame_desc d = desc[n];
    const bool ok = dt_frame_desc_ok(d, n_frames, n_transforms);
    uint8_t* o = out + (n * pixels + p0) * 3;
    const bool wide = count == DT_GROUP && (reinterpret_cast<uintptr_t>(o) & 15u) == 0;      // a whole group on a 16-byte boundary
    if (!ok) {
        if (wide) {
            dt_u4* q = reinterpret_cast<dt_u4*>(o);
            const dt_u4 zero = {0u, 0u, 0u, 0u};
            q[0] = zero; q[1] = zero; q[2] = zero;
        } else {
            for (int i = 0; i < count * 3; ++i) o[i] = 0;
        }
        return;
    }
    const int64_t frame_elems = pixels * C;
    DtSource<F32> src;
    src.base = F32 ? (const void*)(reinterpret_cast<const float*>(frames) + (int64_t)d.frame * frame_elems)
                   : (const void*)(reinterpret_cast<const uint8_t*>(frames) + (int64_t)d.frame * frame_elems);
    src.W = W;
    src.C = C;
    double m[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (d.transform >= 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = transforms[(int64_t)d.transform * 6 + i];
    }
    int32_t y = (int32_t)(p0 / W), x = (int32_t)(p0 - (int64_t)y * W);
    if (wide) {                                                                  // fully unrolled: the 12 words stay in registers
        uint32_t words[DT_GROUP * 3 / 4];
#pragma unroll
        for (int i = 0; i < DT_GROUP * 3 / 4; ++i) words[i] = 0u;
#pragma unroll
        for (int i = 0; i < DT_GROUP; ++i) {
            uint8_t b[3];
            if (d.transform < 0) src(y, x, b);
            else dt_warp_pixel(m, x, y, W, H, src, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) words[(3 * i + c) >> 2] |= (uint32_t)b[c] << (8 * ((3 * i + c) & 3));
            if (++x == W) { x = 0; ++y; }
        }
        dt_u4* q = reinterpret_cast<dt_u4*>(o);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dt_u4 v;
            v.x = words[4 * i]; v.y = words[4 * i + 1]; v.z = words[4 * i + 2]; v.w = words[4 * i + 3];
            q[i] = v;
        }
        return;
    }
#pragma unroll 1
    for (int i = 0; i < count; ++i) {                                            // the last, partial group or an unaligned frame: bytewise
        uint8_t b[3];
        if (d.transform < 0) src(y, x, b);
        else dt_warp_pixel(m, x, y, W, H, src, b);
        o[3 * i] = b[0];
        o[3 * i + 1] = b[1];
        o[3 * i + 2] = b[2];
        if (++x == W) { x = 0; ++y; }
    }
}

static int dt_check_frames(const void* frames, bool f32, int64_t n_frames, int32_t height, int32_t width, int32_t channels, const double* transforms,
                           int64_t n_transforms, const void* desc, int64_t n_out, const void* out) {
    if (n_frames < 0 || n_transforms < 0 || n_out < 0 || height < 1 || width < 1 || channels < 3 || (!f32 && channels != 3)) return VRG_ERR_BAD_ARG;
    if (height > DT_MAX_SIDE || width > DT_MAX_SIDE) return VRG_ERR_BAD_ARG;
    if (n_out == 0) return VRG_OK;
    if (!frames || !desc || !out || (n_transforms > 0 && !transforms) || n_frames < 1) return VRG_ERR_BAD_ARG;
    if ((f32 && (reinterpret_cast<uintptr_t>(frames) & 3u) != 0) || (reinterpret_cast<uintptr_t>(transforms) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(desc) & 3u) != 0 || frames == out)
        return VRG_ERR_BAD_ARG;
    if (n_frames > 0x7fffffffll || n_transforms > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    return -1;                                                                   // launch
}

static int dt_blobs(const void* frames, bool f32, int64_t n_frames, int32_t height, int32_t width, int32_t channels, const double* transforms,
                    int64_t n_transforms, const vrg_detect_desc* desc, int64_t n_blobs, float* out, void* stream) {
    const int st = dt_check_frames(frames, f32, n_frames, height, width, channels, transforms, n_transforms, desc, n_blobs, out);
    if (st >= 0) return st;
    if ((reinterpret_cast<uintptr_t>(out) & 3u) != 0) return VRG_ERR_BAD_ARG;
    if (n_blobs > 0x7fffffffll / DT_BLOCKS_PER_BLOB) return VRG_ERR_UNSUPPORTED;
    const dim3 grid((uint32_t)(n_blobs * DT_BLOCKS_PER_BLOB));
    if (f32)
        hipLaunchKernelGGL((k_detect_blobs<true>), grid, dim3(DT_THREADS), 0, (hipStream_t)stream, frames, transforms, desc, out, n_frames, n_transforms,
                           height, width, channels);
    else
        hipLaunchKernelGGL((k_detect_blobs<false>), grid, dim3(DT_THREADS), 0, (hipStream_t)stream, frames, transforms, desc, out, n_frames, n_transforms,
                           height, width, channels);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_linear_taps(int32_t n_in, int32_t n_out, int32_t* ofs_host, int16_t* coef_host) {
    if (!ofs_host || !coef_host || n_in < 1 || n_out < 1 || n_in > DT_MAX_SIDE || n_out > DT_MAX_SIDE) return VRG_ERR_BAD_ARG;
    dt_fill_taps(n_in, n_out, ofs_host, coef_host);
    return VRG_OK;
}

int vrg_detect_check(const vrg_detect_desc* desc_host, int64_t n_desc, int64_t n_frames, int32_t height, int32_t width, int64_t n_transforms) {
    if (n_desc < 0 || n_frames < 0 || n_transforms < 0 || height < 1 || width < 1 || height > DT_MAX_SIDE || width > DT_MAX_SIDE) return VRG_ERR_BAD_ARG;
    if (n_desc > 0 && !desc_host) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_desc; ++i)
        if (!dt_desc_ok(desc_host[i], n_frames, n_transforms, height, width)) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

int vrg_detect_blobs_f32(const float* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels, const double* transforms,
                         int64_t n_transforms, const vrg_detect_desc* desc, int64_t n_blobs, float* out, void* stream) {
    return dt_blobs(frames, true, n_frames, height, width, channels, transforms, n_transforms, desc, n_blobs, out, stream);
}

int vrg_detect_blobs_u8(const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, const double* transforms, int64_t n_transforms,
                        const vrg_detect_desc* desc, int64_t n_blobs, float* out, void* stream) {
    return dt_blobs(frames, false, n_frames, height, width, 3, transforms, n_transforms, desc, n_blobs, out, stream);
}

int vrg_warp_linear_u8(const void* frames, int32_t f32_channels, int64_t n_frames, int32_t height, int32_t width, const double* transforms,
                       int64_t n_transforms, const vrg_detect_frame_desc* desc, int64_t n_out, uint8_t* out, void* stream) {
    if (f32_channels != 0 && f32_channels < 3) return VRG_ERR_BAD_ARG;
    const bool f32 = f32_channels != 0;
    const int st = dt_check_frames(frames, f32, n_frames, height, width, f32 ? f32_channels : 3, transforms, n_transforms, desc, n_out, out);
    if (st >= 0) return st;
    const int64_t per_block = (int64_t)DT_THREADS * DT_GROUP;
    const int64_t blocks_per_frame = ((int64_t)height * width + per_block - 1) / per_block;
    if (n_out > 0x7fffffffll / blocks_per_frame) return VRG_ERR_UNSUPPORTED;
    const dim3 grid((uint32_t)(n_out * blocks_per_frame));
    if (f32)
        hipLaunchKernelGGL((k_warp_linear<true>), grid, dim3(DT_THREADS), 0, (hipStream_t)stream, frames, transforms, desc, out, n_frames, n_transforms, height,
                           width, f32_channels, (uint32_t)blocks_per_frame);
    else
        hipLaunchKernelGGL((k_warp_linear<false>), grid, dim3(DT_THREADS), 0, (hipStream_t)stream, frames, transforms, desc, out, n_frames, n_transforms, height,
                           width, 3, (uint32_t)blocks_per_frame);
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
