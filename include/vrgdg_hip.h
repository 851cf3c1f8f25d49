/*
 * vrgdg_hip.h -- C ABI of libvrgdg_hip.so: the MI355X (gfx950 / CDNA4) implementation of the
 * per-pixel video post-processing hot path of comfyui-vrgamedevgirl.
 *
 * This is the drop-in boundary: plain pointers, sizes and scalars, no torch types.  The Python
 * node classes (comfyui-vrgamedevgirl_amd/nodes.py, VRGDG_IV_Adjustments.py) bind it with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.  All image pointers are
 * DEVICE pointers to fp32 NHWC frames ([F][H][W][C], C innermost), values nominally in [0,1].
 * `stream` is a hipStream_t passed as void* (0 = the null stream); every entry point only
 * enqueues work on that stream and returns immediately.  No entry point allocates device memory;
 * scratch is supplied by the caller (sizes from the *_scratch_bytes helpers).
 *
 * Return value: 0 = ok; VRG_ERR_* otherwise (vrg_error_string() gives the text; the Python layer
 * raises RuntimeError / ValueError like the reference's nodes do).
 *
 * Arithmetic contract: every fp32 operation of the reference is performed
 * as its own correctly rounded fp32 operation in the reference's order -- the kernels are built
 * with -ffp-contract=off and use IEEE divide / sqrt.  Scalars that the reference computes in
 * Python doubles (1.0 - s, strength/10, ...) are computed by the CALLER in double and passed
 * here already rounded to fp32.
 */
#ifndef VRGDG_HIP_H_
#define VRGDG_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRG_ABI_VERSION 8

enum vrg_status {
    VRG_OK = 0,
    VRG_ERR_BAD_ARG = 1,      /* null pointer, negative size, C < 3 where RGB is required ... */
    VRG_ERR_UNSUPPORTED = 2,  /* valid request this build does not implement */
    VRG_ERR_LAUNCH = 3,       /* hipLaunchKernel / hipGetLastError failed */
    VRG_ERR_NO_DEVICE = 4
};

/* Operands must not overlap.  The kernels take every operand through a restrict-qualified pointer, and nearly all of them read pixels
 * other than the one they store (3x3 and 9x9 windows, resampling taps, crop gathers; the marches store a last strip twice).  An entry
 * point whose operand sizes follow from its scalar arguments therefore returns VRG_ERR_BAD_ARG, before it touches a device, when an
 * operand it writes (out, mask_out, the tmp ring of vrg_adjust_*) shares a byte with an operand it reads or with another one it writes.
 * Operands are half-open byte ranges; one of no bytes overlaps nothing, and ranges that only touch are fine.  Entry points that reach
 * their inputs through descriptor tables check what they can; for them the caller keeps the outputs apart from every picture the
 * records name (ops.py does, with the same rule, in ops._disjoint). */

enum vrg_border {
    VRG_BORDER_REPLICATE = 0, /* reference CPU/numpy path: np.pad(mode="edge")            (nodes.py:188-192) */
    VRG_BORDER_ZERO = 1       /* reference use_gpu=True path: avg_pool2d / conv2d padding=1 (nodes.py:171, 257) */
};

enum vrg_stencil_op {
    VRG_STENCIL_UNSHARP = 0,        /* FastUnsharpSharpen.apply_unsharp     nodes.py:156-209 */
    VRG_STENCIL_LAPLACIAN = 1,      /* FastLaplacianSharpen.apply_laplacian nodes.py:234-289 */
    VRG_STENCIL_SOBEL = 2,          /* FastSobelSharpen.apply_sobel         nodes.py:314-384 */
    VRG_STENCIL_NONE = 3
};

/*
 * Noise stream description: the torch-HIP `randn` mapping (ATen DistributionTemplates.h:52-99,
 * rocrand_philox4x32_10.h, rocrand_normal.h:52-68).  The frames are cut into RNG chunks of
 * `chunk_frames` frames (FastFilmGrain: batch_size, nodes.py:46-51; per-frame seeding: 1,
 * VRGDG_StandaloneVideoEnhancerNodes.py:268-271).  Chunk j (absolute index chunk0 + j) draws
 *     randn(chunk_numel) with Philox key  seed0 + (chunk0+j)*seed_stride,
 *                              offset      offset0 + (chunk0+j)*offset_stride   (multiple of 4)
 * and element li of the chunk takes component (li / G) % 4 of call (li / G) / 4 of Philox
 * subsequence li % G.  `grid_threads` = G = grid.x*256 of torch's calc_execution_policy for
 * chunk_numel on this device.  All chunks of one call must have the same numel (the host issues
 * a second call for a ragged tail chunk).
 */
typedef struct vrg_noise_desc {
    uint64_t seed0;
    uint64_t seed_stride;
    uint64_t offset0;
    uint64_t offset_stride;
    int64_t  chunk0;        /* absolute index of the first chunk handled by this call */
    int32_t  chunk_frames;  /* frames per RNG chunk (>= 1) */
    uint32_t grid_threads;  /* G */
} vrg_noise_desc;

/*
 * Split noise: ONE `randn` of more than 2^29 elements, which ATen runs as several kernels over 32-bit indexable sub-ranges
 * (TensorIteratorBase::with_32bit_indexing), every sub-range ("leaf") with a grid and a generator offset of its own.  A launch names the
 * leaves its frames meet, in memory order and without gaps: `start` is the leaf's first element relative to the FIRST ELEMENT OF THE
 * LAUNCH (negative where the leaf begins before it), and element e of the launch, start <= e < start + size, takes the value
 * vrg_noise_desc describes for element e - start of a chunk drawn with `grid_threads` at `offset`.  The record travels in the
 * kernel arguments: nothing is uploaded.  count in 1 .. VRG_NOISE_LEAVES_MAX, every grid_threads a non-zero multiple of 256, the leaves
 * cover the launch's elements; anything else is VRG_ERR_BAD_ARG.
 */
#define VRG_NOISE_LEAVES_MAX 8
typedef struct vrg_noise_leaf {
    int64_t  start;
    uint32_t size;
    uint32_t grid_threads;
    uint64_t offset;        /* multiple of 4 */
} vrg_noise_leaf;
typedef struct vrg_noise_split {
    uint64_t seed;
    int32_t  count;
    int32_t  reserved;
    vrg_noise_leaf leaves[VRG_NOISE_LEAVES_MAX];
} vrg_noise_split;

/* Film grain over frames whose noise is a split draw: vrg_grain_f32 with the noise of `split`.  Frames are whole frames of the draw, in
 * any number; a frame may lie across leaves, and a leaf may begin or end inside a pixel. */
int vrg_grain_split_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                        float intensity, float sat, float one_minus_sat,
                        const vrg_noise_split* split, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1/a2  Film grain.  Replaces FastFilmGrain.apply_grain (nodes.py:41-66),
 * _apply_film_grain_tensor (VRGDG_LUTVideoTools.py:262-277) and _apply_seeded_grain
 * (VRGDG_StandaloneVideoEnhancerNodes.py:262-278).
 *   g_c = fl(fl(S*fl(k_c*n_c)) + fl(T*n_G)),  k = (2,1,3);  out = clamp(fl(x + fl(g_c*I)), 0, 1)
 * `frames` must be a whole number of RNG chunks except that the last chunk may not be ragged
 * (see vrg_noise_desc).  C is fixed at 3.
 * ------------------------------------------------------------------------------------------- */
int vrg_grain_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                  float intensity, float sat, float one_minus_sat,
                  const vrg_noise_desc* noise, void* stream);

/* f1  Unsharp, then per-frame-seeded grain, in ONE pass over the frames (24 B/px instead of 48): the effect order of the stand-alone
 * enhancer, _apply_effects_batch = _apply_unsharp then _apply_seeded_grain (VRGDG_StandaloneVideoEnhancerNodes.py:233-294).
 * out = vrg_grain_f32(vrg_stencil3x3_f32(in, VRG_OP_UNSHARP, border, strength), ...) bit for bit; `noise` as for vrg_grain_f32 with
 * chunk_frames == 1 (one generator per frame).  in != out.  Returns VRG_ERR_UNSUPPORTED -- and the caller runs the two entry points
 * above -- unless width % 4 == 0, width * 3 / 4 >= 256, chunk_frames == 1 and both pointers are 16-byte aligned. */
int vrg_sharpen_grain_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                          float strength, int32_t border, float intensity, float sat, float one_minus_sat,
                          const vrg_noise_desc* noise, void* stream);

/* f1 x f3  The same pass on DECODED frames, uint8 B,G,R in and out -- the stand-alone enhancer's render loop body
 * _tensor_to_frames(_apply_effects_batch(_frames_to_tensor(frames))) (VRGDG_StandaloneVideoEnhancerNodes.py:311-324, 278-294,
 * 417-421) as ONE kernel moving 3 + 3 B/px: v / 255 at the load, unsharp (border as above), per-frame-seeded grain,
 * clip(x * 255, 0, 255) truncated to uint8 at the store.  out = vrg_f32rgb_to_u8bgr(vrg_sharpen_grain_f32(vrg_u8bgr_to_f32rgb(in)))
 * byte for byte.  in != out.  Any width, height and pointer alignment (ABI v7: frames with width % 4 == 0, width * 3 / 4 >= 256 and
 * 4-byte aligned pointers run on the frame's dword grid; everything else -- 854 x 480, 1366 x 768, thumbnails, frames that start off a
 * dword -- in flat byte space with unaligned dword accesses, same bytes).  VRG_ERR_UNSUPPORTED (the caller runs that three-kernel
 * route) only for chunk_frames != 1 and for a batch of fewer than four bytes. */
int vrg_sharpen_grain_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t height, int32_t width,
                         float strength, int32_t border, float intensity, float sat, float one_minus_sat,
                         const vrg_noise_desc* noise, void* stream);

/* Same arithmetic with the N(0,1) noise supplied by the caller (device pointer, same shape as
 * `in`): the noise-injection form used to prove arithmetic parity against the CPU reference. */
int vrg_grain_injected_f32(const float* in, const float* noise, float* out, int64_t pixels,
                           float intensity, float sat, float one_minus_sat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a4/a5/a6  3D LUT trilinear apply + strength blend.  Replaces VRGDG_LUTS._apply_cube_lut and
 * the blend in apply_lut (VRGDG_IV_Adjustments.py:288-361), _apply_lut_tensor
 * (VRGDG_LUTVideoTools.py:172-185).
 * A LUT is prepared once: vrg_lut_prepare_f32 rewrites the parsed table `lut` (device fp32
 * [N][N][N][3] indexed [blue][green][red], as _parse_cube_file returns it) into the gather-friendly
 * form the kernels read -- (N-1)^2*N records of 12 floats, one per (b0, g0, red node), the four (g,b)
 * corner values of each channel copied verbatim -- so that a pixel fetches one contiguous 96-byte
 * run (red nodes r0, r0+1) instead of eight scattered corners.  `cells` must hold vrg_lut_cells_floats(N) floats, 16-byte aligned.  2 <= N <= 256.
 * `channels` >= 3; channels beyond RGB are copied through.  blend_mode: 1 = LUT only (blend>=1),
 * 2 = fl(fl(x*one_minus_blend) + fl(y*blend)).  (blend <= 0 is the caller's no-op.)
 * ------------------------------------------------------------------------------------------- */
int64_t vrg_lut_cells_floats(int32_t lut_size);
int vrg_lut_prepare_f32(const float* lut, int32_t lut_size, float* cells, void* stream);
int vrg_lut3d_f32(const float* in, float* out, int64_t pixels, int32_t channels,
                  const float* cells, int32_t lut_size,
                  const float domain_min[3], const float domain_max[3],
                  int32_t blend_mode, float blend, float one_minus_blend, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a9/a10/a11  3x3 stencils, any channel count.  out = clamp(x + strength*f(3x3), 0, 1).
 * Sum orders: see csrc/vrg_pixel_math.hpp (reference order for the replicate border; raster
 * (kh,kw) order over the non-zero taps for the zero border).
 * ------------------------------------------------------------------------------------------- */
int vrg_stencil3x3_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                       int32_t channels, int32_t op, int32_t border, float strength, void* stream);

/* Arithmetic policy of the Lab transforms and the statistics transfer (a7/a8).
 *   VRG_CM_MATH_DEVICE (default): every element-wise op is the one torch-ROCm executes for it on this GPU -- what the
 *       reference computes when ComfyUI runs ColorMatchToReference on the MI355X (nodes.py:98-115): `tensor / python
 *       scalar` = x * fl(1/c), torch.pow = ocml powf, tensor / tensor = IEEE quotient.  Bit-equal to the restated kornia
 *       formulas evaluated by torch on the device (tests/test_gpu_parity.py), given the same statistics.
 *   VRG_CM_MATH_FAST: IEEE quotients (torch-CPU behaviour) and table-driven powers with <= 0.534 ulp error instead of
 *       ocml powf: a few ulp from either reference, 1.2-1.4x faster than the device policy (which reaches ocml's value through
 *       a cheaper logarithm plus a rounding test, and through ocml's own operation sequence where the test fails). */
enum vrg_cm_math { VRG_CM_MATH_DEVICE = 0, VRG_CM_MATH_FAST = 1 };

/* ---------------------------------------------------------------------------------------------
 * a7/a8  Colour match (nodes.py:91-124 + kornia.color Lab transforms).
 * Pass 1: per-frame Lab statistics.  stats[f][c] = {n, mean, M2} in fp64 (M2 = sum (x-mean)^2),
 * c = L,a,b.  Deterministic two-stage reduction (no atomics).  `scratch` must hold
 * vrg_lab_stats_scratch_bytes(frames) bytes.
 * Pass 2: out = clamp(lab_to_rgb(K*((lab-mu)/sigma*sigma_ref+mu_ref) + T*lab)).
 *   img_ms / ref_ms: device fp32 [frames][3][2] = {mean, std_unbiased + 1e-5} (vrg_lab_stats_finalize
 *   converts the fp64 triple); ref frame of image frame f = (ref_frames == 1) ? 0 : f % ref_frames.
 * ------------------------------------------------------------------------------------------- */
int64_t vrg_lab_stats_scratch_bytes(int64_t frames);
int vrg_lab_stats_f32(const float* in, int64_t frames, int32_t height, int32_t width,
                      double* stats, void* scratch, int32_t cm_math, void* stream);
int vrg_lab_stats_finalize(const double* stats, float* mean_std, int64_t frames, void* stream);
/* The same statistics with the BITS the reference gets on this GPU: `lab.mean(dim=[2,3])` / `lab.std(dim=[2,3]) + 1e-5` as
 * torch-ROCm evaluates them (nodes.py:99-100, 109-110) -- ATen's reduce_kernel with MeanOps / WelfordOps in fp32, whose value
 * depends on the launch geometry torch derives from the tensor shape ([chunk_frames,3,H,W] per call: the node's batch_size, or the
 * whole reference batch), on the order in which thread accumulators, lanes and warps are combined, and on which multiply-adds of
 * the Welford update hipcc contracted in libtorch_hip.so.  csrc/vrg_torch_stats.hip replays that computation (geometry of the
 * MI355X: 256 CUs; VRG_ERR_UNSUPPORTED elsewhere) on the interleaved Lab image `lab` ([frames][H][W][3] fp32: the `lab_out` of
 * vrg_chain_stats_lab_f32).  Frames are taken `chunk_frames` per reference call, the last call holds the remainder.
 * mean_std = device fp32 [frames][3][2] = {mean, std + eps} (eps = 1e-5f for the node), the layout vrg_colormatch_apply_f32 /
 * vrg_chain_desc::img_ms / ref_ms read.  With these statistics the whole colour match is bit-equal to the reference's formulas
 * evaluated by torch on the device (tests/test_gpu_parity.py). */
int vrg_lab_stats_torch_f32(const float* lab, int64_t frames, int32_t height, int32_t width, int32_t chunk_frames,
                            float* mean_std, float eps, void* stream);
/* The same with a caller-supplied scratch buffer (16-byte aligned, vrg_lab_stats_torch_scratch_bytes(frames) bytes -- 0 when the batch is
 * too large for the form that uses one; NULL = none): small batches of video-sized frames are then reduced by EIGHT half-block
 * workgroups per frame (one wave per SIMD: the dependent Welford update chains are issue bound next to a second wave) plus a finishing
 * kernel.  Same result bits. */
int64_t vrg_lab_stats_torch_scratch_bytes(int64_t frames);
int vrg_lab_stats_torch_ws_f32(const float* lab, int64_t frames, int32_t height, int32_t width, int32_t chunk_frames,
                               float* mean_std, float eps, void* scratch, int64_t scratch_bytes, void* stream);
/* The same statistics with the LATENCY form allowed for calls of at most two frames (one accumulator per lane: seven-wave workgroups,
 * 65 KB of LDS each -- 0.78 instead of 1.12 ms for one 4K frame on an otherwise idle GPU, slower than the automatic choice beside a
 * full-size pass): for the reference frame's statistics of a small step.  Same arguments, same result bits. */
int vrg_lab_stats_torch_lat_f32(const float* lab, int64_t frames, int32_t height, int32_t width, int32_t chunk_frames,
                                float* mean_std, float eps, void* scratch, int64_t scratch_bytes, void* stream);
int vrg_colormatch_apply_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                             const float* img_ms, const float* ref_ms, int32_t ref_frames,
                             float k, float one_minus_k, int32_t cm_math, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: frames shard across ranks with no data-path collective; the one exchange is this --
 * (n, mean, M2) triples of DISJOINT pixel sets (the rows of a reference frame reduced on different GPUs, vrg_lab_stats_f32 on
 * each rank's row slice) are combined in place into the statistics of their union with two SUM all-reduces over RCCL / xGMI
 * enqueued on `stream`: (n, n*mean) gives the global mean, then M2 + n*(mean - mean_tot)^2 gives the global M2.  72 bytes per
 * reference frame: latency bound.  `comm` is the caller's ncclComm_t (RCCL's nccl.h), passed as void*; `stats` = `count`
 * triples (count = frames*3), `scratch` = vrg_stats_allreduce_scratch_bytes(count) bytes of device memory.  RCCL is resolved
 * at run time from the copy the process already loaded (the library links only the HIP runtime): VRG_ERR_UNSUPPORTED when
 * there is none.  The Python host performs the same arithmetic through torch.distributed (sharding.allreduce_stats).
 * ------------------------------------------------------------------------------------------- */
int64_t vrg_stats_allreduce_scratch_bytes(int64_t count);
int vrg_stats_allreduce(double* stats, int64_t count, void* comm, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused chain: grain -> LUT -> colour match -> 3x3 sharpen in one pass over HBM (12 B/px read +
 * 12 B/px written; colour match adds the 12 B/px statistics pass).  Bit-identical to running the
 * stand-alone entry points one after the other.  Stages are switched by `stages`.
 * ------------------------------------------------------------------------------------------- */
#define VRG_STAGE_GRAIN      1
#define VRG_STAGE_LUT        2
#define VRG_STAGE_COLORMATCH 4
#define VRG_STAGE_SHARPEN    8
/* With VRG_STAGE_COLORMATCH: `in` already holds the Lab image of the colour-match input (written by
 * vrg_chain_stats_lab_f32), so grain / LUT / rgb_to_lab are not re-evaluated in the apply pass. */
#define VRG_STAGE_FROM_LAB   16

typedef struct vrg_chain_desc {
    int32_t stages;               /* VRG_STAGE_* bits */
    int32_t variant;              /* 0 = automatic; 1 = LDS-tile / point-wise kernels; 2 = register-resident wave-march kernel
                                     (chains it cannot take -- colour match, chunks > 0x60000000 elements -- use 1) */
    /* grain */
    float intensity, sat, one_minus_sat;
    vrg_noise_desc noise;
    /* LUT (cell-major table from vrg_lut_prepare_f32) */
    const float* lut; int32_t lut_size;
    float domain_min[3], domain_max[3];
    int32_t blend_mode; float blend, one_minus_blend;
    /* colour match (statistics of the LUT output are produced by vrg_chain_stats_f32) */
    const float* img_ms; const float* ref_ms; int32_t ref_frames;
    float k, one_minus_k;
    /* sharpen */
    int32_t stencil_op, border; float strength;
    /* colour-match arithmetic policy: enum vrg_cm_math (0 = device-exact, the default) */
    int32_t cm_math;
} vrg_chain_desc;

int vrg_fused_chain_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                        const vrg_chain_desc* desc, void* stream);
/* Lab statistics of the grain->LUT output (the input of the colour-match stage), same layout and
 * as vrg_lab_stats_f32; `scratch` must hold vrg_chain_stats_scratch_bytes(...) bytes. */
int vrg_chain_stats_f32(const float* in, int64_t frames, int32_t height, int32_t width,
                        const vrg_chain_desc* desc, double* stats, void* scratch, void* stream);
/* Scratch size for vrg_chain_stats_f32 / vrg_chain_stats_lab_f32 with this descriptor (chains that start with
 * grain use a pass that shares the Philox work and keeps one partial record per (workgroup, strip)). */
int64_t vrg_chain_stats_scratch_bytes(int64_t frames, int32_t height, int32_t width, const vrg_chain_desc* desc);
/* Same pass, additionally storing the Lab image it reduces (`lab_out`, same shape as `in`): the apply pass
 * then runs with VRG_STAGE_COLORMATCH | VRG_STAGE_FROM_LAB (| VRG_STAGE_SHARPEN) on `lab_out`.  Trades
 * 12 B/px of extra HBM traffic for not evaluating grain, the LUT gathers and six powers twice -- the chain is
 * ALU / L1-request bound, not HBM bound.  Results are bit-identical to the recomputing form.
 * `stats` may be NULL (then `scratch` may be NULL too): only the Lab image is produced -- the form used with the device
 * statistics (vrg_lab_stats_torch_f32 reduces `lab_out`). */
int vrg_chain_stats_lab_f32(const float* in, float* lab_out, int64_t frames, int32_t height, int32_t width,
                            const vrg_chain_desc* desc, double* stats, void* scratch, void* stream);
/* The same three with the grain stage's noise taken from `split` (vrg_noise_split) instead of desc->noise, which is ignored: desc->stages
 * must hold VRG_STAGE_GRAIN.  Always the LDS-tile / point-wise kernels and the general statistics pass (the wave-march and
 * shared-Philox kernels address one chunk with one grid); a colour-match stage in the apply pass is VRG_ERR_UNSUPPORTED -- pass 2 runs
 * from the Lab image of vrg_chain_stats_lab_split_f32 through vrg_fused_chain_f32, which has no grain stage left.  `scratch` holds
 * vrg_lab_stats_scratch_bytes(frames) bytes. */
int vrg_fused_chain_split_f32(const float* in, float* out, int64_t frames, int32_t height, int32_t width,
                              const vrg_chain_desc* desc, const vrg_noise_split* split, void* stream);
int vrg_fused_chain_split_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t height, int32_t width,
                             const vrg_chain_desc* desc, const vrg_noise_split* split, void* stream);
int vrg_chain_stats_lab_split_f32(const float* in, float* lab_out, int64_t frames, int32_t height, int32_t width,
                                  const vrg_chain_desc* desc, const vrg_noise_split* split, double* stats, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 13-slider Adjust of the video routes.
 * Replaces _apply_adjust_tensor, VRGDG_LUTVideoTools.py:307-391: clamp, white balance (temperature / tint),
 * exposure, contrast, saturation, highlights / shadows / whites / blacks masks, clarity (k x k reflect box,
 * k = min(9, odd(H), odd(W))), sharpen (3x3 replicate box), fade, vignette, clamp.  The host rounds the
 * slider arithmetic (Python doubles, :309-315) once to fp32 and passes the terms below; the kernels keep the
 * reference's fp32 rounding order, including avg_pool2d's raster-order running sums.
 * `tmp` (same shape as `in`) is needed only when clarity and sharpen are both active; it may be NULL otherwise.
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_adjust_desc {
    int32_t enabled;                 /* 0: output = clamp(in, 0, 1) (:308) */
    float shift[3];                  /* temp/400 - tint/900, tint/450, -temp/400 - tint/900 (:319-326) */
    float exposure;                  /* 2 ** (exposure/100) (:327) */
    float contrast, saturation;      /* 1 + slider/100 (:328,330) */
    float highlights, shadows;       /* slider/220 (:336-337) */
    float whites, blacks;            /* slider/240 (:338-339) */
    int32_t has_clarity; float clarity;      /* slider != 0; slider/100 (:342-356) */
    int32_t has_sharpen; float sharpen;      /* slider > 0;  slider/100 (:358-372) */
    int32_t has_fade; float fade_mul, fade_add;   /* 1 - fade*0.35, fade*0.18 (:374-375) */
    int32_t has_vignette; float vignette;    /* slider > 0; slider/100 (:377-389) */
    /* `tensor / 0.45`, `/ 1.05` (:333-334, :388): the reference runs on the device its `device` argument names -- the
     * IEEE quotient on the CPU, x * fl32(1.0 / c) on the GPU (ATen BinaryDivTrueKernel).  enum vrg_adjust_div. */
    int32_t div_mode;
} vrg_adjust_desc;
enum vrg_adjust_div { VRG_ADJUST_DIV_IEEE = 0, VRG_ADJUST_DIV_DEVICE = 1 };

int vrg_adjust_f32(const float* in, float* out, float* tmp, int64_t frames, int32_t height, int32_t width,
                   const vrg_adjust_desc* desc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * uint8 BGR frames at the video I/O edge.
 * Replaces _frames_to_tensor / _tensor_to_frames (VRGDG_LUTVideoTools.py:736-752,
 * VRGDG_StandaloneVideoEnhancerNodes.py:311-324): `astype(float32) / 255.0` after the BGR->RGB swap on the way
 * in, `clip(x * 255.0, 0, 255).astype(uint8)` (truncation) and RGB->BGR on the way out.  In the *_u8 entry points
 * both conversions happen inside the kernel that does the work, so a route batch (_process_video_batch,
 * _process_film_grain_batch, _process_adjust_batch, :1365-1386) moves 3 + 3 B/px instead of 12 + 12; results are
 * identical to convert -> fp32 entry point -> convert.  Frames are [frames][height][width][3] uint8, B,G,R order.
 * ------------------------------------------------------------------------------------------- */
int vrg_u8bgr_to_f32rgb(const uint8_t* in, float* out, int64_t pixels, void* stream);
int vrg_f32rgb_to_u8bgr(const float* in, uint8_t* out, int64_t pixels, void* stream);
/* Exact per-frame channel sums of uint8 frames, `sums` = [frames][3 channels in memory order][sum, sum of squares]
 * as 64-bit integers (zeroed by the call).  Replaces PIL.ImageStat.Stat(...).sum / .sum2 in the opening colour match
 * (VRGDG_WorkflowRunnerNodes.py:4385-4392); mean / stddev follow on the host in double exactly as ImageStat does. */
int vrg_u8_channel_sums(const uint8_t* frames, int64_t frames_n, int32_t height, int32_t width, unsigned long long* sums,
                        void* stream);
/* The per-pixel step of the opening colour match with ffmpeg's filter arithmetic instead of this library's LUT stage
 * (reference filter graph lut3d + blend, VRGDG_WorkflowRunnerNodes.py:4407-4412): tetrahedral interpolation of the cube on
 * 8-bit B,G,R frames, truncation to 8 bits, then `A*(1-w)+B*w` in double per byte with the per-frame weight `weights[f]`
 * (device pointer, NULL = no blend), truncated.  `table` = the parsed .cube [N][N][N][3] fp32 (index [blue][green][red]) on
 * the device, `domain_min/max` = host float[3].  Restated from ffmpeg's published sources (libavfilter/vf_lut3d.c,
 * vf_blend.c); ffmpeg is absent here, so this entry point's parity is unpinned. */
int vrg_lut3d_tetra_u8(const uint8_t* in, uint8_t* out, int64_t frames, int64_t pixels_per_frame, const float* table,
                       int32_t lut_size, const float* domain_min, const float* domain_max, const double* weights, void* stream);
/* grain / LUT / 3x3 sharpen in any combination (no colour match: VRG_ERR_UNSUPPORTED); desc as for vrg_fused_chain_f32 */
int vrg_fused_chain_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t height, int32_t width,
                       const vrg_chain_desc* desc, void* stream);
/* `tmp`: fp32, frames*height*width*3 floats, needed only when clarity and sharpen are both active */
int vrg_adjust_u8(const uint8_t* in, uint8_t* out, float* tmp, int64_t frames, int32_t height, int32_t width,
                  const vrg_adjust_desc* desc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame resize and the Video Enhance restore.  Replaces _resize_batch / _restore_batch (VRGDG_VideoEnhanceNodes.py:54-106) and
 * the blend of VRGDGVideoEnhanceRestoreOriginal.restore (:404-419).
 * Arithmetic: torch's CPU kernels behind F.interpolate in their plain one-rounding-per-operation form (what
 * ATEN_CPU_CAPABILITY=default executes), fp32 throughout: bicubic (A = -0.75) and bilinear with align_corners = False, area
 * (adaptive average pooling) and nearest (csrc/vrg_resize_math.hpp states each rule).  torch's AVX2 / AVX-512 builds differ from that
 * form -- and so from these kernels -- by a few ulp(1.0) in most elements.
 * ------------------------------------------------------------------------------------------- */
enum vrg_resize_method { VRG_RESIZE_BICUBIC = 0, VRG_RESIZE_BILINEAR = 1, VRG_RESIZE_AREA = 2, VRG_RESIZE_NEAREST = 3 };

/* The source rectangle (src_x0, src_y0, src_w, src_h) of the RGB of every [in_h][in_w][in_channels >= 3] frame is resampled to
 * dst_w x dst_h and written at (dst_x0, dst_y0) of the [out_h][out_w][3] output frame, clamped to [0, 1]; the rest of the output is
 * zero.  The source rectangle lies inside the input frame.  The destination rectangle may hang over the output frame (negative
 * offsets, or a size past the frame): only its part inside is produced, at the resample positions of the whole rectangle -- stretch
 * is dst = the frame, crop to fill a dst larger than the frame, letterbox a dst inside it, the letterbox undo a src rectangle.  The
 * caller computes the rectangles (the reference does so with Python's round() and //).  in != out. */
int vrg_resize_f32(const float* in, float* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t in_channels,
                   int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h, int32_t out_h, int32_t out_w,
                   int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h, int32_t method, void* stream);

/* The fused restore: `work` = work_frames working-resolution frames, `originals` and `out` = frames [out_h][out_w][channels >= 3]
 * frames.  For frame f < min(work_frames, frames):
 *     out.rgb = clamp(fl(fl(originals.rgb * one_minus_strength) + fl(clamp(resampled, 0, 1) * strength)), 0, 1)
 * with `resampled` as vrg_resize_f32 produces it for the same geometry, further channels = clamp(originals, 0, 1); the remaining
 * frames = clamp(originals, 0, 1).  one_minus_strength = (float)(1.0 - strength) formed in double by the caller.  `out` aliases
 * neither input. */
int vrg_restore_f32(const float* work, const float* originals, float* out, int64_t work_frames, int64_t frames,
                    int32_t in_h, int32_t in_w, int32_t in_channels, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                    int32_t out_h, int32_t out_w, int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h,
                    int32_t channels, int32_t method, float strength, float one_minus_strength, void* stream);

/* The pixels of VRGDGVideoEnhancePrepare.prepare (:224-228) in one launch: output frame i is the resize of source frame frame_index[i]
 * of `in` = [frames][in_h][in_w][in_channels >= 3], by the geometry and method rules of vrg_resize_f32 and bit-identical to it.
 * `frame_index`: n_out entries in DEVICE memory, in any order and with repeats, or null for source frames 0 .. n_out - 1; the caller checks
 * the list (an entry outside 0 .. frames - 1 is VRG_ERR_BAD_ARG there); the kernel leaves the output frame of such an entry unwritten
 * and reads nothing for it.  Both outputs are [n_out][out_h][out_w][3] and come from the same computed value v in [0, 1]: out_f32 gets
 * v, out_u8 gets rintf(v * 255.0f) as R,G,B bytes -- the fp32 product rounded half to even, numpy's (x * 255).round().astype("uint8")
 * of _save_image_batch (:117).  Letterbox padding is 0.0f and 0.  Either output may be null, not both; no two of `in`, `frame_index`,
 * `out_f32` and `out_u8` may overlap anywhere in the bytes the call covers (checked: VRG_ERR_BAD_ARG).  n_out == 0 succeeds without a launch; frames == 0 with n_out > 0 is VRG_ERR_BAD_ARG.  Bicubic brings every
 * source row a band of output rows needs through LDS once (csrc/vrg_prepare.hip); the other methods run the direct form. */
int vrg_prepare_frames_f32(const float* in, int64_t frames, int32_t in_h, int32_t in_w, int32_t in_channels,
                           const int32_t* frame_index, int64_t n_out, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                           int32_t out_h, int32_t out_w, int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h, int32_t method,
                           float* out_f32, uint8_t* out_u8, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Feathered crop composite.  Replaces the per-frame loops of VRGDG_ImagePasteBack.paste_back (VRGDG_ImagePasteBack.py:224-260),
 * VRGDGFaceFixComposite.composite and VRGDGFaceFixCompositeOpaque.composite (VRGDG_StandaloneFaceFixNodes.py:827-849, 891-916):
 * a crop / work frame is bicubic-resized to a box of the frame, an analytic alpha (x an optional bilinear-resized user mask) is
 * formed, the crop is optionally shifted towards the mean colour of the frame under the alpha (measured on the device), blended in,
 * and the whole frame clamped.  csrc/vrg_composite_math.hpp states each rule.
 * ------------------------------------------------------------------------------------------- */
enum vrg_composite_rule {
    VRG_COMPOSITE_NONE = 0,        /* no box: out = clamp(original, 0, 1) (or the original itself: VRG_COMPOSITE_RAW_COPY), mask = 0 */
    VRG_COMPOSITE_ELLIPSE = 1,     /* Paste Back: p = cx, cy, rx, ry, min(rx, ry), feather */
    VRG_COMPOSITE_RECTANGLE = 2,   /* Paste Back: p = inset, width - 1 - inset, height - 1 - inset, -, -, feather */
    VRG_COMPOSITE_RADIAL = 3,      /* Face Fix: p = linspace step x, step y, feather_scale, entry strength */
    VRG_COMPOSITE_OPAQUE = 4       /* Face Fix Opaque: p = linspace step x, step y, edge */
};
enum vrg_composite_flags {
    VRG_COMPOSITE_CLAMP_CROP = 1,  /* clamp the resampled crop to [0, 1] before anything else (Face Fix) */
    VRG_COMPOSITE_MATCH = 2,       /* colour match requested (strength > 0): the frame is measured by vrg_composite_stats_f32 */
    VRG_COMPOSITE_STEP = 4,        /* feather <= 0 / edge <= 0: alpha is the 0 / 1 step */
    VRG_COMPOSITE_USER_MASK = 8,   /* multiply the resized, clamped user mask in */
    VRG_COMPOSITE_RAW_COPY = 16    /* with VRG_COMPOSITE_NONE: out = original as it is, not clamped (Paste Back with the rectangle outside the frame) */
};
/* One OUTPUT frame.  The box (left, top, box_w x box_h) is the resample target; paste_w x paste_h is its part inside the frame
 * (the box may hang over the right / bottom edge; left, top >= 0).  All constants are fp32 roundings of the reference's Python
 * doubles, formed by the caller. */
typedef struct vrg_composite_desc {
    int32_t rule, flags;
    int32_t original_index, crop_index, mask_index;   /* frames of `originals`, `crops`, `user_mask` this output frame reads */
    int32_t left, top, box_w, box_h, paste_w, paste_h;
    float match_strength;                              /* (float)color_match */
    float threshold;                                   /* selected = alpha > threshold: 0.25 Paste Back, 0.35 Face Fix */
    float p[7];
} vrg_composite_desc;

/* Bytes of `scratch` for vrg_composite_stats_f32 measuring `frames` frames whose pasted regions hold at most `max_box_pixels`. */
int64_t vrg_composite_scratch_bytes(int64_t frames, int64_t max_box_pixels);

/* Measures the `n_match` output frames listed in `match_frames` (device, int32, ascending): over the pixels of the pasted region
 * with alpha > threshold, the selected count and the fp64-accumulated means of the resampled crop and of the original under it.
 * Writes for each listed frame f the record stats[f] of 16 32-bit words: [0] count (int32), [1] matched = count >= 16 (int32),
 * [2..5] crop means, [6..9] original means, [10..13] shift = fl(fl(original mean - crop mean) * match_strength) (fp32; channels
 * past `match_channels` and everything of an unmatched frame's shift are 0), [14..15] 0.  Records of other frames are not touched.
 * Partial sums are combined in a fixed order: the same inputs give the same bits on every run.  `desc`: device, one record per
 * output frame.  crops [.][crop_h][crop_w][crop_channels], originals [.][height][width][channels], user_mask (or NULL)
 * [.][mask_h][mask_w] with `mask_stride` floats between mask pixels; match_channels (3 or 4) <= both channel counts.  `frames` = records in `desc`
 * and `stats`; a record whose indices or box do not fit the stated frame counts and sizes is treated as VRG_COMPOSITE_NONE. */
int vrg_composite_stats_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                            const int32_t* match_frames, int64_t n_match, int64_t max_box_pixels,
                            int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                            int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                            int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels,
                            void* scratch, void* stats, void* stream);

/* One pass over `frames` output frames [height][width][channels] and their masks [height][width]: outside the frame's box
 * out = clamp(original, 0, 1), mask = 0; inside, the first match_channels channels are
 *     clamp(fl(fl(original * fl(1 - alpha)) + fl(crop' * alpha)), 0, 1),  crop' = matched ? clamp(crop + shift, 0, 1) : crop
 * with `matched` and `shift` from stats[f] when the frame has VRG_COMPOSITE_MATCH, further channels clamp(original), mask = alpha.
 * `out` aliases no input.  channels is 3 or 4. */
int vrg_composite_apply_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                            const void* stats, float* out, float* mask_out,
                            int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                            int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                            int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Face Fix crop sequence.  Replaces the per-frame crop (slice, permute, F.interpolate bicubic, permute, clamp), the hole filling, the
 * LTX prefix and the torch.stack of VRGDGFaceFixPrepare.prepare and VRGDGFaceFixPrepareShotAware.prepare
 * (VRGDG_StandaloneFaceFixNodes.py:320-351, 387-389, 486-516, 537-539): one launch produces the whole 512 x 512 work batch.
 * ------------------------------------------------------------------------------------------- */
/* One OUTPUT frame: the rectangle of RGB(+) pixels it is resampled from.  A rectangle inside device-resident frames [F][H][W][C] is
 * src_offset = ((f*H + top)*W + left)*C, row_pitch = W*C, pixel_stride = C; a rectangle packed on its own [box_h][box_w][3] is
 * row_pitch = box_w*3, pixel_stride = 3.  Records may repeat (a hole re-reads another frame's rectangle): equal records give output
 * frames that are equal bit for bit. */
typedef struct vrg_crop_desc {
    int64_t src_offset;      /* floats from `in` to the rectangle's first value */
    int32_t row_pitch;       /* floats between rows of the rectangle */
    int32_t pixel_stride;    /* floats between pixels: the source's channel count (>= 3); the first three are read */
    int32_t box_w, box_h;    /* >= 1 */
    int32_t reserved[2];     /* 0 */
} vrg_crop_desc;

/* out = [n_out][size_h][size_w][3]; frame f = clamp(bicubic(rectangle of desc[f] -> size_h x size_w), 0, 1) in the arithmetic of
 * vrg_resize_f32 with the rectangle as the resampled view (taps clamped to the rectangle, not to the frame around it).  `desc`: device,
 * n_out records.  `in_floats`: the floats readable from `in`; a record whose rectangle does not lie inside them (or with a size < 1, a
 * pixel stride < 3, a negative offset or pitch) is never read: its frame is written as zeros.  The caller checks its table on the host. */
int vrg_crop_resize_f32(const float* in, int64_t in_floats, float* out, const vrg_crop_desc* desc, int64_t n_out,
                        int32_t size_h, int32_t size_w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The stand-alone enhancer's upscale: cv2.resize(frame, (out_w, out_h), interpolation=INTER_LANCZOS4) on decoded uint8 B,G,R frames
 * (VRGDG_StandaloneVideoEnhancerNodes.py:213-230), restated in csrc/vrg_lanczos_math.hpp: an 8 x 8-tap separable filter with 11-bit
 * integer weights, int32 sums, one rounding at the end -- integer arithmetic, the same bytes on every machine.
 *
 * vrg_lanczos4_taps fills, ON THE HOST, the table both kernels read: out_w column records then out_h row records of 20 bytes each
 * (int32 s = floor of the source coordinate, then the eight int16 weights of taps s - 3 .. s + 4).  The caller keeps one table per
 * geometry and uploads it; `taps` of the two launches below is that table in device memory, 4-byte aligned.
 *
 * vrg_lanczos4_u8: [frames][in_h][in_w][3] -> [frames][out_h][out_w][3], any sizes >= 1, any ratio (a downscale uses the same eight
 * taps, no antialiasing, as cv2 does), any alignment.  in != out; `in` is never written.
 *
 * vrg_upscale_sharpen_grain_u8 = vrg_sharpen_grain_u8(vrg_lanczos4_u8(in)) byte for byte, in one launch: the upscaled frame never goes
 * to memory.  strength <= 0 leaves the unsharp out, intensity <= 0 the grain (`noise` may then be null), as the two-launch route of the
 * Python layer does.  Borders and noise are those of the OUTPUT frame.  VRG_ERR_UNSUPPORTED (the caller runs the two entry points)
 * when an output tile of 34 rows needs more than 44 source rows (vertical ratios below about 0.9) or chunk_frames != 1. */
int vrg_lanczos4_taps(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, void* taps_host);
int vrg_lanczos4_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                    const void* taps, void* stream);
int vrg_upscale_sharpen_grain_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h,
                                 int32_t out_w, const void* taps, float strength, int32_t border, float intensity, float sat,
                                 float one_minus_sat, const vrg_noise_desc* noise, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The landmark-aligned Face Fix composite (VRGDGFaceFixCompositeLandmarkAligned.composite, VRGDG_StandaloneFaceFixNodes.py:1015-1054):
 * the work frame is bicubic-resized to the box and quantised to bytes, the bytes are warped with
 * cv2.warpAffine(..., INTER_LANCZOS4, BORDER_REFLECT101), divided by 255 and blended in under the opaque alpha.  The warp is cv2's
 * fixed-point affine remap, restated in csrc/vrg_warp_math.hpp: integer arithmetic, the same bytes on every machine.
 *
 * vrg_warp_phase_table fills, ON THE HOST, the 1024 x 8 x 8 int16 weights (131072 bytes, phase = fy * 32 + fx, then tap row, tap column)
 * that the two warping launches read from device memory; every phase sums to exactly 32768.
 * vrg_warp_record fills, ON THE HOST, the record of one warped frame from the forward 2 x 3 float transform, as warpAffine takes it, for
 * an out_w x out_h result read from a [src_h][src_w][3] byte image that starts src_offset bytes into the byte buffer.  It returns
 * VRG_ERR_BAD_ARG and clears the record when an entry is not finite or a fixed-point term leaves int32 for some pixel of the result (cv2
 * leaves both undefined).  A singular matrix follows cv2 (determinant 0 inverts to the zero matrix).
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_warp_desc {
    double m[6];          /* the INVERTED matrix (result -> source), as warpAffine forms it in double */
    int64_t src_offset;   /* bytes from the byte buffer to this frame's [src_h][src_w][3] image */
    int32_t src_w, src_h;
    int32_t set;          /* 0: no transform -- the composite takes the bicubic face, the stand-alone warp writes zeros */
    int32_t reserved;     /* 0 */
} vrg_warp_desc;

int vrg_warp_phase_table(void* table_host);
int vrg_warp_record(const float* transform, int32_t out_w, int32_t out_h, int32_t src_w, int32_t src_h, int64_t src_offset,
                    vrg_warp_desc* record_host);

/* Steps 1-2 of the node for every output frame of `desc` (device, the table of the composite) whose offsets[f] >= 0 (device, one int64
 * per frame: bytes from `generated` / `source` to that frame's [box_h][box_w][3] image): generated = uint8(clip(rint(clamp(bicubic(crop ->
 * box), 0, 1) * 255), 0, 255)) in the arithmetic of the composite, and -- when `source` is not NULL -- source = the same quantisation of
 * the unclamped original under the box.  A NaN gives byte 0.  An image that does not end inside `capacity` bytes, or whose record the
 * composite would not use, is not written.  max_box_pixels >= the largest box_w * box_h. */
int vrg_face_bytes_u8(const float* crops, const float* originals, const vrg_composite_desc* desc, const int64_t* offsets,
                      uint8_t* generated, uint8_t* source, int64_t capacity, int64_t max_box_pixels,
                      int64_t frames, int64_t original_frames, int64_t crop_frames,
                      int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                      void* stream);

/* The warp alone: out[f] = warpAffine(in + rec[f].src_offset, ..., (out_w, out_h), INTER_LANCZOS4, BORDER_REFLECT101) for `frames`
 * records (device).  `in_bytes`: the bytes readable from `in`; a record that is not set or whose image does not lie inside them gives a
 * frame of zeros.  `table`: device copy of vrg_warp_phase_table.  in != out; `in` is never written. */
int vrg_warp_affine_u8(const uint8_t* in, int64_t in_bytes, uint8_t* out, const vrg_warp_desc* rec, const void* table, int64_t frames,
                       int32_t out_h, int32_t out_w, void* stream);

/* vrg_composite_apply_f32 with a side table of `frames` warp records (device) parallel to `desc`: a frame whose record is set (and whose
 * image is box_w x box_h and lies inside `n_bytes`) takes fl(warped byte / 255) as its face, every other frame the bicubic face -- bit
 * for bit what vrg_composite_apply_f32 gives.  `bytes`: the packed images of vrg_face_bytes_u8. */
int vrg_composite_warp_apply_f32(const float* crops, const float* originals, const float* user_mask, const vrg_composite_desc* desc,
                                 const void* stats, const vrg_warp_desc* rec, const uint8_t* bytes, int64_t n_bytes, const void* table,
                                 float* out, float* mask_out,
                                 int64_t frames, int64_t original_frames, int64_t crop_frames, int64_t mask_frames,
                                 int32_t crop_h, int32_t crop_w, int32_t crop_channels, int32_t height, int32_t width, int32_t channels,
                                 int32_t mask_h, int32_t mask_w, int32_t mask_stride, int32_t match_channels, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The hard-cut score of the shot-aware Face Fix Prepare nodes (VRGDGFaceFixPrepareShotAware._cut_score,
 * VRGDG_StandaloneFaceFixNodes.py:421-435, with the quantisation of :456), restated in csrc/vrg_area_math.hpp: frames are quantised to
 * bytes, reduced to 64 x 64 thumbnails as cv2.resize(..., (64, 64), INTER_AREA) does for sides >= 64 (fp32 sums in cv2's order, or its
 * integer fast path when both ratios are integers), turned into 32 x 32 hue / saturation histograms (cvtColor's fixed-point RGB2HSV), and
 * every consecutive pair gives four exact integers from which the host finishes the score in double.
 *
 * vrg_area_taps fills, ON THE HOST, the table the thumbnail kernel reads: 64 column cells then 64 row cells of 20 bytes each (int32 first
 * source sample, int32 count, then the fp32 weights of the first, the middle and the last tap).  `taps` below is that table in device
 * memory, 4-byte aligned.
 *
 * vrg_cut_thumbs_f32: [frames][height][width][channels] fp32 -> [frames][64][64][3] bytes in one launch; height, width >= 64 (a smaller
 * side is VRG_ERR_BAD_ARG: cv2 takes another route there), channels 3 or 4 (the fourth is ignored), `in` 4-byte aligned and never written.
 * vrg_cut_hist_u8: [frames][64][64][3] bytes -> int32 [frames][1024] (bin = hue bin * 32 + saturation bin).
 * vrg_cut_pair_sums: int64 [frames - 1][4] = (sum |a - b| over the bytes, sum ha^2, sum hb^2, sum ha * hb) of thumbnails / histograms
 * (i, i + 1); fewer than two frames write nothing.
 * ------------------------------------------------------------------------------------------- */
int vrg_area_taps(int32_t in_h, int32_t in_w, void* taps_host);
int vrg_cut_thumbs_f32(const float* in, uint8_t* out, int64_t frames, int32_t height, int32_t width, int32_t channels, const void* taps,
                       void* stream);
int vrg_cut_hist_u8(const uint8_t* thumbs, int32_t* hist, int64_t frames, void* stream);
int vrg_cut_pair_sums(const uint8_t* thumbs, const int32_t* hist, int64_t* sums, int64_t frames, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The AI Video Builder's Face Fix (VRGDG_FaceFix.py of the reference: prepare_face_fix :473-476, finalize_face_fix :937-957) on decoded
 * uint8 B,G,R frames: square boxes resized with cv2's byte Lanczos-4 to the enhance size; and, on the way back, the repaired frame
 * resized to its box, colour matched by a mean shift over a soft ellipse and blended into a copy of the original.  Arithmetic:
 * csrc/vrg_facefix_math.hpp (and csrc/vrg_lanczos_math.hpp for the resize).
 *
 * HOST tables.  vrg_ff_ellipse_spans fills `height` records of two int32 (x0, x1: the filled pixels of the row, x0 > x1 = none) -- the
 * restated cv2.ellipse(..., -1) of _soft_ellipse_mask(width, height, .).  vrg_ff_gauss_coeffs fills the max(3, 4 * feather + 1) fp32
 * coefficients of its GaussianBlur (0 <= feather <= 256).  The Lanczos records are those of vrg_lanczos4_taps, one set of
 * out_w + out_h records per distinct (source size -> result size), concatenated by the caller; `n_taps` = records in the table.
 *
 * Every table and record below is device memory; a record that names anything outside the stated sizes, or a box that does not lie inside
 * the frame, is treated as "no box".
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_ff_box_desc {
    int32_t frame;                     /* frame of `in` the box is cut from */
    int32_t left, top, box_w, box_h;
    int32_t reserved;                  /* 0 */
    int64_t taps_offset;               /* records from `taps` to the out_w + out_h records of (box_h, box_w) -> (out_h, out_w) */
} vrg_ff_box_desc;

typedef struct vrg_ff_mask_desc {
    int32_t width, height;
    int64_t span_offset;               /* records from `spans` to this mask's `height` records */
    int64_t mask_offset;               /* floats from `masks` (and `scratch`) to this mask's [height][width] plane */
} vrg_ff_mask_desc;

typedef struct vrg_ff_desc {           /* one OUTPUT frame f: originals[f] with enhanced[enhanced_index] composited into the box */
    int32_t enhanced_index;
    int32_t left, top, box_w, box_h;
    float strength;                    /* composite_strength in (0, 1]; <= 0: the frame is copied */
    int64_t mask_offset;               /* floats from `masks` to the [box_h][box_w] mask */
    int64_t taps_offset;               /* records from `taps` to the box_w + box_h records of (enh_h, enh_w) -> (box_h, box_w) */
    int64_t bytes_offset;              /* bytes from `bytes` to this frame's [box_h][box_w][3] resized face */
} vrg_ff_desc;

int vrg_ff_ellipse_spans(int32_t width, int32_t height, int32_t* spans_host);
int vrg_ff_gauss_coeffs(int32_t feather, float* coeffs_host);

/* out[i] = cv2.resize(in[frame][top : top + box_h, left : left + box_w], (out_w, out_h), INTER_LANCZOS4) for n_out records, one launch:
 * taps clamp to the BOX (cv2 resizes a view).  A box of exactly the output size comes out as a copy of its bytes.  "No box" writes
 * zeros.  in != out; `in` ([in_frames][height][width][3]) is never written. */
int vrg_lanczos4_boxes_u8(const uint8_t* in, int64_t in_frames, int32_t height, int32_t width, uint8_t* out, const vrg_ff_box_desc* desc,
                          int64_t n_out, int32_t out_h, int32_t out_w, const void* taps, int64_t n_taps, void* stream);

/* The soft-ellipse masks of `n_masks` records, packed into `masks` (`mask_floats` floats; `scratch` of the same size holds the horizontal
 * planes): the 0 / 1 spans blurred horizontally, then vertically, with `n_coeffs` coefficients (BORDER_REFLECT_101), clipped to [0, 1].
 * n_coeffs == 0 (feather 0; `coeffs` and `scratch` may be NULL): the 0 / 1 spans.  max_mask_pixels >= the largest width * height. */
int vrg_ff_masks_f32(const int32_t* spans, int64_t n_spans, const float* coeffs, int32_t n_coeffs, const vrg_ff_mask_desc* desc,
                     int64_t n_masks, int64_t max_mask_pixels, float* scratch, float* masks, int64_t mask_floats, void* stream);

/* For every frame with a box and strength > 0: enhanced[enhanced_index] ([.][enh_h][enh_w][3]) resized to the box into `bytes`
 * (`capacity` bytes), and -- when color_match > 0 -- into stats[f] (12 uint64 per frame, zeroed here): [0] the count of mask > 0.35,
 * [1..3] the sums of the resized face's bytes there, [4..6] of the original's, exact integers; then [7] matched = count >= 16 and
 * [8..9] the three fp32 shifts fl(fl(original mean - face mean) * color_match) and a zero.  max_box_pixels >= the largest box. */
int vrg_ff_resize_stats_u8(const uint8_t* originals, const uint8_t* enhanced, const float* masks, int64_t mask_floats,
                           const vrg_ff_desc* desc, const void* taps, int64_t n_taps, uint8_t* bytes, int64_t capacity, void* stats,
                           int64_t frames, int64_t enhanced_frames, int32_t height, int32_t width, int32_t enh_h, int32_t enh_w,
                           int64_t max_box_pixels, float color_match, void* stream);

/* One pass over out = [frames][height][width][3]: the original's bytes outside the box (and everywhere for "no box" / strength <= 0);
 * inside, face' = matched ? trunc(clip(face + shift, 0, 255)) : face and
 * out = trunc(clip(fl(fl(original * fl(1 - a)) + fl(face' * a)), 0, 255)), a = fl(mask * strength).  out != originals, never written. */
int vrg_ff_composite_u8(const uint8_t* originals, const float* masks, int64_t mask_floats, const vrg_ff_desc* desc, const uint8_t* bytes,
                        int64_t capacity, const void* stats, uint8_t* out, int64_t frames, int32_t height, int32_t width, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same pixels for frames that live on the HOST (csrc/vrg_facefix_packed.hip): only the boxes cross the bus.  `src` is one buffer of
 * `src_bytes` bytes that holds each box's original bytes as a dense [box_h][box_w][3] block at its record's src_offset; the composite
 * writes each box's result as such a block at dst_offset of `out` (`out_bytes` bytes).  The masks, the Lanczos records, the byte scratch
 * and the statistics are those of the entry points above; `stats` holds 12 uint64 per RECORD.
 *
 * Grids are one-dimensional.  A workgroup of the statistics and composite launches is one tile of VRG_FF_PACKED_TILE box pixels; it
 * finds its record in `tile_prefix` (device, n + 1 int64, 8-byte aligned): tile_prefix[i] = the first tile of record i,
 * tile_prefix[n] = `tiles`, the grid.  vrg_lanczos4_packed_u8 writes out_h * out_w pixels for every record, so its workgroups divide.
 *
 * vrg_ff_packed_check refuses ON THE HOST (VRG_ERR_BAD_ARG) what the launches do not follow: a box below 1 x 1 or of 2^31 bytes or more,
 * a span (src, taps; and for the composite dst, mask, bytes) that leaves the stated sizes, an enhanced_index outside enhanced_frames,
 * a strength that is not > 0, a tile_prefix that is not the running sum of ceil(box_w * box_h / 256) from 0.  out_h, out_w >= 1: the
 * records of vrg_lanczos4_packed_u8 (taps: out_w + out_h records; tile_prefix may be NULL; dst, mask, bytes, strength, enhanced_index
 * are not read).  out_h == out_w == 0: the records of the other two (taps: box_w + box_h records).  n == 0 is fine.
 * On the device a record that fails these checks writes zeros (vrg_lanczos4_packed_u8), is skipped (statistics), or -- where its src
 * and dst blocks lie inside the buffers -- comes out as a copy of its original bytes (composite; otherwise nothing is written).
 * ------------------------------------------------------------------------------------------- */
#define VRG_FF_PACKED_TILE 256

typedef struct vrg_ff_packed_desc {
    int64_t src_offset;                /* bytes from `src` to the box's [box_h][box_w][3] original bytes */
    int64_t dst_offset;                /* bytes from `out` of the composite to the box's [box_h][box_w][3] result */
    int32_t box_w, box_h;
    int32_t enhanced_index;
    float strength;                    /* composite_strength in (0, 1] */
    int64_t mask_offset;               /* floats from `masks` to the [box_h][box_w] mask */
    int64_t taps_offset;               /* records from `taps`: (box_h, box_w) -> (out_h, out_w), or (enh_h, enh_w) -> (box_h, box_w) */
    int64_t bytes_offset;              /* bytes from `bytes` to this record's [box_h][box_w][3] resized face */
} vrg_ff_packed_desc;

int vrg_ff_packed_check(const vrg_ff_packed_desc* desc_host, int64_t n, const int64_t* tile_prefix_host, int64_t src_bytes, int64_t out_bytes,
                        int64_t enhanced_frames, int64_t mask_floats, int64_t n_taps, int64_t capacity, int32_t out_h, int32_t out_w);

/* out[i] = cv2.resize(box i, (out_w, out_h), INTER_LANCZOS4) for n records ([n][out_h][out_w][3]), one launch; taps clamp to the box. */
int vrg_lanczos4_packed_u8(const uint8_t* src, int64_t src_bytes, const vrg_ff_packed_desc* desc, int64_t n, uint8_t* out, int32_t out_h,
                           int32_t out_w, const void* taps, int64_t n_taps, void* stream);

/* enhanced[enhanced_index] ([enhanced_frames][enh_h][enh_w][3]) resized to the box into `bytes`, and -- when color_match > 0 -- stats[i]
 * in the layout of vrg_ff_resize_stats_u8 (zeroed here; the means and shifts are finished on the device). */
int vrg_ff_packed_resize_stats_u8(const uint8_t* src, int64_t src_bytes, const uint8_t* enhanced, int64_t enhanced_frames, int32_t enh_h,
                                  int32_t enh_w, const float* masks, int64_t mask_floats, const vrg_ff_packed_desc* desc,
                                  const int64_t* tile_prefix, int64_t n, int64_t tiles, const void* taps, int64_t n_taps, uint8_t* bytes,
                                  int64_t capacity, void* stats, float color_match, void* stream);

/* out[dst_offset ..] = the composite of vrg_ff_composite_u8 inside the box, for every record.  out != src, which is never written. */
int vrg_ff_packed_composite_u8(const uint8_t* src, int64_t src_bytes, const float* masks, int64_t mask_floats, const vrg_ff_packed_desc* desc,
                               const int64_t* tile_prefix, int64_t n, int64_t tiles, const uint8_t* bytes, int64_t capacity, const void* stats,
                               uint8_t* out, int64_t out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The input of the Face Fix face detector (`_detect_with_rotation` / `_detect`, VRGDG_StandaloneFaceFixNodes.py:95-185 and
 * VRGDG_FaceFix.py:67-157 of the reference), restated in csrc/vrg_detect_math.hpp: frames quantised to B,G,R bytes, rotated about the frame
 * centre (cv2.warpAffine, INTER_LINEAR, BORDER_REPLICATE, the classic fixed-point path), cut into regions, each resized to 300 x 300
 * (cv2.resize, INTER_LINEAR on bytes) and made a blob (fp32 [3][300][300], byte - (104, 177, 123)).  The network itself is not here.
 *
 * Frames are [n_frames][height][width][channels >= 3] fp32 R,G,B (channels beyond 3 are ignored) or [n_frames][height][width][3] uint8
 * B,G,R; height, width <= 32767.  `transforms`: n_transforms x 6 doubles (device, 8-byte aligned), each the INVERTED 2 x 3 matrix
 * (result -> source) as warpAffine forms it in double; the host makes them (trigonometry in libm).  Descriptors are device memory; one
 * that names a frame, a transform or a region outside what the call states writes zeros.  vrg_detect_check refuses such descriptors ON
 * THE HOST (VRG_ERR_BAD_ARG): a region must lie inside the frame with both sides >= 8.  n_blobs / n_out == 0 succeeds without a launch.
 * Frames are never written.
 *
 * vrg_linear_taps fills, ON THE HOST, the tables of one axis of cv2.resize(INTER_LINEAR, 8U) from n_in to n_out samples: ofs = 2 * n_out
 * int32, coef = 4 * n_out int16.  First the horizontal rule (ofs[d] = s in 0 .. n_in - 1, coef[2d], coef[2d + 1] the weights of S[s] and
 * S[s + 1]), then, n_out entries on, the vertical rule (ofs = floor(f), which may be -1 or n_in - 1: the two rows are clamped).
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_detect_desc {       /* one blob */
    int32_t frame;
    int32_t transform;                 /* index into `transforms`, -1: the frame as it is */
    int32_t left, top, right, bottom;  /* the region of the (rotated) frame */
} vrg_detect_desc;

typedef struct vrg_detect_frame_desc { /* one rotated frame */
    int32_t frame;
    int32_t transform;                 /* -1: the quantised B,G,R frame itself */
} vrg_detect_frame_desc;

int vrg_linear_taps(int32_t n_in, int32_t n_out, int32_t* ofs_host, int16_t* coef_host);
int vrg_detect_check(const vrg_detect_desc* desc_host, int64_t n_desc, int64_t n_frames, int32_t height, int32_t width,
                     int64_t n_transforms);

/* out[i] = blob(resize(warp(frame)[top:bottom, left:right], (300, 300))) for n_blobs descriptors in ONE launch: fp32
 * [n_blobs][3][300][300].  The rotated frame is never written: a value reads 4 source pixels without a transform, 16 with one. */
int vrg_detect_blobs_f32(const float* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels, const double* transforms,
                         int64_t n_transforms, const vrg_detect_desc* desc, int64_t n_blobs, float* out, void* stream);
int vrg_detect_blobs_u8(const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, const double* transforms,
                        int64_t n_transforms, const vrg_detect_desc* desc, int64_t n_blobs, float* out, void* stream);

/* The rotated B,G,R byte frames themselves, [n_out][height][width][3] (what the YuNet branch hands its detector).  f32_channels == 0:
 * `frames` are uint8 B,G,R; >= 3: fp32 R,G,B with that many channels.  16-byte stores where a frame of `out` starts on a 16-byte
 * boundary. */
int vrg_warp_linear_u8(const void* frames, int32_t f32_channels, int64_t n_frames, int32_t height, int32_t width, const double* transforms,
                       int64_t n_transforms, const vrg_detect_frame_desc* desc, int64_t n_out, uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Introspection
 * ------------------------------------------------------------------------------------------- */
int vrg_abi_version(void);
const char* vrg_error_string(int status);
/* multiProcessorCount and maxThreadsPerMultiProcessor of the current device (what torch's
 * calc_execution_policy reads); returns VRG_ERR_NO_DEVICE without a GPU. */
int vrg_device_info(int32_t* cu_count, int32_t* max_threads_per_cu);
/* HIP-event timing helper for bench.py: records an event on `stream` and returns elapsed ms
 * between two recorded events (torch.cuda.Event only sees torch's current stream). */
int vrg_event_create(void** ev);
int vrg_event_record(void* ev, void* stream);
int vrg_event_elapsed_ms(void* start, void* stop, float* ms);
int vrg_event_destroy(void* ev);

/* Raw N(0,1) stream of the given chunks, bit-identical to torch.randn on this device; `frame_elems` = H*W*3.  The node layer materialises the
 * noise of an RNG chunk of more than 2^29 elements with it, leaf by leaf as ATen splits such a randn (reference: nodes.py:51 with batch_size 0
 * or >= 22 4K frames), and the tests compare the stream itself against torch. */
int vrg_noise_f32(float* out, int64_t frames, int64_t frame_elems,
                  const vrg_noise_desc* noise, void* stream);

/* First-use self-check of the one toolchain-calibrated arithmetic form of the colour match (csrc/vrg_pixel_math.hpp dev_pow_ziv: table
 * logarithm + rounding test whose half-widths were measured against ROCm 7.0's ocml): out[i] = the power of in[i] exactly as call site
 * `site` of the Lab transforms evaluates it -- 0: sRGB -> linear (x^2.4 on [0.0625, 2]), 1: linear -> sRGB (x^(1/2.4) on [0.0031308, 4]),
 * 2: the Lab cube root (x^(1/3) on [0.008856, 4]).  The host compares with this ROCm's powf (torch.pow, which the reference's kornia calls:
 * nodes.py:98, 115) and reports a mismatch (ops.toolchain_status). */
int vrg_selfcheck_pow_f32(const float* in, float* out, int64_t n, int32_t site, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Far-face repair composite on decoded bytes (reference: scripts/far_face_repair_backend.py composite :339-371): every repaired crop
 * resized to its box with Pillow's LANCZOS, a soft-ellipse mask (ImageDraw.ellipse + GaussianBlur), an optional mean shift with numpy's
 * sequential fp32 means, and Image.paste under the mask into a copy of the frame.  Arithmetic: csrc/vrg_pil_math.hpp, pinned byte for
 * byte against Pillow itself.
 *
 * HOST tables.  vrg_pil_lanczos_ksize gives the taps per output index of one axis `n_in` -> `n_out` (0: a size below 1);
 * vrg_pil_lanczos_table fills bounds[n_out][2] (first source index, tap count) and weights[n_out][ksize] (22-bit fixed point, zero beyond
 * the count); it is vrg_pil_filter_table with filter 1 over the whole axis, with no float in between: exact for every n_in.  On the
 * device one axis table is these two arrays back to back: n_out * (2 + ksize) int32.  vrg_pil_box_parameters fills
 * out[3] = radius, ww, fw (the last two uint32) of one box pass of GaussianBlur(radius = sigma), 0 < sigma <= 4096.
 *
 * Every table and record below is device memory; a record that names anything outside the stated sizes, or a box that does not lie inside
 * the frame, is treated as "no box" / "no image".
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_pil_resize_desc {   /* one OUTPUT image: src[in_h][in_w][C] -> dst[out_h][out_w][C] */
    int64_t src_offset, dst_offset;    /* bytes from `src` / `dst` */
    int64_t tmp_offset;                /* bytes from `tmp` to the [in_h][out_w][C] image of the horizontal pass (read when both passes run) */
    int64_t h_table, v_table;          /* int32 from `tables` to the axis table in_w -> out_w / in_h -> out_h (read when the sizes differ) */
    int32_t in_w, in_h, out_w, out_h;
    int32_t h_ksize, v_ksize;
} vrg_pil_resize_desc;

typedef struct vrg_pil_mask_desc {
    int32_t width, height;             /* each at most 8192 */
    int32_t radius;                    /* of a box pass; < 0: no blur, the mask is the 0 / 255 spans */
    uint32_t ww, fw;
    int32_t reserved;                  /* 0 */
    int64_t span_offset;               /* records (two int32: first and last set column) from `spans` to this mask's `height` rows */
    int64_t mask_offset;               /* bytes from `masks` (and `scratch`) to this mask's [height][width] plane */
} vrg_pil_mask_desc;

typedef struct vrg_pil_box_desc {      /* one OUTPUT frame f */
    int32_t left, top, box_w, box_h;   /* box_w < 1: no box, the frame is copied */
    int32_t color_match;               /* != 0: the mean shift of color_match_repaired */
    int32_t reserved;                  /* 0 */
    int64_t mask_offset;               /* bytes from `masks` to the [box_h][box_w] mask */
    int64_t rep_offset;                /* bytes from `repaired` to the [box_h][box_w][3] resized crop */
} vrg_pil_box_desc;

int32_t vrg_pil_lanczos_ksize(int32_t n_in, int32_t n_out);
int vrg_pil_lanczos_table(int32_t n_in, int32_t n_out, int32_t* bounds_host, int32_t* weights_host);
int vrg_pil_box_parameters(float sigma, int32_t* out_host);

/* dst image i = Image.resize((out_w, out_h), LANCZOS) of src image i for n_out records (sources of any sizes, packed in `src`), channels =
 * 3 (RGB) or 1 (L): the horizontal byte pass into `tmp`, then the vertical one; a pass whose size does not change is skipped, both: a copy.
 * max_pixels >= the largest in_h * out_w and out_h * out_w.  `src` is never written; src, tmp and dst are distinct. */
int vrg_pil_resize_u8(const uint8_t* src, int64_t src_bytes, const vrg_pil_resize_desc* desc, int64_t n_out, int32_t channels,
                      const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes, uint8_t* dst, int64_t dst_bytes,
                      int64_t max_pixels, void* stream);

/* The masks of `n_masks` records, packed into `masks` (`mask_bytes` bytes; `scratch` of the same size holds the row passes): the 0 / 255
 * spans through three box passes along the rows, then three along the columns, each rounded to bytes, from integer prefix sums.
 * max_width / max_height >= the largest of the records. */
int vrg_pil_mask_u8(const int32_t* spans, int64_t n_spans, const vrg_pil_mask_desc* desc, int64_t n_masks, int32_t max_width,
                    int32_t max_height, uint8_t* scratch, uint8_t* masks, int64_t mask_bytes, void* stream);

/* stats[f] (12 uint32 per frame) for every frame with a box and color_match != 0 (all zero otherwise): [0] the count of mask >= 64,
 * [1..3] numpy's fp32 means of the original's box there (the sequential fp32 sum in row-major order / the count), [4..6] those of the
 * resized crop, [7..9] the shifts fl(fl(original mean - crop mean) * strength), [10] matched = count >= 16, [11] 0; fp32 as bit patterns. */
int vrg_np_masked_means_f32(const uint8_t* originals, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks, int64_t mask_bytes,
                            const vrg_pil_box_desc* desc, uint32_t* stats, int64_t frames, int32_t height, int32_t width, float strength,
                            void* stream);

/* One pass over out = [frames][height][width][3]: the original's bytes outside the box (and everywhere for "no box"); inside,
 * r' = matched ? trunc(clip(fl(r + shift), 0, 255)) : r and t = o (255 - m) + r' m + 128, out = ((t >> 8) + t) >> 8.  out != originals,
 * which is never written. */
int vrg_pil_paste_u8(const uint8_t* originals, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks, int64_t mask_bytes,
                     const vrg_pil_box_desc* desc, const uint32_t* stats, uint8_t* out, int64_t frames, int32_t height, int32_t width,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same composite for frames that live on the HOST (csrc/vrg_farface_packed.hip): only the boxes cross the bus.  `src` is one buffer
 * of `src_bytes` bytes that holds each box's original bytes as a dense [box_h][box_w][3] block at its record's src_offset; the paste
 * writes each box's result as such a block at dst_offset of `out` (`out_bytes` bytes).  `repaired` and `masks` are the packed outputs of
 * vrg_pil_resize_u8 / vrg_pil_mask_u8 above, `stats` holds 12 uint32 per RECORD, laid out as vrg_np_masked_means_f32 writes them.
 *
 * Grids are one-dimensional.  The means are one workgroup per record.  A workgroup of the paste is one tile of VRG_PIL_PACKED_TILE box
 * pixels; it finds its record in `tile_prefix` (device, n + 1 int64, 8-byte aligned): tile_prefix[i] = the first tile of record i,
 * tile_prefix[n] = `tiles`, the grid (workgroups past the last tile do nothing; tiles > 2^31 - 1: VRG_ERR_UNSUPPORTED).
 *
 * vrg_pil_packed_check refuses ON THE HOST (VRG_ERR_BAD_ARG) what the launches do not follow: a box below 1 x 1 or of 2^31 bytes or
 * more, a span (src, dst, rep, mask) that leaves the stated sizes, a tile_prefix that is not the running sum of
 * ceil(box_w * box_h / VRG_PIL_PACKED_TILE) from 0.  n == 0 is fine.  On the device a record that fails these checks gets a zero
 * statistics record; the paste writes a copy of its original bytes where its src and dst blocks lie inside the buffers and nothing
 * otherwise.
 * ------------------------------------------------------------------------------------------- */
#define VRG_PIL_PACKED_TILE 256

typedef struct vrg_pil_packed_desc {
    int64_t src_offset;                /* bytes from `src` to the box's [box_h][box_w][3] original bytes */
    int64_t dst_offset;                /* bytes from `out` of the paste to the box's [box_h][box_w][3] result */
    int32_t box_w, box_h;
    int32_t color_match;               /* != 0: the mean shift of color_match_repaired */
    int32_t reserved;                  /* 0 */
    int64_t mask_offset;               /* bytes from `masks` to the [box_h][box_w] mask */
    int64_t rep_offset;                /* bytes from `repaired` to the [box_h][box_w][3] resized crop */
} vrg_pil_packed_desc;

int vrg_pil_packed_check(const vrg_pil_packed_desc* desc_host, int64_t n, const int64_t* tile_prefix_host, int64_t src_bytes,
                         int64_t rep_bytes, int64_t mask_bytes, int64_t out_bytes);

/* stats[i] of vrg_np_masked_means_f32 for record i: the same sequential fp32 means, the box's pixel p read at src_offset + 3 p. */
int vrg_np_packed_masked_means_f32(const uint8_t* src, int64_t src_bytes, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks,
                                   int64_t mask_bytes, const vrg_pil_packed_desc* desc, uint32_t* stats, int64_t n, float strength,
                                   void* stream);

/* out[dst_offset ..] = the paste of vrg_pil_paste_u8 inside the box, for every record.  out != src, which is never written. */
int vrg_pil_packed_paste_u8(const uint8_t* src, int64_t src_bytes, const uint8_t* repaired, int64_t rep_bytes, const uint8_t* masks,
                            int64_t mask_bytes, const vrg_pil_packed_desc* desc, const int64_t* tile_prefix, int64_t n, int64_t tiles,
                            const uint32_t* stats, uint8_t* out, int64_t out_bytes, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Host side of the node path (reference: nodes.py:50, 61-66 -- CPU tensors in, `images.to(device)` per batch)
 * ------------------------------------------------------------------------------------------- */
/* memcpy of `bytes` from `src` to `dst` (host pointers, not overlapping) split over `threads` host threads (0 = 8; at most 64; parts of
 * whole pages, none below 2 MiB).  The node layer stages pageable frames into a page-locked ring with it, so that upload, kernels and
 * download of a pageable batch overlap like those of a page-locked one.  Blocks until the bytes are there.  No device work. */
int vrg_host_copy(void* dst, const void* src, int64_t bytes, int32_t threads);

/* ---------------------------------------------------------------------------------------------
 * The Video Folder Grid Plot (VRGDG_VideoFolderGridPlot, LTXLoraTrain.py:7926-8314 of the reference), restated in csrc/vrg_grid_math.hpp:
 * every tile of every output frame is quantised (np.clip(x * 255.0, 0, 255).astype(uint8): truncation; NaN gives 0), resized to
 * new_w x new_h as cv2.resize(..., INTER_AREA) does on bytes -- unchanged, its integer fast paths, its general fp32 area sums, or its
 * fixed-point bilinear rule with area-mode coefficients when an axis enlarges -- and written as (float)byte / 255.0f into the grid frame
 * [frames][grid_h][grid_w][3] at (dst_y + y_off, dst_x + x_off); the first `band` rows of the tile take the overlay's bytes / 255, every
 * other float of the cell_w x cell_h tile is 0.  One descriptor per (output frame, tile), empty cells included (src null): the launch writes
 * every float of every tile it is given exactly once and reads no float of the grid.  Sources are never written.
 *
 * vrg_grid_plan gives, ON THE HOST, the rule (enum vrg_grid_mode) a resize of in_w x in_h to out_w x out_h takes, 1.0f / (sx * sy) of the
 * fast rules and `cps`, the columns a wave stages at a time; VRG_ERR_UNSUPPORTED when the taps of one column pass the staging buffer.
 * vrg_grid_taps fills, ON THE HOST, the n_out records of 20 bytes of one axis in one mode (int32 first sample, int32 count, three fp32:
 * the weights of the first, the middle and the last tap; for VRG_GRID_LINEAR count is 1 or 2 and the first and the last hold the two
 * integer coefficients 0 .. 2048).  A mode the pair (n_in, n_out) cannot take is VRG_ERR_BAD_ARG.
 * vrg_grid_check refuses ON THE HOST (VRG_ERR_BAD_ARG) descriptors that name a frame or a tile outside the grid, a picture outside the
 * tile or above the band, a mode other than vrg_grid_plan's, or a source of more than 2^31 - 1 values; the kernel writes nothing for a
 * tile outside the grid and no picture for one outside its tile.
 * vrg_grid_tiles_f32: sources are [height][width][channels] fp32 R,G,B frames, channels 3 or 4 (the fourth ignored), 4-byte aligned.
 * vrg_grid_tiles_u8: sources are [height][width][3] decoded B,G,R byte frames (their own quantisation); the grid is R,G,B.
 * `desc`, the tables and the overlays ([band][cell_w][3] bytes R,G,B) are device memory; n_desc == 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------------- */
enum vrg_grid_mode { VRG_GRID_COPY = 0, VRG_GRID_FAST = 1, VRG_GRID_FAST_2X2 = 2, VRG_GRID_GENERAL = 3, VRG_GRID_LINEAR = 4 };

typedef struct vrg_grid_desc {         /* one tile of one output frame */
    const void* src;                   /* the source frame, or null: no picture */
    const void* xtab;                  /* new_w records of vrg_grid_taps(width, new_w, mode) */
    const void* ytab;                  /* new_h records of vrg_grid_taps(height, new_h, mode) */
    const uint8_t* overlay;            /* the label band, or null */
    int32_t height, width, channels, mode;
    int32_t frame;                     /* the output frame */
    int32_t dst_x, dst_y;              /* the tile's origin in the grid frame */
    int32_t new_w, new_h, x_off, y_off;
    int32_t band;                      /* rows of the overlay */
    int32_t cps;                       /* vrg_grid_plan */
    float inv;                         /* vrg_grid_plan */
} vrg_grid_desc;

int vrg_grid_plan(int32_t in_h, int32_t in_w, int32_t channels, int32_t out_h, int32_t out_w, int32_t* mode, int32_t* cps, float* inv);
int vrg_grid_taps(int32_t n_in, int32_t n_out, int32_t mode, void* taps_host);
int vrg_grid_check(const vrg_grid_desc* desc_host, int64_t n_desc, int32_t bytes, int64_t frames, int32_t cell_w, int32_t cell_h,
                   int32_t grid_w, int32_t grid_h);
int vrg_grid_tiles_f32(const vrg_grid_desc* desc, int64_t n_desc, float* out, int64_t frames, int32_t cell_w, int32_t cell_h,
                       int32_t grid_w, int32_t grid_h, void* stream);
int vrg_grid_tiles_u8(const vrg_grid_desc* desc, int64_t n_desc, float* out, int64_t frames, int32_t cell_w, int32_t cell_h,
                      int32_t grid_w, int32_t grid_h, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The input of the landmark estimator (VRGDGFaceFixCompositeLandmarkAligned._landmarks, VRGDG_StandaloneFaceFixNodes.py:955-979 of the
 * reference): cv2.cvtColor(cv2.resize(rgb, (320, 320), interpolation=cv2.INTER_AREA), COLOR_RGB2BGR) of the packed byte images
 * vrg_face_bytes_u8 writes, for a list of descriptors in one launch.  out = [n_desc][320][320][3] bytes B,G,R, 16-byte aligned: channel c
 * is channel 2 - c of the resize, which takes the rule, the tables and the arithmetic of the grid plot above
 * (vrg_grid_plan(box_h, box_w, 3, 320, 320, ...), vrg_grid_taps(box_w | box_h, 320, mode)).  Every byte of every thumbnail is written
 * exactly once, nothing else is, and the images are never written.
 *
 * vrg_face_thumbs_check refuses ON THE HOST (VRG_ERR_BAD_ARG) a side below 1 or above 32767, a `which` outside {0, 1}, which == 1 without
 * a source buffer (has_source == 0), an image that does not end inside n_bytes, a mode, cps or inv other than vrg_grid_plan's and a null
 * table.  vrg_face_thumbs_u8: `desc` and the tables are device memory; n_desc == 0 succeeds without a launch; a null or misaligned out
 * and an out that is one of the inputs are argument errors; the kernel writes nothing for a descriptor whose image does not lie inside
 * n_bytes (or that names a buffer that is not there).
 * ------------------------------------------------------------------------------------------- */
#define VRG_THUMB_SIDE 320
#define VRG_THUMB_MAX_SIDE 32767

typedef struct vrg_thumb_desc {        /* one thumbnail */
    const void* xtab;                  /* 320 records of vrg_grid_taps(box_w, 320, mode) */
    const void* ytab;                  /* 320 records of vrg_grid_taps(box_h, 320, mode) */
    int64_t offset;                    /* bytes from `generated` / `source` to the [box_h][box_w][3] R,G,B image, any alignment */
    int32_t which;                     /* 0: generated, 1: source */
    int32_t box_w, box_h;
    int32_t mode;                      /* enum vrg_grid_mode, vrg_grid_plan */
    int32_t cps;                       /* vrg_grid_plan */
    float inv;                         /* vrg_grid_plan */
} vrg_thumb_desc;

int vrg_face_thumbs_check(const vrg_thumb_desc* desc_host, int64_t n_desc, int64_t n_bytes, int has_source);
int vrg_face_thumbs_u8(const uint8_t* generated, const uint8_t* source, int64_t n_bytes, const vrg_thumb_desc* desc, int64_t n_desc,
                       uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference sheets (VRGDG_LTXICIngredientsGrid.build, VRGDG_LTXICIngredientsGrid.py of the reference, and the three sheet builders of
 * VRGDG_MusicVideoBuilderNodes.py:7169-7238), restated in csrc/vrg_sheet_math.hpp: every panel's source quantised
 * (np.clip(x * 255.0, 0, 255).astype(uint8): truncation; NaN gives 0), resized as Image.resize((new_w, new_h), LANCZOS) does on bytes
 * (csrc/vrg_pil_math.hpp), cropped (cover_crop) or centred on the cell colour (contain_pad), and pasted in order onto a canvas of one
 * colour, under the 0 / 255 mask of ImageDraw.rounded_rectangle where the panel has one.  Two launches:
 *   vrg_sheet_rows_*     per panel, the horizontal pass over the source rows and the columns the kept window needs, into
 *                        tmp + tmp_offset as [rows][pic_w][3] bytes (the quantised window itself where src_w == new_w).  `_f32`: sources
 *                        are [src_h][src_w][channels] fp32 R,G,B, 4-byte aligned; `_u8`: the same as bytes.  channels == 1 is repeated,
 *                        channels > 3 gives its first three.  Grid: max_segments x ceil(max_rows / 4) x n workgroups, max_segments >=
 *                        ceil(pic_w / cps) and max_rows >= rows of every record.  Sources are never written.
 *   vrg_sheet_compose_*  one pass over the canvas out[height][width][3]: every element is written exactly once and none is read.  For a
 *                        pixel the LAST record whose rectangle (left, top, w, h) and mask span cover it decides: the vertical pass over
 *                        tmp inside the window, the cell colour around it; no record: `background` (R | G << 8 | B << 16).  `_f32`
 *                        writes (float)byte / 255.0f, `_u8` the byte.  Rectangles may leave the canvas.
 * Tables: one axis table is vrg_pil_lanczos_table's bounds and weights back to back, n_out * (2 + ksize) int32, at h_table / v_table in
 * `tables` (ignored for an axis whose size does not change).  Spans: [n_spans][2] int32, first and last covered column of a panel row
 * (first > last: none); span_offset == -1: no mask.  All of `panels`, `tables`, `spans`, `tmp` and the sources are device memory.
 *
 * HOST helpers.  vrg_sheet_fit gives the eight integers new_w, new_h, win_x, win_y, pic_w, pic_h, pic_x, pic_y of _resize_to_panel for a
 * source of src_w x src_h in a panel of w x h.  vrg_sheet_plan fills row0, rows and cps of records whose other fields are set, from a
 * host copy of `tables`; VRG_ERR_UNSUPPORTED when the taps of ONE window column span more than VRG_SHEET_STAGE_VALUES source values
 * (pixels x channels).  vrg_sheet_check refuses (VRG_ERR_BAD_ARG) a null source, channels outside {1, 3, 4, ...}, tables that are not
 * vrg_pil_lanczos_table's for the stated sizes, a window outside the resized picture or the panel, row0 / rows / cps other than
 * vrg_sheet_plan's, a mask or a temp image outside its buffer, and (VRG_ERR_UNSUPPORTED) a side above VRG_SHEET_MAX_SIDE.  The kernels
 * follow no record that fails the checks which need no table; such a record pastes nothing.
 * n == 0 succeeds without a launch.  A null or misaligned `out` (4 bytes for _f32) and an `out` that is `tmp`, `tables`, `spans` or
 * `panels` are argument errors; so is a canvas side below 1 (above VRG_SHEET_MAX_SIDE: VRG_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
#define VRG_SHEET_MAX_SIDE 32767
#define VRG_SHEET_STAGE_VALUES 16384

typedef struct vrg_sheet_panel {       /* one pasted picture */
    const void* src;                   /* the source frame */
    int64_t h_table, v_table;          /* int32 offsets into `tables` */
    int64_t span_offset;               /* rows into `spans` of the panel's h mask rows, or -1 */
    int64_t tmp_offset;                /* bytes into `tmp` */
    int32_t src_h, src_w, channels;
    int32_t new_w, new_h;              /* the resized picture */
    int32_t h_ksize, v_ksize;          /* vrg_pil_lanczos_ksize per axis */
    int32_t win_x, win_y;              /* the kept window's origin in the resized picture */
    int32_t pic_w, pic_h;              /* the window's size */
    int32_t row0, rows;                /* the rows of tmp: source rows (window rows where src_h == new_h); vrg_sheet_plan */
    int32_t left, top, w, h;           /* the panel on the canvas */
    int32_t pic_x, pic_y;              /* the window's origin inside the panel */
    int32_t cps;                       /* window columns per staged segment; vrg_sheet_plan */
    uint8_t cell[4];                   /* the cell colour R, G, B, 0 */
    int32_t reserved;
} vrg_sheet_panel;

int vrg_sheet_fit(int32_t src_w, int32_t src_h, int32_t w, int32_t h, int32_t cover, int32_t* fit_host);
int vrg_sheet_plan(vrg_sheet_panel* panels_host, int64_t n, const int32_t* tables_host, int64_t table_ints);
int vrg_sheet_check(const vrg_sheet_panel* panels_host, int64_t n, int32_t bytes, const int32_t* tables_host, int64_t table_ints,
                    int64_t n_spans, int64_t tmp_bytes);
int vrg_sheet_rows_f32(const vrg_sheet_panel* panels, int64_t n, const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes,
                       int32_t max_segments, int32_t max_rows, void* stream);
int vrg_sheet_rows_u8(const vrg_sheet_panel* panels, int64_t n, const int32_t* tables, int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes,
                      int32_t max_segments, int32_t max_rows, void* stream);
int vrg_sheet_compose_f32(const vrg_sheet_panel* panels, int64_t n, int32_t bytes, const int32_t* tables, int64_t table_ints,
                          const int32_t* spans, int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, float* out, int32_t width,
                          int32_t height, uint32_t background, void* stream);
int vrg_sheet_compose_u8(const vrg_sheet_panel* panels, int64_t n, int32_t bytes, const int32_t* tables, int64_t table_ints,
                         const int32_t* spans, int64_t n_spans, const uint8_t* tmp, int64_t tmp_bytes, uint8_t* out, int32_t width,
                         int32_t height, uint32_t background, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The far-face repair contact sheet (contact_sheet of scripts/far_face_repair_backend.py:374-408 of the reference): per entry the
 * original and the fixed frame side by side, shrunk by Image.thumbnail -- Image.reduce by integer factors, then a BICUBIC (or LANCZOS)
 * resize over the fractional source box -- and pasted into the cells of a sheet.  Arithmetic: csrc/vrg_pil_math.hpp, pinned byte for byte
 * to the installed Pillow.  Two launches (csrc/vrg_thumb.hip):
 *   vrg_thumb_rows_u8     per entry, the pair (never stored), the reduce (never stored) and the horizontal pass into tmp + tmp_offset as
 *                         [red_h][out_w][3] bytes.  The left half is src + left_offset as [left_h][left_w][3]; the right half is
 *                         src + right_offset as [right_h][right_w][3] pasted at (left_w, 0) onto black and clipped to left_w x left_h;
 *                         right_offset == -1: a single picture, no pair.  A workgroup reads fy source rows of a segment of `cps` output
 *                         columns once.  Grid: max_segments x max_rows x n, max_segments >= ceil(out_w / cps), max_rows >= red_h.
 *                         Sources are never written and may lie at any byte address.
 *   vrg_thumb_compose_u8  one pass over out[height][width][3]: every byte is written once and none is read.  Entry i owns the cell
 *                         (i % columns, i / columns) of cell_w x cell_h; inside its thumbnail at (dst_x, dst_y) the byte is the vertical
 *                         pass over tmp, everywhere else `background` (R | G << 8 | B << 16).
 * Tables: one axis table is vrg_pil_filter_table's bounds and weights back to back, n_out * (2 + ksize) int32, at h_table / v_table in
 * `tables`; h_ksize / v_ksize == 0: the axis is copied (out == red and the box is the whole axis).
 *
 * HOST helpers.  vrg_pil_filter_ksize / vrg_pil_filter_table: one axis of Image.resize(size, filter, box) -- filter 3 = BICUBIC,
 * 1 = LANCZOS, the source interval [in0, in1) given as the C floats Pillow receives, 0 <= in0 <= in1 <= n_in; with the box (0, n_in) and
 * LANCZOS they equal vrg_pil_lanczos_*.  vrg_pil_reduce_host: Image.reduce((fx, fy)) of a whole host picture.
 * vrg_thumb_plan fills, from left_w, left_h, right_offset (>= 0: a pair) of every entry and the size requested of Image.thumbnail
 * (req_host[i] = {width, height} as given, >= 1), fx, fy, red_w, red_h, out_w, out_h, h_ksize, v_ksize, cps, tmp_offset, dst_x, dst_y --
 * reducing_gap <= 0 stands for None, else it must be >= 1 -- and sheet_host = {columns, rows, cell_w, cell_h, bytes of tmp}.
 * VRG_ERR_UNSUPPORTED -- before any launch, nothing is truncated -- for a factor above VRG_THUMB_MAX_FACTOR, a side above
 * VRG_THUMB_MAX_SOURCE, taps of one output column that pass the staging buffer (VRG_THUMB_STAGE_BYTES source bytes of one row,
 * VRG_THUMB_STAGE_VALUES reduced values), and a reduced picture more than 100 times as tall as wide (Pillow resizes it vertically first).
 * vrg_thumb_plan_reduce plans Image.reduce((fx, fy)) alone in the same way: the reduced picture is the thumbnail, no table.
 * vrg_thumb_check refuses (VRG_ERR_BAD_ARG) entries that are not vrg_thumb_plan's, tables that do not fit them, sources or temp images
 * outside their buffers and a sheet that is not the plan's; (VRG_ERR_UNSUPPORTED) a segment whose taps pass the staging buffer.  The kernels
 * follow no entry that fails the checks which need no table; such an entry pastes nothing.  n == 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------------- */
#define VRG_THUMB_MAX_FACTOR 64
#define VRG_THUMB_MAX_SOURCE 32767
#define VRG_THUMB_STAGE_BYTES 8192
#define VRG_THUMB_STAGE_VALUES 4096
#define VRG_PIL_FILTER_LANCZOS 1
#define VRG_PIL_FILTER_BICUBIC 3

typedef struct vrg_thumb_entry {       /* one thumbnail of the sheet */
    int64_t left_offset;               /* bytes into `src` */
    int64_t right_offset;              /* bytes into `src`, or -1: no right half */
    int64_t tmp_offset;                /* bytes into `tmp`; vrg_thumb_plan */
    int64_t h_table, v_table;          /* int32 offsets into `tables` */
    int32_t left_w, left_h;            /* the original; the pair is 2 left_w x left_h */
    int32_t right_w, right_h;          /* the fixed frame */
    int32_t fx, fy;                    /* the reduce factors */
    int32_t red_w, red_h;              /* the reduced pair: ceil(pair / factor) */
    int32_t out_w, out_h;              /* the thumbnail */
    int32_t h_ksize, v_ksize;          /* vrg_pil_filter_ksize per axis, 0: the axis is copied */
    int32_t dst_x, dst_y;              /* the thumbnail's origin on the sheet */
    int32_t cps;                       /* output columns per staged segment */
    int32_t reserved;
} vrg_thumb_entry;

int32_t vrg_pil_filter_ksize(int32_t filter, float in0, float in1, int32_t n_out);
int vrg_pil_filter_table(int32_t filter, int32_t n_in, float in0, float in1, int32_t n_out, int32_t* bounds_host, int32_t* weights_host);
int vrg_pil_reduce_host(const uint8_t* src_host, int32_t height, int32_t width, int32_t channels, int32_t fx, int32_t fy, uint8_t* dst_host);
int vrg_thumb_plan(vrg_thumb_entry* entries_host, int64_t n, const double* req_host, int32_t filter, double reducing_gap, int32_t columns,
                   int64_t* sheet_host);
int vrg_thumb_plan_reduce(vrg_thumb_entry* entries_host, int64_t n, int32_t fx, int32_t fy, int32_t columns, int64_t* sheet_host);
int vrg_thumb_check(const vrg_thumb_entry* entries_host, int64_t n, const int32_t* tables_host, int64_t table_ints, int64_t src_bytes,
                    int64_t tmp_bytes, int32_t width, int32_t height, int32_t columns, int32_t cell_w, int32_t cell_h);
int vrg_thumb_rows_u8(const uint8_t* src, int64_t src_bytes, const vrg_thumb_entry* entries, int64_t n, const int32_t* tables,
                      int64_t table_ints, uint8_t* tmp, int64_t tmp_bytes, int32_t max_segments, int32_t max_rows, void* stream);
int vrg_thumb_compose_u8(const vrg_thumb_entry* entries, int64_t n, const int32_t* tables, int64_t table_ints, const uint8_t* tmp,
                         int64_t tmp_bytes, uint8_t* out, int32_t width, int32_t height, int32_t columns, int32_t cell_w, int32_t cell_h,
                         uint32_t background, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The LTX MSR reference frames (VRGDG_LTXMSRReferenceBuilder and VRGDG_LTX25MSRReferenceLoader, vrgdg_ltx_msr_reference_builder.py of the
 * reference), csrc/vrg_msr.hip and csrc/vrg_msr_math.hpp: a few distinct byte pictures, each stretched to out_w x out_h as
 * cv2.resize(..., INTER_LANCZOS4) does on bytes (what vrg_lanczos4_u8 computes, from the records of vrg_lanczos4_taps) unless it already has
 * that size, each repeated into a run of frames of out = [frames][out_h][out_w][3] fp32 (4-byte aligned) as (float)byte / 255.0f,
 * correctly rounded.  One launch: a workgroup filters one tile of one descriptor once, converts it once and stores it to every frame of
 * the run -- 16-byte non-temporal stores where the address allows them, 4-byte stores elsewhere.  Every float of every frame a
 * descriptor names is written exactly once and none is read; sources are never written and may lie at any byte address.  Any sizes >= 1
 * and any ratio.
 * vrg_msr_check refuses ON THE HOST (VRG_ERR_BAD_ARG) descriptors whose frame ranges overlap or leave a frame of 0 .. frames - 1
 * uncovered, a `taps` range outside the table of n_taps records, taps == -1 at a size other than the output's and sizes below 1.  The
 * kernel follows no descriptor that names a frame outside the batch or records outside the table; it cannot see a gap.
 * `desc` and `taps` of the launch are device memory (`taps` 4-byte aligned); zero frames or zero descriptors succeed without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct vrg_msr_desc {      /* one distinct picture of the batch */
    const uint8_t* src;            /* [in_h][in_w][3] bytes R,G,B in device memory, any alignment; null = the constant colour `fill` */
    int32_t in_h, in_w;
    int32_t taps;                  /* index of this picture's first record in `taps` (out_w column records, then out_h row records,
                                      as vrg_lanczos4_taps writes them); -1 = the picture already has the output size: its bytes, unfiltered */
    int32_t first_frame, repeats;  /* it becomes output frames first_frame .. first_frame + repeats - 1; repeats may be 0 */
    uint8_t fill[4];               /* R,G,B for src == null */
} vrg_msr_desc;

int vrg_msr_check(const vrg_msr_desc* desc_host, int64_t n_desc, int64_t n_taps, int64_t frames, int32_t out_h, int32_t out_w);
int vrg_msr_frames_f32(const vrg_msr_desc* desc, int64_t n_desc, const void* taps, int64_t n_taps,
                       float* out, int64_t frames, int32_t out_h, int32_t out_w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The LTX First / Last temporal guide (VRGDG_LTXFirstLastGuide.add_first_last_guide, VRGDG_LTXFirstLastGuide.py:52-69 of the reference),
 * csrc/vrg_flf.hip and csrc/vrg_flf_math.hpp: out[f] = first * w0[f] + last' * w1[f] for every frame f, each product and the sum rounded
 * once, where last' is the rectangle (src_x0, src_y0, src_w, src_h) of `last` resampled to w x h as F.interpolate(mode="bilinear",
 * align_corners=False) resamples the narrowed channels-last view (taps clamped to the rectangle, the result not clamped) -- or `last`
 * itself, no filter evaluated, when it has h x w and the rectangle is all of it.  first = [h][w][channels], last =
 * [last_h][last_w][channels], weights = [frames][2] (w0, w1: (float)(1.0 - amount), (float)amount, formed in double by the caller),
 * out = [frames][h][w][channels]; all fp32 in device memory, 4-byte aligned, `out` at any such address (frames that start off the 16-byte
 * grid are written with 4-byte stores).  Every float of `out` is written exactly once and none is read; `out` aliases neither input.
 * channels is 3 or 4.  vrg_flf_check refuses ON THE HOST what the launch refuses: VRG_ERR_BAD_ARG for negative frames, sizes below 1,
 * other channel counts and a rectangle that does not lie inside `last`; VRG_ERR_UNSUPPORTED for pictures of more than 2^31 - 1 floats or
 * more than 65535 * 32 frames.  Zero frames succeed without a launch.
 * ------------------------------------------------------------------------------------------- */
int vrg_flf_check(int64_t frames, int32_t h, int32_t w, int32_t channels, int32_t last_h, int32_t last_w,
                  int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h);
int vrg_flf_guide_f32(const float* first, const float* last, const float* weights, float* out, int64_t frames, int32_t h, int32_t w,
                      int32_t channels, int32_t last_h, int32_t last_w, int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-reference image batches (VRGDG_MultiReferenceConditioning, VRGDG_MultiReferenceConditioningFromPaths and
 * VRGDG_ImageBatchMultiFromPaths, VRGDG_GeneralNodes2.py:3801-4145 of the reference), csrc/vrg_refbatch.hip and
 * csrc/vrg_refbatch_math.hpp: many pictures of unrelated sizes and channel counts, each resampled as
 * comfy.utils.common_upscale(picture.movedim(-1, 1), dst_w, dst_h, method, crop) resamples it -- F.interpolate over the rectangle
 * (src_x0, src_y0, src_rw, src_rh) of the channels-last view, taps clamped to the rectangle, EVERY channel, the result NOT clamped --
 * into its own place of one output buffer, all in ONE launch.  A record is one output picture, or a run of `frames` pictures of one
 * geometry: source frame f starts at src_offset + f * src_h * src_w * src_c, output frame f at dst_offset + f * dst_h * dst_w * dst_c.
 * Channels src_c .. dst_c - 1 are the reference's F.pad(value=1.0) before the resize: a plane of 1.0f through the same filter.
 * VRG_REFBATCH_COPY moves the rectangle unfiltered, bit for bit (dst_h x dst_w is the rectangle's size); VRG_REFBATCH_BYTES does the same
 * from bytes, out = (float)byte / 255.0f correctly rounded.  The filters are evaluated even where source and target sizes agree.
 * Workgroups map to (record, frame, tile of VRG_REFBATCH_TILE floats) through first_tile, the running sum of
 * frames * ceil(dst_h * dst_w * dst_c / VRG_REFBATCH_TILE) over the earlier records, which the caller fills in; `tiles` is the sum over
 * all records.  Every float of every output picture is written exactly once and none is read; pictures that start on the 16-byte grid
 * take 16-byte stores, the others 4-byte stores; sources are never written.  src_f32, out: device fp32, 4-byte aligned; src_u8: device
 * bytes, any alignment; either source may be null when no record reads it.  `desc` of the launch is device memory.
 * vrg_refbatch_check refuses ON THE HOST what the launch refuses: VRG_ERR_BAD_ARG for sizes below 1, negative offsets or frames, channel
 * counts other than 3 or 4 (or dst_c < src_c), a rectangle outside its picture, an unknown method, a copy whose sizes differ, a span
 * outside its buffer, a first_tile that is not the running sum, and outputs that overlap; VRG_ERR_UNSUPPORTED for pictures of more than
 * 2^31 - 1 elements, more than 2^31 - 1 tiles, and an area window of more than 65536 source pixels under one output pixel.  The kernel
 * follows no record that breaks these rules or leaves the buffers; it cannot see an overlap.  Zero records succeed without a launch.
 * vrg_refbatch_quantise_u8 is the fp32 -> byte step of comfy's lanczos (np.clip(255. * x, 0, 255).astype(np.uint8): the product in fp32,
 * truncated; NaN, which numpy leaves undefined, becomes 0) for a table of VRG_REFBATCH_COPY records with dst_c == src_c, one launch:
 * dst_offset and `dst_bytes` count bytes there.  The bytes are then resampled by vrg_pil_resize_u8.
 * ------------------------------------------------------------------------------------------- */
#define VRG_REFBATCH_TILE 1024
typedef enum vrg_refbatch_method {
    VRG_REFBATCH_BICUBIC = 0, VRG_REFBATCH_BILINEAR = 1, VRG_REFBATCH_AREA = 2, VRG_REFBATCH_NEAREST_EXACT = 3,
    VRG_REFBATCH_COPY = 4, VRG_REFBATCH_BYTES = 5
} vrg_refbatch_method;

typedef struct vrg_refbatch_desc {
    int64_t src_offset;                        /* first element of the first source frame: floats of src_f32, bytes of src_u8 */
    int64_t dst_offset;                        /* first element of the first output frame */
    int32_t src_h, src_w, src_c;               /* a source frame: [src_h][src_w][src_c] */
    int32_t src_x0, src_y0, src_rw, src_rh;    /* the rectangle of it that is resampled */
    int32_t dst_h, dst_w, dst_c;               /* an output frame: [dst_h][dst_w][dst_c] */
    int32_t method;                            /* vrg_refbatch_method */
    int32_t frames;
    int32_t first_tile;
    int32_t reserved;
} vrg_refbatch_desc;

int vrg_refbatch_check(const vrg_refbatch_desc* desc_host, int64_t n, int64_t src_floats, int64_t src_bytes, int64_t out_elems);
int vrg_refbatch_f32(const float* src_f32, int64_t src_floats, const uint8_t* src_u8, int64_t src_bytes, const vrg_refbatch_desc* desc,
                     int64_t n, int64_t tiles, float* out, int64_t out_floats, void* stream);
int vrg_refbatch_quantise_u8(const float* src_f32, int64_t src_floats, const vrg_refbatch_desc* desc, int64_t n, int64_t tiles,
                             uint8_t* dst, int64_t dst_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Music-video assembly (VRGDG_CombinevideosV2 / V3, HumoAutomation.py:50-133 and :892-1030; VRGDG_CombinevideosV5,
 * HumoAutomationExtra2.py:309-498; VRGDG_PadVideoWithLastFrame, GeneralVideoNodes.py:1945-1987; VRGDG_LoadVideos, nodes.py:1327-1377 of
 * the reference), csrc/vrg_assemble.hip and csrc/vrg_assemble_math.hpp: up to VRG_ASSEMBLE_MAX_SOURCES clips of one frame shape,
 * trimmed, padded and joined into one batch by ONE launch.  `map` holds one (source, frame) entry per output frame: output frame f is
 * frame map[f].frame of clip map[f].source.  The clips' base pointers travel by value in the descriptor; `map` of a launch is device
 * memory, 4-byte aligned.
 * vrg_assemble_f32: out = [n_out][height][width][channels] fp32.  fp32 clips (bytes == 0) are copied bit for bit: NaN payloads, +-Inf,
 * -0.0 and subnormals pass.  uint8 R,G,B clips (bytes == 1, any alignment) give (float)byte / 255.0f correctly rounded.
 * vrg_assemble_labelled_u8 (channels == 3): out_u8 = [n_out][height + VRG_ASSEMBLE_BAR][width][3] bytes in B,G,R -- what the reference
 * hands its MP4 writer for the labelled copy: per value q1 = trunc(x * 255f), f = (float)q1 / 255f, q2 = trunc(f * 255f), q2 stored, both
 * roundings kept; the bar rows are 0, or byte by byte q2 of the clip's overlay[source] = [VRG_ASSEMBLE_BAR][width][3] bytes B,G,R in
 * device memory (null: a black bar).  Parity with the reference is claimed for finite x with 0 <= x * 255 < 256; outside that range the
 * bytes saturate to 0 / 255 and NaN gives 0.  out_f32, where not null, receives the batch vrg_assemble_f32 writes, from the same read.
 * Two routes, the same bits: 16-byte loads and stores when every base pointer and the frame size in bytes are multiples of 16, 4-byte
 * (bytes: 1-byte) ones otherwise.  Every element of the outputs is written exactly once and none is read; sources are never written.
 * vrg_assemble_check refuses ON THE HOST what the launches refuse (map_host, where not null, is checked too): VRG_ERR_BAD_ARG for no
 * or more than 16 clips, clips whose height, width or channels differ or are below 1, a map entry outside its clip, outputs that
 * overlap a clip, an overlay or each other, a labelled call with channels != 3, fp32 pointers off the 4-byte grid;
 * VRG_ERR_UNSUPPORTED for frames of more than 2^31 - 1 elements (frames are addressed with 64 bits).  The kernels follow no entry that
 * leaves its clip.  Zero output frames succeed without a launch.
 * ------------------------------------------------------------------------------------------- */
#define VRG_ASSEMBLE_MAX_SOURCES 16
#define VRG_ASSEMBLE_BAR 60
typedef struct vrg_assemble_desc {
    const void* src[VRG_ASSEMBLE_MAX_SOURCES];          /* [frames][height][width][channels], fp32 or bytes, device memory */
    const uint8_t* overlay[VRG_ASSEMBLE_MAX_SOURCES];   /* labelled launches: the bar of this clip's frames, or null */
    int32_t frames[VRG_ASSEMBLE_MAX_SOURCES];
    int32_t height[VRG_ASSEMBLE_MAX_SOURCES], width[VRG_ASSEMBLE_MAX_SOURCES], channels[VRG_ASSEMBLE_MAX_SOURCES];
    int32_t n_src;
    int32_t bytes;                                      /* 0: fp32 clips; 1: uint8 R,G,B clips */
} vrg_assemble_desc;

typedef struct vrg_assemble_entry { int32_t source, frame; } vrg_assemble_entry;

int vrg_assemble_check(const vrg_assemble_desc* desc, const vrg_assemble_entry* map_host, int64_t n_out, const float* out_f32,
                       const uint8_t* out_u8, int32_t labelled);
int vrg_assemble_f32(const vrg_assemble_desc* desc, const vrg_assemble_entry* map, int64_t n_out, float* out, void* stream);
int vrg_assemble_labelled_u8(const vrg_assemble_desc* desc, const vrg_assemble_entry* map, int64_t n_out, float* out_f32, uint8_t* out_u8,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * The anchor round trip of the Video Enhance and Face Fix pipelines (the Load Anchors (Meta Batch) and Store Enhanced Anchors nodes of
 * VRGDG_VideoEnhanceNodes.py and VRGDG_StandaloneFaceFixNodes.py of the reference), csrc/vrg_anchor.hip and csrc/vrg_anchor_math.hpp.
 *
 * vrg_anchor_frames_f32: n decoded R,G,B byte pictures of unrelated sizes, packed in `src`, one record each, become
 * out = [n][out_h][out_w][3] fp32 (4-byte aligned) in one launch: picture i is Image.resize((out_w, out_h), LANCZOS) of Pillow on its
 * bytes -- horizontal pass, rounded byte image, vertical pass, from the tables of vrg_pil_lanczos_table; an axis whose size stays has no
 * pass and a picture of the output's size is its own bytes -- and each byte becomes (float)byte / 255.0f, correctly rounded.  The resized
 * bytes never reach memory.  16-byte non-temporal stores where the address allows them, 4-byte stores elsewhere; every float of `out` is
 * written exactly once and none is read; `src` may lie at any byte address and is never written.  Any sizes >= 1 and any ratio.
 * vrg_anchor_check refuses ON THE HOST (VRG_ERR_BAD_ARG) a record whose picture leaves `src`, whose table leaves `tables`, whose ksize is
 * below 1 on an axis that changes, or whose table holds a record that reaches outside its axis; the kernel follows no such record
 * either (its frame is then left unwritten).  Not built, refused with VRG_ERR_UNSUPPORTED: a picture more than 100 times as tall as wide
 * whose height shrinks (Image.resize takes those vertically first).  `src`, `desc` (8-byte aligned) and `tables` (4-byte aligned) of the launch are device memory.
 *
 * vrg_anchor_store_u8: in = [pixels][channels] fp32 (channels >= 3, only the first three are read), out = [pixels][3] bytes at any
 * address: (uint8)rint(clamp(x, 0, 1) * 255.0f), the product in fp32, ties to even -- numpy's (x.clip(0, 1) * 255).round().astype("uint8")
 * -- in R,G,B order (VRG_ANCHOR_RGB) or B,G,R (VRG_ANCHOR_BGR).  NaN gives 0, what numpy yields on x86.  The bytes are written as a flat
 * run of 16-byte non-temporal pieces with single bytes in front of the first 16-byte boundary and behind the last piece.
 * ------------------------------------------------------------------------------------------- */
#define VRG_ANCHOR_RGB 0
#define VRG_ANCHOR_BGR 1

typedef struct vrg_anchor_desc {   /* one decoded picture */
    int64_t src_offset;            /* its [in_h][in_w][3] bytes in `src` */
    int64_t h_table, v_table;      /* index in `tables` of the axis table (bounds [n_out][2], weights [n_out][ksize]); unused where the axis stays */
    int32_t in_w, in_h;
    int32_t h_ksize, v_ksize;
} vrg_anchor_desc;

int vrg_anchor_check(const vrg_anchor_desc* desc_host, int64_t n, const int32_t* tables_host, int64_t table_ints, int64_t src_bytes,
                     int32_t out_h, int32_t out_w);
int vrg_anchor_frames_f32(const uint8_t* src, int64_t src_bytes, const vrg_anchor_desc* desc, int64_t n, const int32_t* tables,
                          int64_t table_ints, float* out, int32_t out_h, int32_t out_w, void* stream);
int vrg_anchor_store_u8(const float* in, uint8_t* out, int64_t pixels, int32_t channels, int32_t order, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The guidance combine of the LTX Sigma Advanced guider (_LTXSigmaAdvancedGuider.predict_noise of the reference's CustomLTXNodes.py,
 * between its model evaluations): CFG-star, CFG or APG, STG and the variance rescale; csrc/vrg_guidance.hip, arithmetic and folds in
 * csrc/vrg_guidance_math.hpp.  positive / negative / perturbed / average / guided / negative_out / average_out are fp32 tensors of ONE
 * shape, contiguous, 4-byte aligned: rows * row_len elements, row = the last three dimensions, the rows of one batch entry adjacent
 * (rows % batch == 0).  One record describes the call; Python scalars arrive rounded to fp32 once.
 *
 * The phases are separate launches on `stream`, in this order, each only where the record asks for it:
 *   vrg_guidance_sums_f32     cfg_star: per batch sum(p * n), sum(n * n) -> alpha
 *   vrg_guidance_rows_f32     APG with a negative: g = p - n' (+ momentum * average, stored to average_out where has_momentum), per row
 *                             ||g||^2, ||p||^2, <g, p> -> the row's threshold scale and projection coefficient
 *   vrg_guidance_combine_f32  guided (and negative_out = the CFG-star negative where want_negative); with has_rescale the moments of
 *                             positive and guided -> the rescale factor
 *   vrg_guidance_rescale_f32  has_rescale: guided *= factor, in place
 * Every sum is fp64: lane, wave, LDS, one partial record per workgroup in `scratch` by vector stores, and a finishing launch that adds the
 * records in a fixed order -- no atomics, no workgroup waits for another, the same inputs give the same bits.  Derived scalars stay in
 * `scratch` (device memory, 8-byte aligned, vrg_guidance_scratch_bytes(desc) bytes, the same buffer for every phase of a call); nothing
 * is read back.  A workgroup takes VRG_GUIDANCE_SPAN elements of one row: 16-byte accesses where every operand of the phase is on the
 * 16-byte grid at the same element, 4-byte accesses elsewhere.  vrg_guidance_check refuses ON THE HOST what the launches refuse:
 * VRG_ERR_BAD_ARG for sizes below 1, rows that do not divide into the batches, flags other than 0 / 1 or flags that contradict one
 * another (a star, an average or want_negative without a negative; momentum / threshold outside APG), a threshold that is not positive,
 * a rescale of fewer than two elements; VRG_ERR_UNSUPPORTED for more than 2^40 elements or 2^23 workgroups (every phase is one launch).  Outputs must not overlap
 * inputs or one another (average_out and average included).
 * ------------------------------------------------------------------------------------------- */
#define VRG_GUIDANCE_SPAN 4096
#define VRG_GUIDANCE_CFG 0
#define VRG_GUIDANCE_APG 1

typedef struct vrg_guidance_desc {
    int64_t rows, row_len, batch;
    int32_t mode;                  /* VRG_GUIDANCE_CFG / VRG_GUIDANCE_APG (read only with a negative) */
    int32_t has_negative, has_perturbed, cfg_star, has_average, has_momentum, has_threshold, has_rescale, want_negative;
    float cfg_m1;                  /* cfg - 1.0 */
    float eta, momentum, threshold, stg_scale, rescale, one_minus_rescale;
} vrg_guidance_desc;

int vrg_guidance_check(const vrg_guidance_desc* desc);
int64_t vrg_guidance_scratch_bytes(const vrg_guidance_desc* desc);      /* 0 for a record vrg_guidance_check refuses */
int vrg_guidance_sums_f32(const float* positive, const float* negative, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes,
                          void* stream);
int vrg_guidance_rows_f32(const float* positive, const float* negative, const float* average, float* average_out,
                          const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream);
int vrg_guidance_combine_f32(const float* positive, const float* negative, const float* perturbed, const float* guidance, float* guided,
                             float* negative_out, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream);
int vrg_guidance_rescale_f32(float* guided, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The Video Compare Slider's IMAGE batch as the rgb24 bytes its ffmpeg pipe takes (_write_image_batch_video of the reference's
 * VRGDG_VideoCompareNode.py), csrc/vrg_compare.hip and csrc/vrg_compare_math.hpp.
 *
 * vrg_rgb24_frames_u8: src = [pixels][channels] fp32 (4-byte aligned; channels >= 3, only the first three of a pixel are read),
 * dst = [pixels][3] bytes in R,G,B at any address: (uint8)trunc(min(max(x * 255.0f, 0.0f), 255.0f)), ONE fp32 product rounded once, then
 * the clip, then truncation -- numpy's np.clip(frame[..., :3] * 255.0, 0, 255).astype(np.uint8).  NaN gives 0 (what numpy yields on
 * x86), +Inf 255, -Inf, negatives and -0.0 give 0.  Not vrg_anchor_store_u8's rule: that one rounds, so every product in [k + 0.5, k + 1)
 * is k + 1 there and k here (a byte level k / 255.0f itself is k under both: its product is never below k, csrc/vrg_compare_math.hpp).
 * The batch is one run of pixels (a frame seam may fall inside a piece); the bytes are written as a flat run of
 * 16-byte non-temporal pieces with single bytes in front of the first 16-byte boundary and behind the last piece.  One launch;
 * VRG_ERR_UNSUPPORTED for more pieces than one grid takes (about 2^43 bytes).  src and dst must not overlap.
 * ------------------------------------------------------------------------------------------- */
int vrg_rgb24_frames_u8(const float* src, uint8_t* dst, int64_t pixels, int32_t channels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VRGDG_HIP_H_ */
