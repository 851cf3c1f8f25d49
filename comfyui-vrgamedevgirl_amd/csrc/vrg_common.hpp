// vrg_common.hpp -- kernel-side parameter blocks shared by the translation units of libvrgdg_hip.so
#pragma once

// The tuning constants and the A/B or ablation switches that rounds 1-4 passed with -D are FIXED in the product sources (plain #defines
// next to their measurements; the march's and the wrong-pixel ablations are gone altogether).  Nothing in this library is selected by a
// command-line macro: a -D of one of the old names is a build error, so that no flag can turn the product into another -- or a
// wrong-answer -- library.  Variants for A/B runs are separate source files under tools/ab/ (tools/build_variant.py --source, which
// defines VRG_LAB_VARIANT_SOURCE for that one file: the frozen round-4 march still takes its -DVRG_MARCH_... switches that way).
#if !defined(VRG_LAB_VARIANT_SOURCE) && (defined(VRG_APPLY_EARLY_LOAD) || defined(VRG_APPLY_ROWS) || defined(VRG_FLAT_ROWS) || defined(VRG_GRAIN_NT) || \
    defined(VRG_PRODUCE_MAX_WAVES_LABONLY) || defined(VRG_PRODUCE_WAVES) || defined(VRG_PRODUCE_WAVES_LABONLY) || defined(VRG_PR_PIPE) || \
    defined(VRG_PR_SUBS) || defined(VRG_SG_PIPE) || defined(VRG_TILE_H) || defined(VRG_TILE_PRELOAD) || \
    defined(VRG_TS_LANES) || defined(VRG_TS_LANES_DEPTH) || defined(VRG_TS_LANES_MAX_FRAMES) || defined(VRG_TS_LANES_MEAN_DEPTH) || \
    defined(VRG_TS_MARKSTEIN) || defined(VRG_TS_ROWS_DEPTH) || defined(VRG_TS_ROWS_MAX_FRAMES) || defined(VRG_TS_SPLIT_DEPTH) || \
    defined(VRG_TS_SPLIT_MAX_FRAMES) || defined(VRG_TS_WHOLE_DEPTH) || defined(VRG_ZIV_REL) || defined(VRG_MARCH_FAST) || \
    defined(VRG_MARCH_MIN_WAVES) || defined(VRG_MARCH_FINITE) || defined(VRG_MARCH_ABLATE) || defined(VRG_MARCH_QUAD) || \
    defined(VRG_MARCH_ENDIO) || defined(VRG_MARCH_ROTATE) || defined(VRG_MARCH_TAPS_UNFOLD) || defined(VRG_MARCH_FAST_FLAT) || \
    defined(VRG_MARCH_EDGE_SHARED) || defined(VRG_MARCH_FAST_LDS) || defined(VRG_NO_POINTWISE4) || defined(VRG_NO_APPLY_MARCH) || \
    defined(VRG_NO_FLAT_STENCIL) || defined(VRG_APPLY_FORCE_GENERAL) || defined(VRG_ABLATE_GATHER) || defined(VRG_NO_DIVT_FASTPATH))
#error "comfyui-vrgamedevgirl_amd: tuning / ablation macros are not build options of the product sources (see the note above this line)"
#endif
#include <stdint.h>

#include "../../include/vrgdg_hip.h"
#include "../../include/vrgdg_hip_debug.h"
#include "vrg_pixel_math.hpp"

namespace vrg {

// Host and device, and all that a plain host compiler sees of this header (tests/host_math).
// Records name their data by offset into buffers that kernels read through raw pointers: do `need` elements from `offset` lie inside `size`?
VRG_HD bool span_fits(int64_t offset, int64_t need, int64_t size) { return offset >= 0 && offset <= size && need <= size - offset; }

}  // namespace vrg

// The one overlap rule of the entry points (include/vrgdg_hip.h, "Operands must not overlap"): do the half-open byte ranges
// [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A range of no (or a negative number of) bytes shares none, wherever it lies, and a
// null pointer is an operand that is not there.  Only the distance between the two starts is formed, never a + a_bytes, so a range that
// ends at the top of the address space does not wrap.
inline bool vrg_ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x <= y ? (uint64_t)a_bytes > (uint64_t)(y - x) : (uint64_t)b_bytes > (uint64_t)(x - y);
}
// count * each bytes of an operand, INT64_MAX where that product does not fit (no operand is that long: the range then reaches as far as
// any can, which is the refusing side)
inline int64_t vrg_operand_bytes(int64_t count, int64_t each) {
    if (count <= 0 || each <= 0) return 0;
    return count > INT64_MAX / each ? INT64_MAX : count * each;
}

namespace vrg {

// blockIdx.y / blockIdx.z take one record each, at most this many per launch
constexpr int64_t LAUNCH_RECORDS = 32768;

// The largest multiple of `align` that is at most `limit` records: the chunk length for which every chunk starts on a multiple of `align`
// (records that share state in groups of `align`: f % ref_frames, the frames of one Philox chunk).  0: no such length, align > limit.
VRG_HD int64_t aligned_step(int64_t limit, int64_t align) { return align < 1 || align > limit ? 0 : limit - limit % align; }
// The alignment that holds two at once (both at least 1 and below 2^31: no overflow).
VRG_HD int64_t chunk_lcm(int64_t a, int64_t b) {
    int64_t x = a, y = b;
    while (y) { const int64_t t = x % y; x = y; y = t; }
    return a / x * b;
}

// launch(first, count) for consecutive chunks of [0, n), each at most LAUNCH_RECORDS long and each starting on a multiple of `align`; stops at
// the first return that is not VRG_OK.  A call of more than one chunk whose alignment no chunk can hold is VRG_ERR_UNSUPPORTED.
template <class Launch>
inline int launch_chunks(int64_t n, int64_t align, Launch launch) {
    if (align < 1) return VRG_ERR_BAD_ARG;
    const int64_t step = n <= LAUNCH_RECORDS ? LAUNCH_RECORDS : aligned_step(LAUNCH_RECORDS, align);
    if (step < 1) return VRG_ERR_UNSUPPORTED;
    for (int64_t first = 0; first < n; first += step) {
        const int rc = launch(first, n - first < step ? n - first : step);
        if (rc != VRG_OK) return rc;
    }
    return VRG_OK;
}
template <class Launch>
inline int launch_chunks(int64_t n, Launch launch) { return launch_chunks(n, 1, launch); }

// Device copy of vrg_noise_desc plus the per-call geometry the noise mapping needs.
struct NoiseK {
    uint64_t seed0, seed_stride, off0, off_stride;
    int64_t chunk0;
    int64_t frame_elems;   // H*W*3
    int32_t chunk_frames;
    uint32_t G;
};

VRG_HD uint64_t chunk_seed(const NoiseK& n, int64_t chunk_rel) { return n.seed0 + (uint64_t)(n.chunk0 + chunk_rel) * n.seed_stride; }
VRG_HD uint64_t chunk_offset(const NoiseK& n, int64_t chunk_rel) { return n.off0 + (uint64_t)(n.chunk0 + chunk_rel) * n.off_stride; }

// Device copy of vrg_noise_split: the leaves of ONE randn that torch splits (more than 2^29 elements) that a launch meets, by value in the
// kernel arguments.  start = the leaf's first element relative to the launch's first element (negative: the leaf begins before it).
constexpr int NOISE_LEAVES_MAX = VRG_NOISE_LEAVES_MAX;
struct NoiseLeafK {
    int64_t start;
    uint32_t size, G;
    uint64_t off;
};
struct NoiseSplitK {
    uint64_t seed;
    int32_t count;
    NoiseLeafK leaf[NOISE_LEAVES_MAX];
};

// The leaf that holds element e of the launch: the last one that starts at or before it (the leaves are in memory order and without gaps,
// split_covers).  An element outside the table takes the nearest leaf -- the caller's own range check decides what it does with it.
VRG_HD int split_leaf_of(const NoiseSplitK& s, int64_t e) {
    int at = 0;
    for (int i = 1; i < NOISE_LEAVES_MAX; ++i)
        if (i < s.count && s.leaf[i].start <= e) at = i;
    return at;
}

// Is `s` a table for the elements [0, total) of a launch: 1 .. NOISE_LEAVES_MAX leaves that follow one another exactly (no overlap, no gap),
// every grid a non-zero multiple of 256, the first at or before element 0 and the last ending at or after `total`?
VRG_HD bool split_covers(const NoiseSplitK& s, int64_t total) {
    if (s.count < 1 || s.count > NOISE_LEAVES_MAX || total < 1) return false;
    if (s.leaf[0].start > 0 || s.leaf[0].start < -((int64_t)1 << 40)) return false;       // (no sum below can overflow)
    for (int i = 0; i < s.count; ++i) {
        const NoiseLeafK& l = s.leaf[i];
        if (l.size == 0 || l.G == 0 || (l.G % 256u) != 0 || (l.off & 3u)) return false;
        if (i > 0 && l.start != s.leaf[i - 1].start + (int64_t)s.leaf[i - 1].size) return false;
    }
    const NoiseLeafK& last = s.leaf[s.count - 1];
    return last.start + (int64_t)last.size >= total;
}

// The table of a launch that starts `elems` elements further on
VRG_HD NoiseSplitK split_shifted(const NoiseSplitK& s, int64_t elems) {
    NoiseSplitK r = s;
    for (int i = 0; i < NOISE_LEAVES_MAX; ++i) r.leaf[i].start -= elems;
    return r;
}

inline NoiseSplitK make_split(const vrg_noise_split* d) {
    NoiseSplitK s{};
    s.seed = d->seed;
    s.count = d->count;
    for (int i = 0; i < NOISE_LEAVES_MAX; ++i) {
        const bool used = i < d->count;
        s.leaf[i] = NoiseLeafK{used ? d->leaves[i].start : 0, used ? d->leaves[i].size : 0u, used ? d->leaves[i].grid_threads : 0u,
                               used ? d->leaves[i].offset : 0ull};
    }
    return s;
}

}  // namespace vrg

#if defined(__HIPCC__) || defined(__HIP__)
namespace vrg {

// one RGB pixel; 4-byte aligned so that a load/store is a single global_*_dwordx3
struct __attribute__((packed, aligned(4))) px3 { float r, g, b; };

// Frame data is streamed once: point-wise kernels load it, and tile / point-wise kernels store it, with the
// non-temporal hint so that it does not displace the LUT records from the per-XCD L2 (measured: 3x3 stencil
// 4.3 -> 4.76 TB/s).  Kernels whose loads are re-read by neighbouring workgroups (tile halos) and the wave-march
// kernel (61-lane partial-line stores) use plain accesses.  clang merges the three scalars into one
// global_load/store_dwordx3 ... nt.
__device__ __forceinline__ px3 load_px_stream(const px3* p) {
    const float* f = reinterpret_cast<const float*>(p);
    px3 v;
    v.r = __builtin_nontemporal_load(f);
    v.g = __builtin_nontemporal_load(f + 1);
    v.b = __builtin_nontemporal_load(f + 2);
    return v;
}
__device__ __forceinline__ void store_px_stream(px3* p, const px3& v) {
    float* f = reinterpret_cast<float*>(p);
    __builtin_nontemporal_store(v.r, f);
    __builtin_nontemporal_store(v.g, f + 1);
    __builtin_nontemporal_store(v.b, f + 2);
}

// Frame element types at the kernel boundary.  IoF32: the reference's fp32 RGB tensors (12 B/px).  IoU8: decoded video
// frames as cv2 hands them over, uint8 BGR (3 B/px) -- the /255, the *255-clip-truncate and the channel swap of
// _frames_to_tensor / _tensor_to_frames happen in the load / store of the kernel that does the work, so a route batch
// moves 3 + 3 B/px through HBM (and over PCIe) instead of 12 + 12.
struct __attribute__((packed)) bgr8 { uint8_t b, g, r; };

struct IoF32 {
    typedef px3 elem;
    static __device__ __forceinline__ px3 load_stream(const elem* p) { return load_px_stream(p); }
    static __device__ __forceinline__ px3 load(const elem* p) { return *p; }
    static __device__ __forceinline__ void store_stream(elem* p, const px3& v) { store_px_stream(p, v); }
    static __device__ __forceinline__ void store(elem* p, const px3& v) { *p = v; }
};
struct IoU8 {
    typedef bgr8 elem;
    static __device__ __forceinline__ px3 load(const elem* p) {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
        return px3{unit_from_u8(q[2]), unit_from_u8(q[1]), unit_from_u8(q[0])};
    }
    static __device__ __forceinline__ px3 load_stream(const elem* p) { return load(p); }
    static __device__ __forceinline__ void store(elem* p, const px3& v) {
        uint8_t* q = reinterpret_cast<uint8_t*>(p);
        q[0] = u8_from_unit(v.b);
        q[1] = u8_from_unit(v.g);
        q[2] = u8_from_unit(v.r);
    }
    static __device__ __forceinline__ void store_stream(elem* p, const px3& v) { store(p, v); }
};

// Stage the node table of a small cube into LDS (one float4 per node) from the record table of vrg_lut_prepare_f32.
// Every thread of the workgroup must call it; the caller synchronises afterwards.
__device__ __forceinline__ void lut_nodes_to_lds(const LutParams& P, f32x4* nodes, int tid, int nthreads) {
    const int n = P.n, nc = n - 1, total = n * n * n;
    for (int i = tid; i < total; i += nthreads) {
        const int r = i % n, g = (i / n) % n, b = i / (n * n);
        const int b0 = b < nc ? b : nc - 1, g0 = g < nc ? g : nc - 1;
        const int k = (g - g0) * 2 + (b - b0);
        const float* rec = P.cells + (size_t)((b0 * nc + g0) * n + r) * LUT_REC_FLOATS;
        f32x4 v;
        v.x = rec[k]; v.y = rec[4 + k]; v.z = rec[8 + k]; v.w = 0.0f;
        nodes[i] = v;
    }
}

struct CmK {
    const float* img_ms;   // [frames][3][2]
    const float* ref_ms;   // [ref_frames][3][2]
    int32_t ref_frames;
    float K, T;
};

struct ChainK {
    int32_t stages;
    float I, S, T;
    NoiseK noise;
    LutParams lut;
    CmK cm;
    DevMath dm;             // pow exponents of the "device" colour-match arithmetic (runtime values, see vrg_pixel_math.hpp)
    int32_t stencil_op, zero_border;
    float strength;
};

// Internal template bit next to the public VRG_STAGE_* bits: Lab / colour-match arithmetic with the fast policy
// (PowTables) instead of the default device policy (DevMath).  Never part of vrg_chain_desc::stages; set from cm_math.
constexpr int VRG_STAGE_FASTMATH = 32;

inline DevMath host_dev_math() { return DevMath{(float)2.4, (float)(1.0 / 2.4), (float)(1.0 / 3.0), nullptr}; }

template <bool FAST> struct CmMathSel { typedef DevMath type; };
template <> struct CmMathSel<true> { typedef PowTables type; };
__device__ __forceinline__ PowTables cm_make_math(const float* lds, const DevMath&, const PowTables*) { return PowTables{lds, lds + 512}; }
__device__ __forceinline__ DevMath cm_make_math(const float* lds, const DevMath& dm, const DevMath*) {
    DevMath m = dm;
    m.logt = lds;            // dev_pow_ziv's log table, staged by VRG_CM_MATH
    return m;
}

inline NoiseK make_noise(const vrg_noise_desc* d, int64_t frame_elems) {
    NoiseK n;
    n.seed0 = d->seed0; n.seed_stride = d->seed_stride; n.off0 = d->offset0; n.off_stride = d->offset_stride;
    n.chunk0 = d->chunk0; n.frame_elems = frame_elems; n.chunk_frames = d->chunk_frames; n.G = d->grid_threads;
    return n;
}

inline LutParams make_lut(const float* cells, int n, const float dmin[3], const float dmax[3], int blend_mode,
                          float blend, float one_minus_blend) {
    LutParams P;
    P.cells = cells; P.n = n; P.top = (float)(n - 1);
    P.unit_domain = 1;
    for (int c = 0; c < 3; ++c) {
        P.dmin[c] = dmin[c];
        const float span = dmax[c] - dmin[c];
        P.span[c] = span < 1e-6f ? 1e-6f : span;   // torch.clamp(domain_max - domain_min, min=1e-6)
        if (!(P.dmin[c] == 0.0f && P.span[c] == 1.0f)) P.unit_domain = 0;
    }
    P.blend_mode = blend_mode; P.blend = blend; P.one_minus_blend = one_minus_blend;
    return P;
}

// The colour-match arithmetic object of a kernel: NEED = does the kernel evaluate Lab at all, FAST = policy.  The fast
// policy stages its pow tables in LDS (2.5 KB), the device policy the log table of dev_pow_ziv (2 KB).  Every thread of the
// block must execute it (barrier).
#define VRG_CM_MATH(PT, NEED, FAST, DM)                                                                       \
    __shared__ __attribute__((aligned(16))) float vrg_pow_lds_[(NEED) ? ((FAST) ? ::vrg::POW_TABLE_WORDS : ::vrg::ZIV_TABLE_WORDS) : 4]; \
    if (NEED) {                                                                                                \
        if (FAST) ::vrg::pow_tables_fill(vrg_pow_lds_, (int)threadIdx.x, (int)blockDim.x);                    \
        else ::vrg::ziv_table_fill(vrg_pow_lds_, (int)threadIdx.x, (int)blockDim.x);                          \
        __syncthreads();                                                                                       \
    }                                                                                                          \
    typedef typename ::vrg::CmMathSel<(FAST)>::type PT##_t;                                                    \
    const PT##_t PT = ::vrg::cm_make_math(vrg_pow_lds_, (DM), (const PT##_t*)nullptr)

#define VRG_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e_ = hipGetLastError();                   \
        if (e_ != hipSuccess) return VRG_ERR_LAUNCH;         \
    } while (0)

// The sums of a 256-thread workgroup: acc[i] of every lane -> the 64-lane xor butterfly -> part[wave][i], synchronised.  Every thread of the
// workgroup must call it; the caller adds the four wave partials of a sum in the order it needs.
template <class T, int N>
__device__ __forceinline__ void block_sum_4waves(T (&acc)[N], T (&part)[4][N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
}

}  // namespace vrg
#endif
