// vrg_guidance.hip -- the guidance combine of the LTX Sigma Advanced guider (CustomLTXNodes.py:436-563 of the reference): CFG-star, CFG or
// APG, STG and the variance rescale over two or three latents.  gfx950 only.  Arithmetic and the two folds: csrc/vrg_guidance_math.hpp.
//
// The latents are small (1 x 128 x 33 x 22 x 38 is 14 MB each) and stay in the L2 / Infinity Cache between the phases, so every phase is a
// streaming launch with plain (temporal) accesses.  The grid is rows x segments of a row -- one dimension, blockIdx.x = row * segments + segment
// of GUIDANCE_SPAN elements, at most GUIDANCE_MAX_WORKGROUPS of them (guidance_check; one launch, nothing is chunked) -- so 128 short rows still make several hundred workgroups.  A lane takes four consecutive
// floats at a time: one 16-byte access per operand where every operand of the phase sits on the 16-byte grid at the same element of the
// segment (a row base is only 4-byte aligned when row_len % 4 != 0 or the tensor is a slice: lane 0 then takes the 1 .. 3 floats in front
// of the grid singly), 4-byte accesses where the operands disagree; the last group of a segment takes its 1 .. 3 floats singly.
//
// Sums: fp64 in the lane (a fixed order), the 64-lane butterfly, four wave partials in LDS, ONE record of GUIDANCE_RECORD fp64 words per
// workgroup stored to the scratch buffer; a finishing launch adds the records of a batch / a row / the tensor in a fixed order and leaves the
// derived scalar in the scratch buffer for the next phase, which is a later launch on the same stream.  No atomics, no workgroup waits for
// another one, nothing returns to the host.
#include "vrg_guidance_math.hpp"

namespace vrg {

typedef float gd_f4 __attribute__((ext_vector_type(4)));

// the segment of a workgroup: `base` = its first element in the tensor, `len` its elements, `head` the floats in front of the 16-byte grid,
// `vec` = every operand of the phase is on the grid at base + head
struct GdSpan {
    int64_t base, row;
    int32_t len, head;
    bool vec;
};

__device__ __forceinline__ GdSpan gd_span(const vrg_guidance_desc& d, const void* const* operands, int count) {
    GdSpan s;
    const uint32_t segments = (uint32_t)((d.row_len + GUIDANCE_SPAN - 1) / GUIDANCE_SPAN);
    s.row = blockIdx.x / segments;
    const int64_t s0 = (int64_t)(blockIdx.x % segments) * GUIDANCE_SPAN, left = d.row_len - s0;
    s.base = s.row * d.row_len + s0;
    s.len = (int32_t)(left < GUIDANCE_SPAN ? left : GUIDANCE_SPAN);
    uint32_t phase = 0;
    bool same = true, any = false;
    for (int i = 0; i < count; ++i) {
        if (!operands[i]) continue;
        const uint32_t ph = (uint32_t)((reinterpret_cast<uintptr_t>(operands[i]) + (uintptr_t)s.base * 4u) & 15u);
        if (!any) { phase = ph; any = true; }
        else if (ph != phase) same = false;
    }
    s.vec = same;
    s.head = same ? (int32_t)(((16u - phase) & 15u) >> 2) : 0;
    if (s.head > s.len) s.head = s.len;
    return s;
}

__device__ __forceinline__ void gd_load(const float* p, int valid, bool vec, float (&v)[4]) {
    if (vec && valid == 4) {
        const gd_f4 t = *reinterpret_cast<const gd_f4*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < valid ? p[k] : 0.0f;
    }
}

__device__ __forceinline__ void gd_store(float* p, int valid, bool vec, const float (&v)[4]) {
    if (vec && valid == 4) {
        *reinterpret_cast<gd_f4*>(p) = gd_f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < valid) p[k] = v[k];
    }
}

// body(offset in the segment, valid floats 1 .. 4, vector access allowed) over the whole segment: the head by lane 0, then the groups of four
template <class Body>
__device__ __forceinline__ void gd_walk(const GdSpan& s, Body body) {
    if (s.head > 0 && threadIdx.x == 0) body(0, s.head, false);
    for (int32_t o = s.head + 4 * (int32_t)threadIdx.x; o < s.len; o += 4 * 256) {
        const int32_t left = s.len - o;
        body(o, left < 4 ? left : 4, s.vec);
    }
}

// the workgroup's sums -> its record
template <int N>
__device__ __forceinline__ void gd_write_record(double (&acc)[N], double* partials, int64_t record) {
    __shared__ double part[4][N];
    block_sum_4waves(acc, part);
    if (threadIdx.x < N) {
        const int i = threadIdx.x;
        partials[record * GUIDANCE_RECORD + i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
    }
}

__device__ __forceinline__ int64_t gd_record(const GdSpan&) { return (int64_t)blockIdx.x; }

// ---- phase 1: per batch sum(p * n), sum(n * n) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gd_sums(const float* __restrict__ p, const float* __restrict__ n, vrg_guidance_desc d,
                                                 double* __restrict__ partials) {
    const void* ops[2] = {p, n};
    const GdSpan s = gd_span(d, ops, 2);
    double acc[2] = {0.0, 0.0};
    gd_walk(s, [&](int32_t o, int valid, bool vec) {
        float pv[4], nv[4];
        gd_load(p + s.base + o, valid, vec, pv);
        gd_load(n + s.base + o, valid, vec, nv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {            // (the floats past `valid` are zeros: they add nothing)
            acc[0] += (double)pv[k] * (double)nv[k];
            acc[1] += (double)nv[k] * (double)nv[k];
        }
    });
    gd_write_record(acc, partials, gd_record(s));
}

// one wave per batch: its records in a fixed order -> alpha
__global__ __launch_bounds__(64) void k_gd_finish_alpha(const double* __restrict__ partials, int64_t records_per_batch, float* __restrict__ alpha) {
    const double* rec = partials + (int64_t)blockIdx.x * records_per_batch * GUIDANCE_RECORD;
    double dot = 0.0, sq = 0.0;
    for (int64_t r = threadIdx.x; r < records_per_batch; r += 64) {
        dot += rec[r * GUIDANCE_RECORD];
        sq += rec[r * GUIDANCE_RECORD + 1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        dot += __shfl_xor(dot, off, 64);
        sq += __shfl_xor(sq, off, 64);
    }
    if (threadIdx.x == 0) alpha[blockIdx.x] = gd_alpha(dot, sq);
}

// ---- phase 2 (APG): the guidance, the new average, per row ||g||^2, ||p||^2, <g, p> -----------------------------------------------------
__global__ __launch_bounds__(256) void k_gd_rows(const float* __restrict__ p, const float* __restrict__ n, const float* __restrict__ average,
                                                 float* __restrict__ average_out, vrg_guidance_desc d,
                                                 const float* __restrict__ alpha, double* __restrict__ partials) {
    const void* ops[4] = {p, n, average, average_out};
    const GdSpan s = gd_span(d, ops, 4);
    const float a = d.cfg_star ? alpha[s.row / (d.rows / d.batch)] : 1.0f;
    double acc[3] = {0.0, 0.0, 0.0};
    gd_walk(s, [&](int32_t o, int valid, bool vec) {
        float pv[4], nv[4], av[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv[4];
        gd_load(p + s.base + o, valid, vec, pv);
        gd_load(n + s.base + o, valid, vec, nv);
        if (average) gd_load(average + s.base + o, valid, vec, av);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gv[k] = gd_row_guidance(d, pv[k], nv[k], av[k], a);
            if (k < valid) {
                acc[0] += (double)gv[k] * (double)gv[k];
                acc[1] += (double)pv[k] * (double)pv[k];
                acc[2] += (double)gv[k] * (double)pv[k];
            }
        }
        if (average_out) gd_store(average_out + s.base + o, valid, vec, gv);
    });
    gd_write_record(acc, partials, gd_record(s));
}

// one wave per row: its records in a fixed order -> the threshold scale and the projection coefficient
__global__ __launch_bounds__(64) void k_gd_finish_rows(const double* __restrict__ partials, int64_t segments, vrg_guidance_desc d,
                                                       float* __restrict__ scale, double* __restrict__ coef) {
    const double* rec = partials + (int64_t)blockIdx.x * segments * GUIDANCE_RECORD;
    double gg = 0.0, pp = 0.0, gp = 0.0;
    for (int64_t r = threadIdx.x; r < segments; r += 64) {
        gg += rec[r * GUIDANCE_RECORD];
        pp += rec[r * GUIDANCE_RECORD + 1];
        gp += rec[r * GUIDANCE_RECORD + 2];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gg += __shfl_xor(gg, off, 64);
        pp += __shfl_xor(pp, off, 64);
        gp += __shfl_xor(gp, off, 64);
    }
    if (threadIdx.x == 0) {
        const float sc = d.has_threshold ? gd_row_scale(gg, d.threshold) : 1.0f;
        scale[blockIdx.x] = sc;
        coef[blockIdx.x] = gd_row_coef(gp, pp, sc);
    }
}

// ---- phase 3: guided (and the CFG-star negative); with a rescale the moments of positive and guided ----------------------------------------
__global__ __launch_bounds__(256) void k_gd_combine(const float* __restrict__ p, const float* __restrict__ n, const float* __restrict__ q,
                                                    const float* __restrict__ g, float* __restrict__ guided, float* __restrict__ n_out,
                                                    vrg_guidance_desc d, const float* __restrict__ alpha,
                                                    const float* __restrict__ scale, const double* __restrict__ coef,
                                                    double* __restrict__ partials) {
    const void* ops[6] = {p, n, q, g, guided, n_out};
    const GdSpan s = gd_span(d, ops, 6);
    const bool apg = d.has_negative && d.mode == VRG_GUIDANCE_APG;
    const float a = d.cfg_star ? alpha[s.row / (d.rows / d.batch)] : 1.0f;
    const float sc = apg ? scale[s.row] : 1.0f;
    const double cf = apg ? coef[s.row] : 0.0;
    double pivot_p = 0.0, pivot_g = 0.0;
    if (d.has_rescale) {                         // the segment's first value of both tensors: one address for all lanes
        float unused;
        const float p0 = p[s.base];
        pivot_p = (double)p0;
        pivot_g = (double)gd_guided(d, p0, n ? n[s.base] : 0.0f, q ? q[s.base] : 0.0f, g ? g[s.base] : 0.0f, a, sc, cf, &unused);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    gd_walk(s, [&](int32_t o, int valid, bool vec) {
        float pv[4], nv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4], ns[4];
        gd_load(p + s.base + o, valid, vec, pv);
        if (n) gd_load(n + s.base + o, valid, vec, nv);
        if (q) gd_load(q + s.base + o, valid, vec, qv);
        if (g) gd_load(g + s.base + o, valid, vec, gv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ns[k] = 0.0f;
            out[k] = gd_guided(d, pv[k], nv[k], qv[k], gv[k], a, sc, cf, &ns[k]);
            if (d.has_rescale && k < valid) {
                const double dp = (double)pv[k] - pivot_p, dg = (double)out[k] - pivot_g;
                acc[0] += dp;
                acc[1] += dp * dp;
                acc[2] += dg;
                acc[3] += dg * dg;
            }
        }
        gd_store(guided + s.base + o, valid, vec, out);
        if (n_out) gd_store(n_out + s.base + o, valid, vec, ns);
    });
    if (d.has_rescale) {                         // (uniform: every thread of the workgroup takes the barrier)
        __shared__ double part[4][4];
        block_sum_4waves(acc, part);
        if (threadIdx.x == 0) {
            double* rec = partials + gd_record(s) * GUIDANCE_RECORD;
            rec[0] = (double)s.len;
            rec[1] = pivot_p;
            rec[2] = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
            rec[3] = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
            rec[4] = pivot_g;
            rec[5] = ((part[0][2] + part[1][2]) + part[2][2]) + part[3][2];
            rec[6] = ((part[0][3] + part[1][3]) + part[2][3]) + part[3][3];
        }
    }
}

// one workgroup: every record's moments merged in a fixed order (a lane's records in turn, then a tree over the lanes) -> the factor
__global__ __launch_bounds__(256) void k_gd_finish_moments(const double* __restrict__ partials, int64_t records, vrg_guidance_desc d,
                                                           float* __restrict__ factor) {
    __shared__ GdMoments mp[256], mg[256];
    GdMoments a{0.0, 0.0, 0.0}, b{0.0, 0.0, 0.0};
    for (int64_t r = threadIdx.x; r < records; r += 256) {
        const double* rec = partials + r * GUIDANCE_RECORD;
        a = gd_merge(a, gd_moments(rec[0], rec[1], rec[2], rec[3]));
        b = gd_merge(b, gd_moments(rec[0], rec[4], rec[5], rec[6]));
    }
    mp[threadIdx.x] = a;
    mg[threadIdx.x] = b;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            mp[threadIdx.x] = gd_merge(mp[threadIdx.x], mp[threadIdx.x + step]);
            mg[threadIdx.x] = gd_merge(mg[threadIdx.x], mg[threadIdx.x + step]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) factor[0] = gd_rescale_factor(mp[0], mg[0], d.rescale, d.one_minus_rescale);
}

// ---- phase 4: guided *= factor -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gd_rescale(float* __restrict__ guided, vrg_guidance_desc d, const float* __restrict__ factor) {
    const void* ops[1] = {guided};
    const GdSpan s = gd_span(d, ops, 1);
    const float f = factor[0];
    gd_walk(s, [&](int32_t o, int valid, bool vec) {
        float v[4];
        gd_load(guided + s.base + o, valid, vec, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] * f;
        gd_store(guided + s.base + o, valid, vec, v);
    });
}

// what every phase checks before it launches: the record, the scratch buffer, its operands (null where the record has none)
struct GdCall {
    GuidanceLayout l;
    char* scratch;
    double* partials() const { return reinterpret_cast<double*>(scratch + l.partials); }
    double* coef() const { return reinterpret_cast<double*>(scratch + l.coef); }
    float* alpha() const { return reinterpret_cast<float*>(scratch + l.alpha); }
    float* scale() const { return reinterpret_cast<float*>(scratch + l.scale); }
    float* factor() const { return reinterpret_cast<float*>(scratch + l.factor); }
};

static int gd_prepare(const vrg_guidance_desc* d, void* scratch, int64_t scratch_bytes, GdCall* call) {
    const int rc = guidance_check(d);
    if (rc != VRG_OK) return rc;
    call->l = guidance_layout(d);
    call->scratch = static_cast<char*>(scratch);
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7u) != 0 || scratch_bytes < call->l.bytes) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

// operands: every tensor of the phase, present or not; the first `writes` are written.  All 4-byte aligned, no written one overlaps another
// operand or the scratch buffer.
static bool gd_operands_ok(const vrg_guidance_desc* d, const GdCall& call, const void* const* operands, int count, int writes) {
    const int64_t bytes = vrg_operand_bytes(d->rows * d->row_len, 4);
    for (int i = 0; i < count; ++i) {
        if (!operands[i]) continue;
        if ((reinterpret_cast<uintptr_t>(operands[i]) & 3u) != 0) return false;
        if (vrg_ranges_overlap(operands[i], bytes, call.scratch, call.l.bytes)) return false;
        for (int j = 0; j < writes && j < count; ++j)
            if (j != i && vrg_ranges_overlap(operands[i], bytes, operands[j], bytes)) return false;
    }
    return true;
}

static dim3 gd_grid(const GdCall& call, const vrg_guidance_desc& d) { return dim3((uint32_t)(d.rows * call.l.segments)); }

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_guidance_check(const vrg_guidance_desc* desc) { return guidance_check(desc); }

int64_t vrg_guidance_scratch_bytes(const vrg_guidance_desc* desc) {
    return guidance_check(desc) == VRG_OK ? guidance_layout(desc).bytes : 0;
}

int vrg_guidance_sums_f32(const float* positive, const float* negative, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes,
                          void* stream) {
    GdCall call;
    const int rc = gd_prepare(desc, scratch, scratch_bytes, &call);
    if (rc != VRG_OK) return rc;
    if (!desc->cfg_star || !positive || !negative) return VRG_ERR_BAD_ARG;
    const void* operands[2] = {positive, negative};
    if (!gd_operands_ok(desc, call, operands, 2, 0)) return VRG_ERR_BAD_ARG;
    const vrg_guidance_desc d = *desc;
    hipLaunchKernelGGL(k_gd_sums, gd_grid(call, d), dim3(256), 0, (hipStream_t)stream, positive, negative, d, call.partials());
    VRG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gd_finish_alpha, dim3((uint32_t)d.batch), dim3(64), 0, (hipStream_t)stream, call.partials(),
                       d.rows / d.batch * call.l.segments, call.alpha());
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_guidance_rows_f32(const float* positive, const float* negative, const float* average, float* average_out,
                          const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream) {
    GdCall call;
    const int rc = gd_prepare(desc, scratch, scratch_bytes, &call);
    if (rc != VRG_OK) return rc;
    if (!desc->has_negative || desc->mode != VRG_GUIDANCE_APG || !positive || !negative) return VRG_ERR_BAD_ARG;
    if ((desc->has_average != 0) != (average != nullptr) || (desc->has_momentum != 0) != (average_out != nullptr)) return VRG_ERR_BAD_ARG;
    const void* operands[4] = {average_out, positive, negative, average};
    if (!gd_operands_ok(desc, call, operands, 4, 1)) return VRG_ERR_BAD_ARG;
    const vrg_guidance_desc d = *desc;
    hipLaunchKernelGGL(k_gd_rows, gd_grid(call, d), dim3(256), 0, (hipStream_t)stream, positive, negative, average, average_out, d,
                       (const float*)call.alpha(), call.partials());
    VRG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gd_finish_rows, dim3((uint32_t)d.rows), dim3(64), 0, (hipStream_t)stream, (const double*)call.partials(), call.l.segments, d,
                       call.scale(), call.coef());
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

int vrg_guidance_combine_f32(const float* positive, const float* negative, const float* perturbed, const float* guidance, float* guided,
                             float* negative_out, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream) {
    GdCall call;
    const int rc = gd_prepare(desc, scratch, scratch_bytes, &call);
    if (rc != VRG_OK) return rc;
    if (!positive || !guided) return VRG_ERR_BAD_ARG;
    if ((desc->has_negative != 0) != (negative != nullptr) || (desc->has_perturbed != 0) != (perturbed != nullptr) ||
        (desc->want_negative != 0) != (negative_out != nullptr) || (desc->has_momentum != 0) != (guidance != nullptr))
        return VRG_ERR_BAD_ARG;
    const void* operands[6] = {guided, negative_out, positive, negative, perturbed, guidance};
    if (!gd_operands_ok(desc, call, operands, 6, 2)) return VRG_ERR_BAD_ARG;
    const vrg_guidance_desc d = *desc;
    hipLaunchKernelGGL(k_gd_combine, gd_grid(call, d), dim3(256), 0, (hipStream_t)stream, positive, negative, perturbed, guidance, guided,
                       negative_out, d, (const float*)call.alpha(), (const float*)call.scale(), (const double*)call.coef(),
                       call.partials());
    VRG_CHECK_LAUNCH();
    if (d.has_rescale) {
        hipLaunchKernelGGL(k_gd_finish_moments, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)call.partials(),
                           d.rows * call.l.segments, d, call.factor());
        VRG_CHECK_LAUNCH();
    }
    return VRG_OK;
}

int vrg_guidance_rescale_f32(float* guided, const vrg_guidance_desc* desc, void* scratch, int64_t scratch_bytes, void* stream) {
    GdCall call;
    const int rc = gd_prepare(desc, scratch, scratch_bytes, &call);
    if (rc != VRG_OK) return rc;
    if (!desc->has_rescale || !guided) return VRG_ERR_BAD_ARG;
    const void* operands[1] = {guided};
    if (!gd_operands_ok(desc, call, operands, 1, 1)) return VRG_ERR_BAD_ARG;
    const vrg_guidance_desc d = *desc;
    hipLaunchKernelGGL(k_gd_rescale, gd_grid(call, d), dim3(256), 0, (hipStream_t)stream, guided, d, (const float*)call.factor());
    VRG_CHECK_LAUNCH();
    return VRG_OK;
}

}  // extern "C"
