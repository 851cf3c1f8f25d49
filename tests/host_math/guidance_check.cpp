// Test scaffolding: csrc/vrg_guidance_math.hpp compiled for the host (g++, -ffp-contract=off), so that the element-wise expressions and the
// derived scalars of the guidance kernels are held to torch without a GPU (tests/test_guidance_host.py).  The sums come from the test
// (numpy, fp64).  Never loaded by the package.
#include <math.h>
#include <stdint.h>
// libm stand-ins for the hardware transcendentals vrg_pixel_math.hpp names (as in resize_check.cpp); this arithmetic uses none
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_guidance_math.hpp"

using namespace vrg;

extern "C" {

int hm_gd_check(const vrg_guidance_desc* d) { return guidance_check(d); }
int64_t hm_gd_scratch_bytes(const vrg_guidance_desc* d) { return guidance_check(d) == VRG_OK ? guidance_layout(d).bytes : 0; }
float hm_gd_alpha(double dot, double squared) { return gd_alpha(dot, squared); }

// the guidance of the rows pass, every element; alpha: [batch]
void hm_gd_rows(const vrg_guidance_desc* d, const float* p, const float* n, const float* average, const float* alpha, float* g) {
    const int64_t rows_per_batch = d->rows / d->batch;
    for (int64_t r = 0; r < d->rows; ++r)
        for (int64_t e = r * d->row_len; e < (r + 1) * d->row_len; ++e)
            g[e] = gd_row_guidance(*d, p[e], n[e], average ? average[e] : 0.0f, alpha[r / rows_per_batch]);
}

// sums: [rows][3] = ||g||^2, ||p||^2, <g, p>
void hm_gd_row_scalars(const vrg_guidance_desc* d, const double* sums, float* scale, double* coef) {
    for (int64_t r = 0; r < d->rows; ++r) {
        scale[r] = d->has_threshold ? gd_row_scale(sums[3 * r], d->threshold) : 1.0f;
        coef[r] = gd_row_coef(sums[3 * r + 2], sums[3 * r + 1], scale[r]);
    }
}

void hm_gd_combine(const vrg_guidance_desc* d, const float* p, const float* n, const float* q, const float* g, const float* alpha,
                   const float* scale, const double* coef, float* guided, float* n_out) {
    const int64_t rows_per_batch = d->rows / d->batch;
    for (int64_t r = 0; r < d->rows; ++r)
        for (int64_t e = r * d->row_len; e < (r + 1) * d->row_len; ++e) {
            n_out[e] = 0.0f;
            guided[e] = gd_guided(*d, p[e], n ? n[e] : 0.0f, q ? q[e] : 0.0f, g ? g[e] : 0.0f, alpha[r / rows_per_batch], scale[r], coef[r],
                                  &n_out[e]);
        }
}

float hm_gd_factor(const vrg_guidance_desc* d, double n, double mean_p, double m2_p, double mean_g, double m2_g) {
    return gd_rescale_factor(GdMoments{n, mean_p, m2_p}, GdMoments{n, mean_g, m2_g}, d->rescale, d->one_minus_rescale);
}

// parts: [count][4] = n, pivot, sum(x - pivot), sum((x - pivot)^2), merged in turn; out: n, mean, M2
void hm_gd_merge(const double* parts, int64_t count, double* out) {
    GdMoments m{0.0, 0.0, 0.0};
    for (int64_t i = 0; i < count; ++i) m = gd_merge(m, gd_moments(parts[4 * i], parts[4 * i + 1], parts[4 * i + 2], parts[4 * i + 3]));
    out[0] = m.n;
    out[1] = m.mean;
    out[2] = m.m2;
}

}  // extern "C"
