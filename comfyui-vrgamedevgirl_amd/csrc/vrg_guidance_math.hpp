// vrg_guidance_math.hpp -- arithmetic of the LTX Sigma Advanced guider's guidance combine (csrc/vrg_guidance.hip), host and device.
//
// What is restated: _LTXSigmaAdvancedGuider.predict_noise of the reference (CustomLTXNodes.py:436-563) between its model evaluations.  With
// p, n, q = positive, negative, perturbed (fp32, one shape, 4 or 5 dimensions; a ROW is the last three dimensions, a BATCH the rows of one
// shape[0]):
//   cfg_star   alpha = sum(p * n) / (sum(n * n) + 1e-8) per batch, n = n * alpha
//   CFG        guided = p + (cfg - 1.0) * (p - n)
//   APG        g = p - n; g = momentum * average + g (the new average); g *= min(1, threshold / max(||g||, 1e-12)) per row;
//              u = p / max(||p||, 1e-12), par = sum(g * u) * u, orth = g - par in fp64, both rounded to fp32;
//              guided = p + (cfg - 1.0) * (orth + eta * par)
//   STG        guided = guided + stg_scale * (p - q)
//   rescale    guided *= rescale * (std(p) / max(std(guided), 1e-12)) + (1.0 - rescale), std unbiased over all elements
// The element-wise fp32 operations are the reference's, one rounding each, in its order (gd_* below; -ffp-contract=off).  Python scalars
// reach the kernels rounded to fp32 once, as torch rounds a scalar operand.
//
// Every sum is fp64 and every scalar derived from sums (alpha, the row scale, the row projection, the rescale factor) is formed in fp64 and
// rounded to fp32 once, where the reference reduces and divides in fp32.  Two folds, both inside the accuracy bar of
// tests/test_gpu_guidance.py (the error against the fp64 truth is at most twice the reference's own):
//   * the projection is par = p * coef with coef = <g, p> / max(||p||, 1e-12)^2 per row, not (sum(g * u)) * u with u materialised: the same
//     value up to fp64 roundings, no fp64 copy of a latent;
//   * under a norm threshold the row scale s multiplies the projection's dot product (coef = s * <g, p> / ...): the sums of the unscaled g
//     are scaled instead of reducing fl(g * s) again, which saves a pass over the latents.
// The standard deviations are merged from per-workgroup (count, mean, M2) moments taken about each workgroup's first value (Chan's rule,
// gd_merge): a constant tensor has deviation exactly 0, as torch's Welford gives, which the 1e-12 clamp of the reference turns on.
// tests/test_guidance_host.py holds this header, compiled for the host, to torch run live.
#pragma once
#include <math.h>

#include "vrg_common.hpp"

namespace vrg {

constexpr int GUIDANCE_SPAN = VRG_GUIDANCE_SPAN;      // elements of a row one workgroup takes
constexpr int GUIDANCE_RECORD = 8;                    // fp64 words of one workgroup's partial sums in the scratch buffer
constexpr int64_t GUIDANCE_MAX_WORKGROUPS = (int64_t)1 << 23;   // of one launch: 256 lanes each, and a launch counts its lanes in 32 bits

// where the derived scalars and the partial sums of a call live in its scratch buffer (byte offsets, all multiples of 8)
struct GuidanceLayout {
    int64_t segments;      // workgroups per row
    int64_t partials;      // [rows][segments][GUIDANCE_RECORD] fp64
    int64_t coef;          // [rows] fp64
    int64_t alpha;         // [batch] fp32
    int64_t scale;         // [rows] fp32
    int64_t factor;        // [2] fp32: the rescale factor (and a spare word)
    int64_t bytes;
};

inline int guidance_check(const vrg_guidance_desc* d) {
    if (!d) return VRG_ERR_BAD_ARG;
    if (d->rows < 1 || d->row_len < 1 || d->batch < 1 || d->rows % d->batch != 0) return VRG_ERR_BAD_ARG;
    if (d->mode != VRG_GUIDANCE_CFG && d->mode != VRG_GUIDANCE_APG) return VRG_ERR_BAD_ARG;
    const int32_t flags[] = {d->has_negative, d->has_perturbed, d->cfg_star, d->has_average, d->has_momentum, d->has_threshold, d->has_rescale,
                             d->want_negative};
    for (int32_t f : flags)
        if (f != 0 && f != 1) return VRG_ERR_BAD_ARG;
    if (!d->has_negative && (d->cfg_star || d->want_negative || d->has_average)) return VRG_ERR_BAD_ARG;
    const bool apg = d->has_negative && d->mode == VRG_GUIDANCE_APG;
    if (!apg && (d->has_average || d->has_momentum || d->has_threshold)) return VRG_ERR_BAD_ARG;
    if (d->has_average && !d->has_momentum) return VRG_ERR_BAD_ARG;
    if (d->has_threshold && !(d->threshold > 0.0f)) return VRG_ERR_BAD_ARG;
    // rows * row_len elements are addressed with 64 bits; the scratch buffer must stay addressable too
    if (d->rows > ((int64_t)1 << 40) / d->row_len) return VRG_ERR_UNSUPPORTED;
    if (d->has_rescale && d->rows * d->row_len < 2) return VRG_ERR_BAD_ARG;
    const int64_t segments = (d->row_len + GUIDANCE_SPAN - 1) / GUIDANCE_SPAN;
    if (segments > GUIDANCE_MAX_WORKGROUPS || d->rows > GUIDANCE_MAX_WORKGROUPS / segments) return VRG_ERR_UNSUPPORTED;      // every phase is ONE launch
    return VRG_OK;
}

// of a descriptor that guidance_check takes
inline GuidanceLayout guidance_layout(const vrg_guidance_desc* d) {
    GuidanceLayout l;
    l.segments = (d->row_len + GUIDANCE_SPAN - 1) / GUIDANCE_SPAN;
    l.partials = 0;
    l.coef = l.partials + d->rows * l.segments * GUIDANCE_RECORD * 8;
    l.alpha = l.coef + d->rows * 8;
    l.scale = l.alpha + (d->batch * 4 + 7) / 8 * 8;
    l.factor = l.scale + (d->rows * 4 + 7) / 8 * 8;
    l.bytes = l.factor + 8;
    return l;
}

// ---- element-wise, fp32, one rounding per operation, the reference's order ----------------------------------------------------------------------
VRG_HD float gd_negative(float n, float alpha) { return n * alpha; }                                         // negative * alpha
VRG_HD float gd_cfg(float p, float n, float cfg_m1) { const float d = p - n; return p + cfg_m1 * d; }        // p + (cfg - 1.0) * (p - n)
VRG_HD float gd_guidance(float p, float n) { return p - n; }
VRG_HD float gd_momentum(float g, float average, float momentum) { return momentum * average + g; }          // momentum * average + g
VRG_HD float gd_stg(float guided, float p, float q, float stg) { const float d = p - q; return guided + stg * d; }

// APG of one element: g already carries the momentum; scale (threshold) and coef (projection) belong to the element's row
VRG_HD float gd_apg(float p, float g, bool scaled, float scale, double coef, float eta, float cfg_m1) {
    const float gs = scaled ? g * scale : g;
    const double par64 = coef * (double)p;
    const float par = (float)par64, orth = (float)((double)gs - par64);
    const float modified = orth + eta * par;
    return p + cfg_m1 * modified;
}

// ---- scalars derived from fp64 sums ------------------------------------------------------------------------------------------------------------------
VRG_HD float gd_alpha(double dot, double squared) { return (float)(dot / (squared + 1e-8)); }
// min(1, threshold / max(||g||, 1e-12))
VRG_HD float gd_row_scale(double gg, float threshold) {
    double norm = sqrt(gg);
    if (norm < 1e-12) norm = 1e-12;
    const double s = (double)threshold / norm;
    return (float)(s < 1.0 ? s : 1.0);
}
// par = p * coef: coef = scale * <g, p> / max(||p||, 1e-12)^2 (scale 1 without a threshold)
VRG_HD double gd_row_coef(double gp, double pp, float scale) {
    double norm = sqrt(pp);
    if (norm < 1e-12) norm = 1e-12;
    return (double)scale * gp / norm / norm;
}

struct GdMoments { double n, mean, m2; };
// the moments of n values x from the sums of (x - pivot) and (x - pivot)^2
VRG_HD GdMoments gd_moments(double n, double pivot, double sd, double sd2) {
    if (!(n > 0.0)) return GdMoments{0.0, 0.0, 0.0};
    const double m2 = sd2 - sd * sd / n;
    return GdMoments{n, pivot + sd / n, m2 > 0.0 ? m2 : 0.0};
}
VRG_HD GdMoments gd_merge(const GdMoments& a, const GdMoments& b) {
    if (!(a.n > 0.0)) return b;
    if (!(b.n > 0.0)) return a;
    const double n = a.n + b.n, delta = b.mean - a.mean;
    return GdMoments{n, a.mean + delta * (b.n / n), a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}
// rescale * (std(p) / max(std(guided), 1e-12)) + (1.0 - rescale), both deviations unbiased
VRG_HD float gd_rescale_factor(const GdMoments& p, const GdMoments& g, float rescale, float one_minus_rescale) {
    const double std_p = sqrt(p.m2 / (p.n - 1.0));
    double std_g = sqrt(g.m2 / (g.n - 1.0));
    if (std_g < 1e-12) std_g = 1e-12;
    return (float)((double)rescale * (std_p / std_g) + (double)one_minus_rescale);
}

// ---- one element of the combine pass ---------------------------------------------------------------------------------------------------------------
// n: the raw negative; g: the guidance of the rows pass where there is a momentum (the new average), recomputed otherwise.  *n_scaled takes
// the CFG-star negative (n where there is no star).
VRG_HD float gd_guided(const vrg_guidance_desc& d, float p, float n, float q, float g, float alpha, float scale, double coef, float* n_scaled) {
    float guided = p;
    if (d.has_negative) {
        const float ns = d.cfg_star ? gd_negative(n, alpha) : n;
        *n_scaled = ns;
        if (d.mode == VRG_GUIDANCE_APG) {
            const float gg = d.has_momentum ? g : gd_guidance(p, ns);
            guided = gd_apg(p, gg, d.has_threshold != 0, scale, coef, d.eta, d.cfg_m1);
        } else {
            guided = gd_cfg(p, ns, d.cfg_m1);
        }
    }
    if (d.has_perturbed) guided = gd_stg(guided, p, q, d.stg_scale);
    return guided;
}

// the guidance of the rows pass: p - n', with the momentum's running average where there is one
VRG_HD float gd_row_guidance(const vrg_guidance_desc& d, float p, float n, float average, float alpha) {
    const float g = gd_guidance(p, d.cfg_star ? gd_negative(n, alpha) : n);
    return d.has_momentum && d.has_average ? gd_momentum(g, average, d.momentum) : g;
}

}  // namespace vrg
