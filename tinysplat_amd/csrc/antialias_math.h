// antialias_math.h - opacity compensation for the 2D low-pass (antialias.hip), for host and device.
//
//   The projection adds kBlur = 0.3 to the diagonal of a Gaussian's projected covariance (splat_math.h, project_mid).  With
//   (a_o, b, c_o) the covariance BEFORE that blur and a_b = a_o + 0.3, c_b = c_o + 0.3 the blurred one,
//
//     det_o = a_o c_o - b^2          det_b = a_b c_b - b^2
//     comp  = sqrt(max(0, det_o / det_b))                       in [0, 1]
//     o_eff = opacity * comp                                    what binning and compositing see in the antialiased mode
//
//   so that the low-pass spreads a Gaussian's energy and adds none.  Where the max clamps (det_o <= 0, or a det_b that is
//   not positive) comp and every derivative of it are exactly 0.  Elsewhere the derivative is exact (no softening):
//   with h = 0.3 and Sigma_o^-1 = adj(Sigma_o) / det_o,
//
//     d comp / d Sigma  =  V  =  comp / 2 (Sigma_o^-1 - Sigma_b^-1)                (symmetric gradient matrix)
//     G  =  -Sigma_b V Sigma_b  =  -(h comp / 2) (I + h Sigma_o^-1)
//
//   G is the gradient with respect to the stored conic X = Sigma_b^-1 that project_one_vjp turns back into V
//   (v_Sigma = -X G X): adding it to v_conic carries the compensation's gradient through the unchanged projection VJP.
//   v_conic holds the true partials of the three stored entries, so its middle entry is 2 G01.
//
// Every product, sum, quotient and square root is a float32 operation rounded on its own in the order written (compiled
// with -ffp-contract=off); the exponentials of the log-scales and of the sigmoid are ts::aa_exp below, not the math
// library's, so that the host build of this header (tests/hostmath/antialias.cpp) and the kernels are one function, bit
// for bit.
#ifndef TINYSPLAT_ANTIALIAS_MATH_H
#define TINYSPLAT_ANTIALIAS_MATH_H

#include "splat_math.h"

namespace ts {

constexpr int kAaLogScales = 1;        // TS_PROJECT_LOG_SCALES
constexpr int kAaRawQuats = 2;         // TS_PROJECT_RAW_QUATS
constexpr int kAaLogitOpacity = 1;     // TS_RASTER_LOGIT_OPACITY

// exp(x) from float32 operations only: x = n ln 2 + r with n = rint(x / ln 2) and ln 2 split in two (Cody and Waite), the
// Taylor polynomial of degree 7 on |r| <= 0.347 (truncation 5e-9 relative) in Horner form, scaled by 2^n.  About 1 ulp.
// Below -87 the result is 0 and above 88 it is +inf (no subnormal results); NaN gives NaN.
TS_HD float aa_exp(float x) {
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) return INFINITY;
    const float n = rintf(x * 1.44269504f);
    const float r = (x - n * 0.693359375f) - n * -2.12194440e-4f;
    float p = 1.98412698e-4f;
    p = p * r + 1.38888889e-3f;
    p = p * r + 8.33333333e-3f;
    p = p * r + 4.16666667e-2f;
    p = p * r + 1.66666667e-1f;
    p = p * r + 0.5f;
    p = ((p * r) * r + r) + 1.0f;
    return ldexpf(p, (int)n);
}

TS_HD float aa_sigmoid(float x) { return 1.0f / (1.0f + aa_exp(-x)); }

// the opacity a kernel argument stands for: sigmoid of a logit (kAaLogitOpacity) or the value itself
TS_HD float aa_opacity(int raster_flags, float op) { return (raster_flags & kAaLogitOpacity) ? aa_sigmoid(op) : op; }

TS_HD bool aa_dets(float ao, float b, float co, float& det_o, float& det_b) {
    const float ab = ao + kBlur, cb = co + kBlur;
    det_o = ao * co - b * b;
    det_b = ab * cb - b * b;
    return det_o > 0.0f && det_b > 0.0f;           // false: the clamp (a NaN entry clamps too)
}

TS_HD float compensation(float ao, float b, float co) {
    float det_o, det_b;
    if (!aa_dets(ao, b, co, det_o, det_b)) return 0.0f;
    return sqrtf(det_o / det_b);
}

// G[3] <- v_comp times the true partials of comp with respect to the three stored conic entries (see above)
TS_HD void compensation_vjp(float ao, float b, float co, float v_comp, float G[3]) {
    G[0] = G[1] = G[2] = 0.0f;
    float det_o, det_b;
    if (!aa_dets(ao, b, co, det_o, det_b)) return;
    const float comp = sqrtf(det_o / det_b);
    const float w = comp / det_o;                  // 1 / sqrt(det_o det_b)
    const float k = (0.5f * kBlur) * v_comp;
    G[0] = -k * (comp + kBlur * (co * w));
    G[1] = (2.0f * k) * (kBlur * (b * w));
    G[2] = -k * (comp + kBlur * (ao * w));
}

// exp of log-scales and normalisation of raw quaternions, as the projection kernels prepare their inputs
// (project_inputs.h), with aa_exp; inv_norm (may be null) <- 1 / |q| of a raw quaternion
TS_HD void aa_prepare(int project_flags, float s[3], float q[4], float* inv_norm) {
    if (project_flags & kAaLogScales) { s[0] = aa_exp(s[0]); s[1] = aa_exp(s[1]); s[2] = aa_exp(s[2]); }
    if (project_flags & kAaRawQuats) {
        const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
        if (inv_norm) *inv_norm = 1.0f / n;
    }
}

// what the forward launch keeps of a Gaussian for the backward launch: one 16-byte record
struct AaRow { float ao, b, co, comp; };

// one Gaussian's record; behind the clip plane: all zeros (comp = 0).  s, q: as stored (prepared here)
TS_HD AaRow aa_forward_row(const Cam& C, int project_flags, const float m[3], float s[3], float q[4]) {
    aa_prepare(project_flags, s, q, nullptr);
    AaRow r{0.0f, 0.0f, 0.0f, 0.0f};
    ProjMid o;
    if (!project_mid(C, m, s, q, o)) return r;
    r.ao = o.ao; r.b = o.b; r.co = o.co;
    r.comp = compensation(o.ao, o.b, o.co);
    return r;
}

// the backward launch's work on one visible Gaussian: from v_oeff = dL/do_eff and the opacity argument `op` (a logit or an
// opacity, as raster_flags says) -> v_op = dL/d(op) and G[3], the addition to v_conic
TS_HD void aa_backward_row(const AaRow& r, int raster_flags, float op, float v_oeff, float& v_op, float G[3]) {
    const float sg = aa_opacity(raster_flags, op);
    compensation_vjp(r.ao, r.b, r.co, v_oeff * sg, G);
    v_op = v_oeff * r.comp;
    if (raster_flags & kAaLogitOpacity) v_op = v_op * (sg * (1.0f - sg));
}

// the stand-alone op's backward pass on one Gaussian: v_comp -> gradients of the stored means, scales and quaternions
// through project_one_vjp with v_xy = v_depth = 0.  C.p is not read for a result (every term it enters is a product with
// the zero v_xy); the caller sets it to zeros.
TS_HD void aa_comp_backward_row(const Cam& C, int project_flags, const float m[3], float s[3], float q[4], float v_comp,
                                ProjGrad& g) {
    float inv_n = 1.0f;
    aa_prepare(project_flags, s, q, &inv_n);
    for (int k = 0; k < 3; ++k) { g.v_mean[k] = 0.0f; g.v_scale[k] = 0.0f; }
    for (int k = 0; k < 4; ++k) g.v_quat[k] = 0.0f;
    ProjMid o;
    if (!project_mid(C, m, s, q, o)) return;
    float G[3];
    compensation_vjp(o.ao, o.b, o.co, v_comp, G);
    if (G[0] == 0.0f && G[1] == 0.0f && G[2] == 0.0f) return;        // the clamp, or no gradient: exact zeros
    const float v_xy[2] = {0.0f, 0.0f};
    project_one_vjp(C, m, s, q, v_xy, 0.0f, G, nullptr, g);
    if (project_flags & kAaLogScales) {               // d exp(x) = exp(x) dx
        g.v_scale[0] *= s[0]; g.v_scale[1] *= s[1]; g.v_scale[2] *= s[2];
    }
    if (project_flags & kAaRawQuats) {                // q_hat = q / |q|
        const float dotp = ((q[0] * g.v_quat[0] + q[1] * g.v_quat[1]) + q[2] * g.v_quat[2]) + q[3] * g.v_quat[3];
        for (int k = 0; k < 4; ++k) g.v_quat[k] = (g.v_quat[k] - q[k] * dotp) * inv_n;
    }
}

}  // namespace ts

#endif  // TINYSPLAT_ANTIALIAS_MATH_H
