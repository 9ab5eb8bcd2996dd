// mcmc_math.h - the per-row arithmetic of the budgeted (MCMC) densifier, DESIGN.md section 6r, shared by the kernels of
// mcmc.hip (device) and by the host build tests/hostmath/mcmc.cpp (g++).  Both are compiled with -ffp-contract=off.
//
//   opacity        o = the float32 nearest to sigmoid(x), evaluated in double and rounded once
//   pick           the row of a uniform draw on an inclusive prefix of the weights
//   relocation     o' = 1 - (1 - o)^(1/M),  D = sum_{a=1..M} sum_{k<a} C(a-1,k) (-1)^k o'^(k+1) / sqrt(k+1),  o / D
//   Philox4x32-10  the counter-based generator of the in-kernel normal draws, and Box-Muller on its outputs
//   noise          g(1 - o) and Sigma z = R diag(exp(2 s)) R^T z in float32
#pragma once

#include <math.h>
#include <stdint.h>

#include "splat_math.h"

#ifndef TS_MCMC_N_MAX
#define TS_MCMC_N_MAX 51             /* M = min(c + 1, 51): a source counts as at most 51 coincident Gaussians */
#endif

// ------------------------------------------------------------------ binomials: exact integers, C(50, 25) < 2^47
struct ts_mcmc_binom_table {
    uint64_t c[TS_MCMC_N_MAX][TS_MCMC_N_MAX];
};

constexpr ts_mcmc_binom_table ts_mcmc_make_binom() {
    ts_mcmc_binom_table t{};
    for (int n = 0; n < TS_MCMC_N_MAX; ++n) {
        t.c[n][0] = 1;
        for (int k = 1; k <= n; ++k) t.c[n][k] = t.c[n - 1][k - 1] + (k <= n - 1 ? t.c[n - 1][k] : 0);
    }
    return t;
}

static constexpr ts_mcmc_binom_table kTsMcmcBinom = ts_mcmc_make_binom();

// ------------------------------------------------------------------ opacity
// sigmoid in double, rounded to float32 once: the dead test, the weights and the relocation start from this value, and
// a float64 oracle reproduces it bit for bit (a float32 expf would differ from it by device and library)
TS_HD float ts_mcmc_sigmoid(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// ------------------------------------------------------------------ drawing a row
// P: inclusive prefix of w (prefix_scan.h), n >= 1.  The bisection of density.hip's sample_kernel for the first row with
// P > target; where it lands on a row of weight 0 (no row exceeds the target, or two neighbouring prefixes associated
// differently disagree in the last bit) the nearest earlier row of positive weight, else the nearest later one.  -1 when
// no row has positive weight.
TS_HD int32_t ts_mcmc_pick(int32_t n, const double* P, const double* w, double target) {
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (P[mid] > target) hi = mid; else lo = mid + 1;
    }
    int32_t r = lo;
    while (r > 0 && !(w[r] > 0.0)) --r;
    while (r < n - 1 && !(w[r] > 0.0)) ++r;
    return w[r] > 0.0 ? r : -1;
}

// ------------------------------------------------------------------ relocation
TS_HD double ts_mcmc_split_opacity(double o, int M) { return -expm1(log1p(-o) / (double)M); }

TS_HD double ts_mcmc_series(double op, int M) {
    double s = 0.0;
    for (int a = 1; a <= M; ++a) {
        double pw = 1.0, sign = 1.0;
        for (int k = 0; k < a; ++k) {
            pw *= op;                                                       // o'^(k+1)
            s += ((double)kTsMcmcBinom.c[a - 1][k] * sign) * pw / sqrt((double)(k + 1));
            sign = -sign;
        }
    }
    return s;
}

// o' and o / D of a row of opacity o treated as M coincident Gaussians: evaluated in double, each rounded to float32 once
// (o = 0: D = 0 and the scale stays, coeff = 1).  A float32 sigmoid that has rounded to 1 is taken as the largest float32
// below 1: at o' = 1 the terms of D reach C(50, 25) = 1.3e14 against a sum below 2 and a double sum keeps no digit of it,
// while from 1 - 2^-24 down (o' <= 0.28 at M = 51) they stay below 2.4e3 and the sum is good to 1e-13.
TS_HD void ts_mcmc_relocate_values(float o, int M, float* new_opacity, float* coeff) {
    const double od = o < 1.0f ? (double)o : 1.0 - 5.9604644775390625e-08;
    const double op = ts_mcmc_split_opacity(od, M);
    const double D = ts_mcmc_series(op, M);
    *new_opacity = (float)op;
    *coeff = D > 0.0 ? (float)(od / D) : 1.0f;
}

// A row of opacity o that `count` draws picked: the logit of its new opacity and the logarithm its three log-scales
// grow by; the logarithms are float32.
TS_HD void ts_mcmc_relocate(float o, int32_t count, float min_opacity, float* new_logit, float* log_coeff) {
    const int M = count + 1 < TS_MCMC_N_MAX ? (count < 0 ? 1 : count + 1) : TS_MCMC_N_MAX;
    float p, coeff;
    ts_mcmc_relocate_values(o, M, &p, &coeff);
    const float top = 1.0f - 1.1920928955078125e-07f;                      // 1 - 2^-23
    p = p < min_opacity ? min_opacity : p;
    p = p > top ? top : p;
    *new_logit = logf(p / (1.0f - p));
    *log_coeff = logf(coeff);
}

// ------------------------------------------------------------------ Philox4x32-10 (Salmon et al., SC 2011)
TS_HD void ts_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 24 bits of a word -> a uniform in (0, 1]: ((x >> 8) + 0.5) * 2^-24 as float32 operations
TS_HD float ts_mcmc_uniform(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f; }

// the three normals of row i at `step`: key = the seed, counter = (i, step, 0, 0), Box-Muller on (u0, u1) and (u2, u3)
TS_HD void ts_mcmc_normals3(uint32_t seed_lo, uint32_t seed_hi, uint32_t i, uint32_t step, float z[3]) {
    const uint32_t ctr[4] = {i, step, 0u, 0u}, key[2] = {seed_lo, seed_hi};
    uint32_t x[4];
    ts_philox4x32_10(ctr, key, x);
    const float two_pi = 6.2831853071795864769f;
    const float r0 = sqrtf(-2.0f * logf(ts_mcmc_uniform(x[0]))), a0 = two_pi * ts_mcmc_uniform(x[1]);
    const float r1 = sqrtf(-2.0f * logf(ts_mcmc_uniform(x[2]))), a1 = two_pi * ts_mcmc_uniform(x[3]);
    z[0] = r0 * cosf(a0);
    z[1] = r0 * sinf(a0);
    z[2] = r1 * cosf(a1);
}

// ------------------------------------------------------------------ noise
// g(1 - o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))): where the exponent overflows, 1 / (1 + inf) is exactly 0
TS_HD float ts_mcmc_gate(float o) { return 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f))); }

// d = R diag(exp(2 s)) R^T z, R of the normalised quaternion (w, x, y, z)
TS_HD void ts_mcmc_sigma_z(const float q[4], const float s[3], const float z[3], float d[3]) {
    const ts::Rot R = ts::quat_to_rot(q[0], q[1], q[2], q[3]);
    const float t0 = ((R.r00 * z[0] + R.r10 * z[1]) + R.r20 * z[2]) * expf(2.0f * s[0]);
    const float t1 = ((R.r01 * z[0] + R.r11 * z[1]) + R.r21 * z[2]) * expf(2.0f * s[1]);
    const float t2 = ((R.r02 * z[0] + R.r12 * z[1]) + R.r22 * z[2]) * expf(2.0f * s[2]);
    d[0] = (R.r00 * t0 + R.r01 * t1) + R.r02 * t2;
    d[1] = (R.r10 * t0 + R.r11 * t1) + R.r12 * t2;
    d[2] = (R.r20 * t0 + R.r21 * t1) + R.r22 * t2;
}
