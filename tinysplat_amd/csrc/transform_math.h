// transform_math.h - the arithmetic of a similarity transform of one Gaussian (transform.hip), for
// host and device.
//
//   x' = s R x + t applied to a model: the host hands over M = fl32(s R) row-major, fl32(t), the unit quaternion r of R
//   (w x y z), fl32(log s) and, per stored SH band l, the (2l+1) x (2l+1) matrix D_l (row-major, float32).
//
//   mean      m'_i = ((M_i0 m_0 + M_i1 m_1) + M_i2 m_2) + t_i
//   scale     s'_i = s_i + log_scale
//   quat      q' = r (x) q, the Hamilton product; each component is four products added left to right as written below
//             (the norm of q is kept up to rounding; no normalisation, no sign rule)
//   SH band   c'_j = sum_k D_jk c_k, k ascending, the sum starting from the first product
//   box       inside <=> |((A_i0 m_0 + A_i1 m_1) + A_i2 m_2) + b_i| <= 1 for i = 0, 1, 2 (a NaN is outside)
//
// Plain float32, every product and sum rounded on its own (compiled with -ffp-contract=off).  The results are defined as
// the bits of this header's host build (tests/hostmath/transform.cpp).
#ifndef TINYSPLAT_TRANSFORM_MATH_H
#define TINYSPLAT_TRANSFORM_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_XF_HD __host__ __device__ inline
#else
#define TS_XF_HD inline
#endif

#define TS_XF_MAX_BANDS 4
#define TS_XF_SH_FLOATS 164      // 9 + 25 + 49 + 81: D_1 | D_2 | D_3 | D_4

// what one call applies to every Gaussian; travels to the kernel by value
struct ts_xf_params {
    float m[9];                  // fl32(s R), row-major
    float t[3];
    float r[4];                  // w x y z
    float log_scale;
    float sh[TS_XF_SH_FLOATS];   // the bands the model stores; the rest is zero and never read
};

// coefficients per channel a model of `bands` SH bands stores above the constant: 0 3 8 15 24
TS_XF_HD int ts_xf_k_rest(int bands) { return bands * (bands + 2); }
// bands of a k_rest, or -1 where k_rest is none of 0 3 8 15 24
TS_XF_HD int ts_xf_bands(int k_rest) {
    for (int b = 0; b <= TS_XF_MAX_BANDS; ++b)
        if (ts_xf_k_rest(b) == k_rest) return b;
    return -1;
}
// where D_l starts in ts_xf_params::sh (l = 1 .. 4): 0 9 34 83
TS_XF_HD constexpr int ts_xf_sh_offset(int l) { return l == 1 ? 0 : l == 2 ? 9 : l == 3 ? 34 : 83; }

// out may be in
TS_XF_HD void ts_xf_mean(const float* m9, const float* t3, const float* in, float* out) {
    const float x = in[0], y = in[1], z = in[2];
    for (int i = 0; i < 3; ++i) out[i] = ((m9[3 * i] * x + m9[3 * i + 1] * y) + m9[3 * i + 2] * z) + t3[i];
}

TS_XF_HD void ts_xf_scale(float log_scale, const float* in, float* out) {
    for (int i = 0; i < 3; ++i) out[i] = in[i] + log_scale;
}

// out may be in
TS_XF_HD void ts_xf_quat(const float* r, const float* in, float* out) {
    const float w = in[0], x = in[1], y = in[2], z = in[3];
    out[0] = ((r[0] * w - r[1] * x) - r[2] * y) - r[3] * z;
    out[1] = ((r[0] * x + r[1] * w) + r[2] * z) - r[3] * y;
    out[2] = ((r[0] * y - r[1] * z) + r[2] * w) + r[3] * x;
    out[3] = ((r[0] * z + r[1] * y) - r[2] * x) + r[3] * w;
}

// one band of one colour channel in place: c [W], W = 2 l + 1 values `stride` floats apart; every input is read before
// the first output is written
template <int W>
TS_XF_HD void ts_xf_band(const float* d, float* c, int stride) {
    float in[W];
#pragma unroll
    for (int k = 0; k < W; ++k) in[k] = c[k * stride];
    for (int j = 0; j < W; ++j) {
        float acc = d[j * W] * in[0];
#pragma unroll
        for (int k = 1; k < W; ++k) acc = acc + d[j * W + k] * in[k];
        c[j * stride] = acc;
    }
}

// one Gaussian's colors_rest row [k_rest, 3] in place; `row` may be any float storage (LDS on the device)
template <int BANDS>
TS_XF_HD void ts_xf_sh_row(const float* sh, float* row) {
    if constexpr (BANDS >= 1) {
        ts_xf_sh_row<BANDS - 1>(sh, row);
        float* band = row + 3 * ((BANDS - 1) * (BANDS + 1));      // coefficients before band l: l^2 - 1
        for (int ch = 0; ch < 3; ++ch) ts_xf_band<2 * BANDS + 1>(sh + ts_xf_sh_offset(BANDS), band + ch, 3);
    }
}

TS_XF_HD bool ts_xf_inside(const float* a9, const float* b3, const float* m) {
    bool in = true;
    for (int i = 0; i < 3; ++i) {
        const float v = ((a9[3 * i] * m[0] + a9[3 * i + 1] * m[1]) + a9[3 * i + 2] * m[2]) + b3[i];
        in = in && (fabsf(v) <= 1.0f);
    }
    return in;
}

#endif
