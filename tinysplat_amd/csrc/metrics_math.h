// metrics_math.h - what the evaluation metrics (metrics.hip) and a host build (tests/hostmath/
// metrics.cpp) share: the conversion of a target byte, the SSIM term of one map location, the PSNR of a mean squared
// error, and the segmentation of an image into waves, which fixes the workspace size and the order of every sum.
//
//   byte      b -> (float)b / 255.0f, the correctly rounded float32 quotient: u8.to(float32) / 255.0 as the host evaluates it
//             (on the device torch multiplies by the reciprocal of a host scalar: one ulp away for 126 of the 256 bytes)
//   SSIM      pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3), the training loss's definition (train.hip):
//             from the five filtered values m1 = F(X), m2 = F(Y), q1 = F(X X), q2 = F(Y Y), r12 = F(X Y) of a location,
//             S = (2 m1 m2 + C1)(2 s12 + C2) / ((m1^2 + m2^2 + C1)(s1 + s2 + C2)), s1 = q1 - m1^2, s2 = q2 - m2^2,
//             s12 = r12 - m1 m2, C1 = 0.01^2, C2 = 0.03^2.  The device takes the two reciprocals from the hardware (1 ulp,
//             as the training kernel does), the host divides: the results differ by ~1e-7 relative
//   PSNR      -10 log10(mse) in double, torchmetrics' PeakSignalNoiseRatio(data_range=1.0); +inf where mse == 0
//   segments  one wave per 64 map columns, channel and `seg` map rows; seg is a function of the map's size alone (never
//             of the device: two devices, or none, give the same workspace and the same summation order)
#ifndef TINYSPLAT_METRICS_MATH_H
#define TINYSPLAT_METRICS_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_METRICS_HD __host__ __device__ inline
#else
#define TS_METRICS_HD inline
#endif

#define TS_METRICS_WIN 11                    // window taps
#define TS_METRICS_HALO 10                   // valid filtering: the map is (H - 10) x (W - 10)
#define TS_METRICS_COLS 64                   // map columns per wave
#define TS_METRICS_CHANNELS 3                // waves per workgroup: one per colour channel
#define TS_METRICS_PARTIALS 3                // doubles per wave: {sum of S, sum of (x - y)^2, sum of |x - y|}
#define TS_METRICS_MASKED_PARTIALS 5         // masked: + {sum of m over pixels, sum of m over window centres}
#define TS_METRICS_SEG_MIN 8
#define TS_METRICS_SEG_MAX 64
#define TS_METRICS_WORKGROUPS 768            // the grid the segmentation aims at: three workgroups on each of 256 CUs

TS_METRICS_HD float ts_metrics_byte_to_float(uint8_t b) { return (float)b / 255.0f; }

TS_METRICS_HD float ts_metrics_ssim_term(float m1, float m2, float q1, float q2, float r12) {
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    const float s1 = q1 - m1 * m1, s2 = q2 - m2 * m2, s12 = r12 - m1 * m2;
    const float A1 = 2.0f * m1 * m2 + c1, A2 = 2.0f * s12 + c2;
    const float B1 = m1 * m1 + m2 * m2 + c1, B2 = s1 + s2 + c2;
#if defined(__HIP_DEVICE_COMPILE__)
    const float i1 = __builtin_amdgcn_rcpf(B1), i2 = __builtin_amdgcn_rcpf(B2);
#else
    const float i1 = 1.0f / B1, i2 = 1.0f / B2;
#endif
    return A1 * A2 * (i1 * i2);
}

TS_METRICS_HD double ts_metrics_psnr(double mse) { return mse == 0.0 ? (double)INFINITY : -10.0 * log10(mse); }

// map rows per wave: the image in about TS_METRICS_WORKGROUPS workgroups, within [SEG_MIN, SEG_MAX]
TS_METRICS_HD int ts_metrics_segment_rows(int ho, int wo) {
    const int blocks_x = (wo + TS_METRICS_COLS - 1) / TS_METRICS_COLS;
    const int segments = TS_METRICS_WORKGROUPS / blocks_x > 0 ? TS_METRICS_WORKGROUPS / blocks_x : 1;
    const int seg = (ho + segments - 1) / segments;
    return seg < TS_METRICS_SEG_MIN ? TS_METRICS_SEG_MIN : (seg > TS_METRICS_SEG_MAX ? TS_METRICS_SEG_MAX : seg);
}

// waves of an H x W image (0 where the window does not fit): wave (segment, column block, channel) writes its partial
// sums at index (segment * column_blocks + column_block) * 3 + channel
TS_METRICS_HD int64_t ts_metrics_waves(int height, int width) {
    if (height <= TS_METRICS_HALO || width <= TS_METRICS_HALO) return 0;
    const int ho = height - TS_METRICS_HALO, wo = width - TS_METRICS_HALO;
    const int seg = ts_metrics_segment_rows(ho, wo);
    return (int64_t)TS_METRICS_CHANNELS * ((wo + TS_METRICS_COLS - 1) / TS_METRICS_COLS) * ((ho + seg - 1) / seg);
}

#endif  // TINYSPLAT_METRICS_MATH_H
