// splat_record.h - the arithmetic of the 32-byte .splat record (splatfile.hip), for host and device.
//
//   record    bytes  0..11  x y z, float32: the bits of the mean
//             bytes 12..23  exp(scale_k), float32 (expf)
//             bytes 24..27  r g b a, uint8: trunc(clip(255 (0.5 + C0 dc_k), 0, 255)), trunc(clip(255 sigmoid(opacity), 0, 255))
//             bytes 28..31  rotation w x y z, uint8: trunc(clip(128 q_k / |q| + 128, 0, 255))
//   key       the importance exp((s0 + s1) + s2) sigmoid(opacity), float32; sigmoid(o) = 1 / (1 + expf(-o))
//   edges     a NaN colour or alpha is byte 0 (clip takes NaN to 0; +inf to 255, -inf to 0); a quaternion whose norm is zero
//             or not finite is the identity 255 128 128 128.  The norm, the quotient and 128 q / |q| + 128 are formed in
//             double, so a quaternion of magnitude 1e-25 or 1e25 normalises (its squares leave float32's range).
//   decode    mean: the bits; scale = log(max(s, FLT_MIN)) (a NaN or negative s: FLT_MIN); dc = (b / 255 - 0.5) / C0;
//             opacity = log(p / (1 - p)), p = clamp(a, 1, 254) / 255; all three in double and rounded once: in float32
//             the differences b / 255 - 0.5 and 1 - p cancel and cost hundreds of ulps, and logf's result measured
//             1.8 ulp from the float64 value on the device; quat = (b - 128) / 128, exact.
//
// Colour, alpha and key are float32 expressions, every operation rounded on its own (compiled with -ffp-contract=off).
#ifndef TINYSPLAT_SPLAT_RECORD_H
#define TINYSPLAT_SPLAT_RECORD_H

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TS_SPLAT_HD __host__ __device__ inline
#else
#define TS_SPLAT_HD inline
#endif

#define TS_SPLAT_C0 0.28209479177387814
#define TS_SPLAT_RECORD_BYTES 32

// the record as the two 16-byte words a lane moves
struct ts_splat_words {
    uint32_t lo[4];   // x y z exp(s0)
    uint32_t hi[4];   // exp(s1) exp(s2) rgba wxyz
};

TS_SPLAT_HD uint32_t ts_splat_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

TS_SPLAT_HD float ts_splat_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

TS_SPLAT_HD float ts_splat_sigmoid(float o) { return 1.0f / (1.0f + expf(-o)); }

TS_SPLAT_HD float ts_splat_key(const float scales[3], float opacity) {
    return expf((scales[0] + scales[1]) + scales[2]) * ts_splat_sigmoid(opacity);
}

// trunc(clip(v, 0, 255)) with NaN -> 0 (a float32 value widens exactly)
TS_SPLAT_HD uint32_t ts_splat_byte(double v) {
    if (!(v > 0.0)) return 0u;
    return v > 255.0 ? 255u : (uint32_t)(int32_t)v;
}

TS_SPLAT_HD uint32_t ts_splat_color_byte(float dc) {
    return ts_splat_byte(255.0f * (0.5f + (float)TS_SPLAT_C0 * dc));
}

TS_SPLAT_HD uint32_t ts_splat_alpha_byte(float opacity) { return ts_splat_byte(255.0f * ts_splat_sigmoid(opacity)); }

// the four rotation bytes, w in the low byte
TS_SPLAT_HD uint32_t ts_splat_quat_bytes(const float q[4]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
    if (!(norm > 0.0) || !(norm <= DBL_MAX)) return 255u | (128u << 8) | (128u << 16) | (128u << 24);
    return ts_splat_byte(128.0 * (w / norm) + 128.0) | (ts_splat_byte(128.0 * (x / norm) + 128.0) << 8) |
           (ts_splat_byte(128.0 * (y / norm) + 128.0) << 16) | (ts_splat_byte(128.0 * (z / norm) + 128.0) << 24);
}

TS_SPLAT_HD ts_splat_words ts_splat_encode(const float mean[3], const float scales[3], const float dc[3], float opacity,
                                           const float quat[4]) {
    ts_splat_words r;
    r.lo[0] = ts_splat_bits(mean[0]);
    r.lo[1] = ts_splat_bits(mean[1]);
    r.lo[2] = ts_splat_bits(mean[2]);
    r.lo[3] = ts_splat_bits(expf(scales[0]));
    r.hi[0] = ts_splat_bits(expf(scales[1]));
    r.hi[1] = ts_splat_bits(expf(scales[2]));
    r.hi[2] = ts_splat_color_byte(dc[0]) | (ts_splat_color_byte(dc[1]) << 8) | (ts_splat_color_byte(dc[2]) << 16) |
              (ts_splat_alpha_byte(opacity) << 24);
    r.hi[3] = ts_splat_quat_bytes(quat);
    return r;
}

TS_SPLAT_HD float ts_splat_decode_scale(uint32_t bits) {
    const float s = ts_splat_float(bits);
    return (float)log((double)(s > FLT_MIN ? s : FLT_MIN));
}

TS_SPLAT_HD float ts_splat_decode_color(uint32_t b) { return (float)(((double)b / 255.0 - 0.5) / TS_SPLAT_C0); }

TS_SPLAT_HD float ts_splat_decode_opacity(uint32_t a) {
    const double p = (double)(a < 1u ? 1u : (a > 254u ? 254u : a)) / 255.0;
    return (float)log(p / (1.0 - p));
}

TS_SPLAT_HD float ts_splat_decode_quat(uint32_t b) { return ((float)b - 128.0f) / 128.0f; }

TS_SPLAT_HD void ts_splat_decode(const ts_splat_words& r, float mean[3], float scales[3], float dc[3], float* opacity,
                                 float quat[4]) {
    mean[0] = ts_splat_float(r.lo[0]);
    mean[1] = ts_splat_float(r.lo[1]);
    mean[2] = ts_splat_float(r.lo[2]);
    scales[0] = ts_splat_decode_scale(r.lo[3]);
    scales[1] = ts_splat_decode_scale(r.hi[0]);
    scales[2] = ts_splat_decode_scale(r.hi[1]);
    for (int k = 0; k < 3; ++k) dc[k] = ts_splat_decode_color((r.hi[2] >> (8 * k)) & 255u);
    *opacity = ts_splat_decode_opacity(r.hi[2] >> 24);
    for (int k = 0; k < 4; ++k) quat[k] = ts_splat_decode_quat((r.hi[3] >> (8 * k)) & 255u);
}

#endif
