// undistort_math.h - the arithmetic of image undistortion and resampling (undistort.hip), for host and
// device.
//
//   distortion  OpenCV's rational model, coefficients d = (k1, k2, p1, p2, k3, k4, k5, k6):
//                 r2  = x x + y y
//                 rad = (1 + r2 (k1 + r2 (k2 + r2 k3))) / (1 + r2 (k4 + r2 (k5 + r2 k6)))
//                 xd  = x rad + p1 (2 x y) + p2 (r2 + 2 x x)
//                 yd  = y rad + p1 (r2 + 2 y y) + p2 (2 x y)
//   COLMAP      SIMPLE_RADIAL k -> k1; RADIAL k1 k2 -> k1 k2; OPENCV k1 k2 p1 p2 and FULL_OPENCV k1 k2 p1 p2 k3 k4 k5 k6 as
//               they are; the pinhole models: zeros.
//   map         output pixel index (u, v) -> x = (u - cx') / fx', y = (v - cy') / fy' -> (xd, yd) -> the source index
//               (fx xd + cx, fy yd + cy).  Indices count pixel centres: the first pixel's centre is 0.
//   lookup      the source index is clamped to [0, W-1] x [0, H-1] (a replicate border; NaN -> 0), then bilinear:
//               (p00 (1 - wx) + p01 wx) (1 - wy) + (p10 (1 - wx) + p11 wx) wy per channel, wx = sx - floor(sx).  The
//               weights are never outside [0, 1) by more than a rounding, so a level stays within 0..255.
//   pixel       n x n sub-samples at offsets (a + 0.5) / n - 0.5 of the output index, summed in row-major order (y outer) and
//               divided by n n; n = min(8, ceil(max(W / W', H / H'))): 1 unless the output is smaller than the source.
//
// All of it is float32, every operation rounded on its own (compiled with -ffp-contract=off), no transcendentals.
#ifndef TINYSPLAT_UNDISTORT_MATH_H
#define TINYSPLAT_UNDISTORT_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_UD_HD __host__ __device__ inline
#else
#define TS_UD_HD inline
#endif

#define TS_UD_MAX_SUPERSAMPLE 8

// COLMAP camera models (the ids of cameras.bin) that the distortion above covers
#define TS_UD_SIMPLE_PINHOLE 0
#define TS_UD_PINHOLE 1
#define TS_UD_SIMPLE_RADIAL 2
#define TS_UD_RADIAL 3
#define TS_UD_OPENCV 4
#define TS_UD_FULL_OPENCV 6

// what one launch needs: source and destination intrinsics (fx fy cx cy), the coefficients, the two sizes
struct ts_undistort_params {
    float src_k[4];
    float dst_k[4];
    float d[8];
    int32_t src_h, src_w;
    int32_t out_h, out_w;
    int32_t n;   // sub-samples per axis
};

// the parameters of a COLMAP camera after its focal lengths and principal point -> d[8]; 0, or -1 for another model
TS_UD_HD int ts_undistort_coefficients(int model, const double* extra, double d[8]) {
    for (int i = 0; i < 8; ++i) d[i] = 0.0;
    int count;
    switch (model) {
        case TS_UD_SIMPLE_PINHOLE:
        case TS_UD_PINHOLE: count = 0; break;
        case TS_UD_SIMPLE_RADIAL: count = 1; break;
        case TS_UD_RADIAL: count = 2; break;
        case TS_UD_OPENCV: count = 4; break;
        case TS_UD_FULL_OPENCV: count = 8; break;
        default: return -1;
    }
    for (int i = 0; i < count; ++i) d[i] = extra[i];
    return 0;
}

TS_UD_HD int ts_undistort_supersample(int src_w, int src_h, int out_w, int out_h) {
    const int nx = (src_w + out_w - 1) / out_w, ny = (src_h + out_h - 1) / out_h;
    const int n = nx > ny ? nx : ny;
    return n > TS_UD_MAX_SUPERSAMPLE ? TS_UD_MAX_SUPERSAMPLE : n;
}

// the radial factor is formed as 1 + delta, delta = (a - b) / (1 + b) with a and b the two polynomials less their 1, and
// added to x last: 1 + a, 1 + b and their quotient would each be rounded at the size of 1 (6e-8, times |x| fx pixels),
// the small terms are rounded at their own size
TS_UD_HD void ts_undistort_distort(const float d[8], float x, float y, float* xd, float* yd) {
    const float xx = x * x, yy = y * y;
    const float r2 = xx + yy;
    const float a = r2 * (d[0] + r2 * (d[1] + r2 * d[4]));
    const float b = r2 * (d[5] + r2 * (d[6] + r2 * d[7]));
    const float delta = (a - b) / (1.0f + b);
    const float xy2 = 2.0f * (x * y);
    *xd = x + ((x * delta + d[2] * xy2) + d[3] * (r2 + 2.0f * xx));
    *yd = y + ((y * delta + d[2] * (r2 + 2.0f * yy)) + d[3] * xy2);
}

// a + b as the rounded sum and its rounding error (Knuth's two-sum: exact, and kept by a build without contraction or
// fast-math)
TS_UD_HD void ts_undistort_two_sum(float a, float b, float* s, float* e) {
    const float sum = a + b;
    const float bb = sum - a;
    *s = sum;
    *e = (a - (sum - bb)) + (b - bb);
}

// destination index (u, v) -> source index, not clamped, each coordinate as two numbers: the rounded value s and the
// rounding error e of its last addition (half an ulp of a coordinate of hundreds of pixels is most of the map's error)
TS_UD_HD void ts_undistort_map(const ts_undistort_params& p, float u, float v, float* sx, float* ex, float* sy,
                               float* ey) {
    const float x = (u - p.dst_k[2]) / p.dst_k[0];
    const float y = (v - p.dst_k[3]) / p.dst_k[1];
    float xd, yd;
    ts_undistort_distort(p.d, x, y, &xd, &yd);
    ts_undistort_two_sum(p.src_k[0] * xd, p.src_k[2], sx, ex);
    ts_undistort_two_sum(p.src_k[1] * yd, p.src_k[3], sy, ey);
}

// a source coordinate s + e clamped to [0, size - 1] -> the lower index, the upper index and the upper one's weight; the
// indices lie in [0, size - 1] for every input, NaN and sizes beyond float32's integers included
TS_UD_HD void ts_undistort_weights(float s, float e, int size, int* i0, int* i1, float* w) {
    const float hi = (float)(size - 1);
    const bool inside = s > 0.0f && s < hi;
    const float c = s >= hi ? hi : (s > 0.0f ? s : 0.0f);
    const float tail = inside ? e : (s == hi ? (e < 0.0f ? e : 0.0f) : 0.0f);
    const float f = floorf(c);
    int lo = (int)f;
    lo = lo > size - 1 ? size - 1 : lo;
    float weight = (c - f) + tail;
    if (weight < 0.0f) {                        // s is a whole number and the coordinate lies just below it
        if (lo > 0) {
            lo -= 1;
            weight = weight + 1.0f;
        } else {
            weight = 0.0f;
        }
    }
    if (weight >= 1.0f && lo < size - 1) {
        lo += 1;
        weight = weight - 1.0f;
    }
    *i0 = lo;
    *i1 = lo + 1 > size - 1 ? size - 1 : lo + 1;
    *w = weight;
}

// one bilinear sample of the uint8 [H, W, 3] source at the source index of destination index (u, v), added to acc
TS_UD_HD void ts_undistort_sample(const ts_undistort_params& p, const uint8_t* src, float u, float v, float acc[3]) {
    float sx, ex, sy, ey;
    ts_undistort_map(p, u, v, &sx, &ex, &sy, &ey);
    int x0, x1, y0, y1;
    float wx, wy;
    ts_undistort_weights(sx, ex, p.src_w, &x0, &x1, &wx);
    ts_undistort_weights(sy, ey, p.src_h, &y0, &y1, &wy);
    const size_t r0 = (size_t)y0 * (size_t)p.src_w, r1 = (size_t)y1 * (size_t)p.src_w;
    const uint8_t* p00 = src + 3 * (r0 + (size_t)x0);
    const uint8_t* p01 = src + 3 * (r0 + (size_t)x1);
    const uint8_t* p10 = src + 3 * (r1 + (size_t)x0);
    const uint8_t* p11 = src + 3 * (r1 + (size_t)x1);
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    for (int c = 0; c < 3; ++c) {
        const float top = (float)p00[c] * ux + (float)p01[c] * wx;
        const float bottom = (float)p10[c] * ux + (float)p11[c] * wx;
        acc[c] = acc[c] + (top * uy + bottom * wy);
    }
}

// output pixel `index` of the flat [out_h out_w] order -> its three channels in levels (0..255), not rounded
TS_UD_HD void ts_undistort_pixel(const ts_undistort_params& p, const uint8_t* src, int32_t index, float levels[3]) {
    const int32_t v = index / p.out_w, u = index - v * p.out_w;
    const float n = (float)p.n;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int b = 0; b < p.n; ++b) {
        const float fv = (float)v + (((float)b + 0.5f) / n - 0.5f);
        for (int a = 0; a < p.n; ++a) {
            const float fu = (float)u + (((float)a + 0.5f) / n - 0.5f);
            ts_undistort_sample(p, src, fu, fv, acc);
        }
    }
    const float nn = n * n;
    for (int c = 0; c < 3; ++c) levels[c] = acc[c] / nn;
}

// the uint8 target: round half to even, clamped to 0..255
TS_UD_HD uint32_t ts_undistort_byte(float level) {
    const float r = rintf(level);
    return !(r > 0.0f) ? 0u : (r > 255.0f ? 255u : (uint32_t)(int32_t)r);
}

#endif
