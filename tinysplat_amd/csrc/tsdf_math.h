// tsdf_math.h - what the fusion kernels (tsdf.hip) and a host build (tests/hostmath/tsdf.cpp)
// share: a camera's row of the device table, the pixel and the observation of one (corner, camera) pair, the
// conservative test of a brick's bounding sphere against a camera, and the world point of a pixel corner at a depth.
//
//   observe   float32, every product and sum rounded on its own (compile with -ffp-contract=off).  z is the third row of
//             the view matrix times the corner, summed left to right as project_mid of splat_math.h sums it; the pixel is
//             project_one's: hx, hy, hw from rows 0, 1, 3 of proj @ view, rw = 1 / (hw + 1e-6), u = ((W / 2) (hx rw) + c_x) -
//             0.5 with c_x = W / 2 (what the rasteriser hands the projection), likewise v; px = rint(u), py = rint(v), half
//             to even.  Then d = depth[py, px], s = d - z, t = min(1, s / trunc).
//   cull      six planes per camera, written by the host in double and rounded to float32: {n, d, |n|} each.  A plane
//             functional L(x) = n . x + d reaches at most L(c) + |n| r over a sphere (c, r).  Plane 0 is z itself, plane 1
//             is hw; planes 2..5 are k (hw + 1e-6) +- hx and +- hy with k = 1.125: where hw + 1e-6 > 0, a pixel inside
//             the image has all four non-negative with an eighth of the image to spare.  The sphere is skipped when z cannot
//             exceed znear on it, or when hw is positive all over it and one of the four is negative all over it.  Every
//             comparison leaves kCullSlack of the functional's summed magnitudes: 2^10 times the float32 rounding of
//             either side's evaluation.
//   unproject the world point x with (PV_0 - n_x PV_3) . x~ = n_x 1e-6, (PV_1 - n_y PV_3) . x~ = n_y 1e-6, V_2 . x~ = z
//             for a pixel position (u, v) (n_x = (u + 0.5 - W / 2) 2 / W: the inverse of `observe`'s u), by Cramer's rule
//             in double: the very functionals `observe` evaluates, so a corner that rounds to a pixel lies in the cone of
//             that pixel's four corner rays.
#ifndef TINYSPLAT_TSDF_MATH_H
#define TINYSPLAT_TSDF_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_TSDF_HD __host__ __device__ inline
#else
#define TS_TSDF_HD inline
#endif

#define TS_TSDF_PLANES 6
#define TS_TSDF_PLANE_FLOATS 5          /* n xyz, d, |n| */

// one camera of the device table (tinysplat_amd/_lib.py: TsTsdfCamera mirrors it)
struct ts_tsdf_camera {
    float view[12];                     // the view matrix's 3 x 4 top, row-major
    float proj[12];                     // rows 0, 1 and 3 of proj @ view
    float planes[TS_TSDF_PLANES * TS_TSDF_PLANE_FLOATS];
    int32_t width, height;
    const float* depth;                 // float32 [height, width], view-space z; not finite or <= 0: no depth
};

constexpr float kTsdfCullSlack = 1.0f / 16384.0f;       // 2^-14 = 2^10 * 2^-24

// no depth: not finite, or <= 0
TS_TSDF_HD bool ts_tsdf_valid_depth(float d) { return d > 0.0f && d <= 3.402823466e38f; }

// -> the flat pixel py W + px of corner x in camera c and *z_out, or -1 when steps 1 and 2 of section 6p skip the pair
TS_TSDF_HD int64_t ts_tsdf_pixel(const ts_tsdf_camera& c, const float x[3], float znear, float* z_out) {
    const float* V = c.view;
    const float z = ((V[8] * x[0] + V[9] * x[1]) + V[10] * x[2]) + V[11];
    *z_out = z;
    if (!(z > znear)) return -1;
    const float* P = c.proj;
    const float hx = ((P[0] * x[0] + P[1] * x[1]) + P[2] * x[2]) + P[3];
    const float hy = ((P[4] * x[0] + P[5] * x[1]) + P[6] * x[2]) + P[7];
    const float hw = ((P[8] * x[0] + P[9] * x[1]) + P[10] * x[2]) + P[11];
    const float rw = 1.0f / (hw + 1e-6f);
    const float half_w = 0.5f * (float)c.width, half_h = 0.5f * (float)c.height;
    const float u = rintf((half_w * (hx * rw) + half_w) - 0.5f);
    const float v = rintf((half_h * (hy * rw) + half_h) - 0.5f);
    if (!(u >= 0.0f && u < (float)c.width && v >= 0.0f && v < (float)c.height)) return -1;
    return (int64_t)v * c.width + (int64_t)u;
}

// steps 3 to 5: the observation of a pair whose pixel holds d -> true and *t, or false when the pair is skipped
TS_TSDF_HD bool ts_tsdf_observe(float d, float z, float trunc, float depth_max, float* t) {
    if (!ts_tsdf_valid_depth(d) || d > depth_max) return false;
    const float s = d - z;
    if (s < -trunc) return false;
    *t = fminf(1.0f, s / trunc);
    return true;
}

// true when no corner inside the sphere (centre, radius) can pass steps 1 and 2 for camera c
TS_TSDF_HD bool ts_tsdf_cull(const ts_tsdf_camera& c, const float centre[3], float radius, float znear) {
    float top[TS_TSDF_PLANES], low1 = 0.0f, mag1 = 0.0f;
    float mag[TS_TSDF_PLANES];
    for (int p = 0; p < TS_TSDF_PLANES; ++p) {
        const float* q = c.planes + p * TS_TSDF_PLANE_FLOATS;
        const float a = q[0] * centre[0], b = q[1] * centre[1], e = q[2] * centre[2];
        const float at = ((a + b) + e) + q[3];
        mag[p] = (((fabsf(a) + fabsf(b)) + fabsf(e)) + fabsf(q[3])) + q[4] * radius;
        top[p] = at + q[4] * radius;
        if (p == 1) {
            low1 = at - q[4] * radius;
            mag1 = mag[p];
        }
    }
    if (top[0] < znear - kTsdfCullSlack * (mag[0] + fabsf(znear))) return true;          // z <= znear everywhere
    if (!(low1 > kTsdfCullSlack * mag1)) return false;                                    // hw may not be positive
    for (int p = 2; p < TS_TSDF_PLANES; ++p)
        if (top[p] < -kTsdfCullSlack * mag[p]) return true;                               // past one side everywhere
    return false;
}

// the world point on the ray of pixel position (u, v) at view depth z -> false when the three planes do not meet
TS_TSDF_HD bool ts_tsdf_unproject(const ts_tsdf_camera& c, double u, double v, double z, double out[3]) {
    const double nx = (u + 0.5 - 0.5 * (double)c.width) * 2.0 / (double)c.width;
    const double ny = (v + 0.5 - 0.5 * (double)c.height) * 2.0 / (double)c.height;
    const float* P = c.proj;
    const float* V = c.view;
    const double eps = (double)1e-6f;
    double a0[3], a1[3], a2[3];
    for (int k = 0; k < 3; ++k) {
        a0[k] = (double)P[k] - nx * (double)P[8 + k];
        a1[k] = (double)P[4 + k] - ny * (double)P[8 + k];
        a2[k] = (double)V[8 + k];
    }
    const double b0 = nx * (eps + (double)P[11]) - (double)P[3];
    const double b1 = ny * (eps + (double)P[11]) - (double)P[7];
    const double b2 = z - (double)V[11];
    const double c0[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
    const double c1[3] = {a2[1] * a0[2] - a2[2] * a0[1], a2[2] * a0[0] - a2[0] * a0[2], a2[0] * a0[1] - a2[1] * a0[0]};
    const double c2[3] = {a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]};
    const double det = a0[0] * c0[0] + a0[1] * c0[1] + a0[2] * c0[2];
    if (!(fabs(det) > 0.0) || !(fabs(det) <= 1.7976931348623157e308)) return false;
    for (int k = 0; k < 3; ++k) out[k] = (b0 * c0[k] + b1 * c1[k] + b2 * c2[k]) / det;
    return isfinite(out[0]) && isfinite(out[1]) && isfinite(out[2]);
}

#endif  // TINYSPLAT_TSDF_MATH_H
