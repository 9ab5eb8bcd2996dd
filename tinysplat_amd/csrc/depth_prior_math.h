// depth_prior_math.h - what the depth-prior kernels (depth_prior.hip) and a host build (tests/hostmath/
// depth_prior.cpp) share: the projection of one SfM point to a pixel, the 64-bit sort key of a projected point, the
// sampling of a stored dense map at a camera pixel, and the order-preserving integer image of a double that the weighted
// median selects on.
//
//   project   tinysplat/depth.py:80-99 in float32, every product and sum rounded on its own (compile with
//             -ffp-contract=off): xyz_cam = R xyz + t summed left to right, z, x / z, y / z,
//             px = rint(x / z * f_x + W / 2), py = rint(y / z * f_y + H / 2), rint rounding half to even (numpy's round).
//             A point is dropped when it lands outside the image, when z is not finite or z <= 0, and when its
//             reprojection error is not finite or <= 0 (the reference has neither of the last two tests)
//   key       (camera, py W + px, position in the camera's list) in 15 + 28 + 20 bits of a non-negative int64: sorted, the
//             points of one camera stay together, row-major by pixel, and the last of a (camera, pixel) run is the point the
//             reference's lil_matrix keeps.  A dropped point carries the pixel TS_DEPTH_NO_PIXEL and sorts behind its
//             camera's kept ones
//   sample    a map of the camera's size: the stored value, bit for bit; any other size: bilinear interpolation with pixel
//             centres aligned (align_corners=False) and edge clamp, float32, every operation rounded on its own
#ifndef TINYSPLAT_DEPTH_PRIOR_MATH_H
#define TINYSPLAT_DEPTH_PRIOR_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TS_DEPTH_HD __host__ __device__ inline
#else
#define TS_DEPTH_HD inline
#endif

#define TS_DEPTH_POS_BITS 20                 // at most 2^20 visible points per camera
#define TS_DEPTH_PIXEL_BITS 28               // images below 2^28 - 1 pixels
#define TS_DEPTH_CAMERA_BITS 15              // at most 2^15 cameras per batch
#define TS_DEPTH_NO_PIXEL ((int64_t)((1 << TS_DEPTH_PIXEL_BITS) - 1))
#define TS_DEPTH_CAM_FLOATS 14               // a camera's float row: the view matrix's 3 x 4 top (row-major), f_x, f_y
#define TS_DEPTH_FIT_DOUBLES 6               // a fit's row: {s, t, f(s, t), m, evaluations, status}

// the status of a fit
#define TS_DEPTH_FIT_OK 0                    // the derivative test stopped the search: (s, t) is a minimiser
#define TS_DEPTH_FIT_ADJACENT 1              // lo and hi became adjacent doubles: the better end
#define TS_DEPTH_FIT_EQUAL_X 2               // all x equal (m = 1 included): s = 1, t = the weighted median of y - x
#define TS_DEPTH_FIT_NO_POINTS 3             // m = 0: no fit, s = t = f = NaN
#define TS_DEPTH_FIT_BRACKET_CAP 4           // the bracket's doublings ran out: the last point tried
#define TS_DEPTH_FIT_NOT_FINITE 5            // a sampled value or a sum is not finite: no fit, s = t = f = NaN

TS_DEPTH_HD int64_t ts_depth_key(int32_t camera, int64_t pixel, int32_t position) {
    return ((int64_t)camera << (TS_DEPTH_PIXEL_BITS + TS_DEPTH_POS_BITS)) | (pixel << TS_DEPTH_POS_BITS) | (int64_t)position;
}
TS_DEPTH_HD int64_t ts_depth_key_pixel(int64_t key) { return (key >> TS_DEPTH_POS_BITS) & TS_DEPTH_NO_PIXEL; }
TS_DEPTH_HD int32_t ts_depth_key_camera(int64_t key) { return (int32_t)(key >> (TS_DEPTH_PIXEL_BITS + TS_DEPTH_POS_BITS)); }
TS_DEPTH_HD int64_t ts_depth_key_run(int64_t key) { return key >> TS_DEPTH_POS_BITS; }          // (camera, pixel)

// cam: TS_DEPTH_CAM_FLOATS floats; -> the pixel index py W + px and *z, or TS_DEPTH_NO_PIXEL for a dropped point
TS_DEPTH_HD int64_t ts_depth_project(const float* cam, int32_t width, int32_t height, float x, float y, float z,
                                     double error, float* z_out) {
    const float xc = cam[0] * x + cam[1] * y + cam[2] * z + cam[3];
    const float yc = cam[4] * x + cam[5] * y + cam[6] * z + cam[7];
    const float zc = cam[8] * x + cam[9] * y + cam[10] * z + cam[11];
    *z_out = zc;
    if (!(zc > 0.0f) || !(zc <= 3.402823466e38f)) return TS_DEPTH_NO_PIXEL;
    if (!(error > 0.0) || !(error <= 1.7976931348623157e308)) return TS_DEPTH_NO_PIXEL;
    const float px = rintf(xc / zc * cam[12] + (float)width / 2.0f);
    const float py = rintf(yc / zc * cam[13] + (float)height / 2.0f);
    if (!(px >= 0.0f && px < (float)width && py >= 0.0f && py < (float)height)) return TS_DEPTH_NO_PIXEL;
    return (int64_t)py * width + (int64_t)px;
}

// the dense map [h, w] at pixel (u, v) of a camera of width x height pixels
TS_DEPTH_HD float ts_depth_sample_dense(const float* map, int32_t h, int32_t w, int32_t height, int32_t width, int32_t u,
                                        int32_t v) {
    if (h == height && w == width) return map[(int64_t)v * w + u];
    float fx = ((float)u + 0.5f) * ((float)w / (float)width) - 0.5f;
    float fy = ((float)v + 0.5f) * ((float)h / (float)height) - 0.5f;
    fx = fx < 0.0f ? 0.0f : (fx > (float)(w - 1) ? (float)(w - 1) : fx);
    fy = fy < 0.0f ? 0.0f : (fy > (float)(h - 1) ? (float)(h - 1) : fy);
    const int32_t x0 = (int32_t)fx, y0 = (int32_t)fy;                      // floor: both are >= 0
    const int32_t x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const float a = fx - (float)x0, b = fy - (float)y0;
    const float top = (1.0f - a) * map[(int64_t)y0 * w + x0] + a * map[(int64_t)y0 * w + x1];
    const float bottom = (1.0f - a) * map[(int64_t)y1 * w + x0] + a * map[(int64_t)y1 * w + x1];
    return (1.0f - b) * top + b * bottom;
}

// a double (not NaN) -> an unsigned integer of the same order; -0 and +0 share an image
TS_DEPTH_HD uint64_t ts_depth_order_key(double r) {
    r += 0.0;
    uint64_t u;
    memcpy(&u, &r, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
TS_DEPTH_HD double ts_depth_order_value(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double r;
    memcpy(&r, &u, sizeof r);
    return r;
}

// the scale-matched target of one pixel from the sampled dense value: one float32 rounding of the double expression
TS_DEPTH_HD float ts_depth_apply(double s, double t, float dense, int32_t disparity) {
    const double v = s * (double)dense + t;
    return (float)(disparity ? 1.0 / v : v);
}

#endif  // TINYSPLAT_DEPTH_PRIOR_MATH_H
