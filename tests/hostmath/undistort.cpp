// Host build of csrc/undistort_math.h for tests/test_undistort_cpu.py: the functions the kernel of csrc/undistort.hip
// calls, behind a C interface (compiled with -ffp-contract=off, as the kernel is).
#include "../../tinysplat_amd/csrc/undistort_math.h"

namespace {

ts_undistort_params params(const float* src_k, const float* dst_k, const float* d, int src_h, int src_w, int out_h,
                           int out_w) {
    ts_undistort_params p;
    for (int i = 0; i < 4; ++i) {
        p.src_k[i] = src_k[i];
        p.dst_k[i] = dst_k[i];
    }
    for (int i = 0; i < 8; ++i) p.d[i] = d[i];
    p.src_h = src_h;
    p.src_w = src_w;
    p.out_h = out_h;
    p.out_w = out_w;
    p.n = ts_undistort_supersample(src_w, src_h, out_w, out_h);
    return p;
}

}  // namespace

extern "C" {

// a COLMAP camera's parameters after the focal lengths and the principal point -> d [8]; -1: a model not covered
int ud_coefficients(int model, const double* extra, double* d) { return ts_undistort_coefficients(model, extra, d); }

int ud_supersample(int src_w, int src_h, int out_w, int out_h) {
    return ts_undistort_supersample(src_w, src_h, out_w, out_h);
}

// normalised points -> distorted normalised points
void ud_distort(int64_t n, const float* d, const float* x, const float* y, float* xd, float* yd) {
    for (int64_t i = 0; i < n; ++i) ts_undistort_distort(d, x[i], y[i], xd + i, yd + i);
}

// destination indices -> unclamped source indices, each as a rounded value and the rounding error of its last addition
void ud_map(int64_t n, const float* src_k, const float* dst_k, const float* d, const float* u, const float* v, float* sx,
            float* ex, float* sy, float* ey) {
    const ts_undistort_params p = params(src_k, dst_k, d, 1, 1, 1, 1);
    for (int64_t i = 0; i < n; ++i) ts_undistort_map(p, u[i], v[i], sx + i, ex + i, sy + i, ey + i);
}

// source coordinates s + e -> lower index, upper index, upper weight
void ud_weights(int64_t n, const float* s, const float* e, int size, int32_t* i0, int32_t* i1, float* w) {
    for (int64_t i = 0; i < n; ++i) {
        int a, b;
        ts_undistort_weights(s[i], e[i], size, &a, &b, w + i);
        i0[i] = a;
        i1[i] = b;
    }
}

// the whole image, as the kernel writes it: levels float32 [out_h, out_w, 3] (not rounded) and bytes uint8 of the same shape
void ud_remap(const uint8_t* src, int src_h, int src_w, const float* src_k, const float* dst_k, const float* d, int out_h,
              int out_w, float* levels, uint8_t* bytes) {
    const ts_undistort_params p = params(src_k, dst_k, d, src_h, src_w, out_h, out_w);
    for (int32_t i = 0; i < out_h * out_w; ++i) {
        ts_undistort_pixel(p, src, i, levels + 3 * (size_t)i);
        for (int c = 0; c < 3; ++c) bytes[3 * (size_t)i + c] = (uint8_t)ts_undistort_byte(levels[3 * (size_t)i + c]);
    }
}

}  // extern "C"
