// field_color.hip - the colour of a point of the SuGaR density field from the spherical harmonics of its 16 nearest
// Gaussians:
//
//   colour(x) = min(sum_j w_j c_j / sum_j w_j, 1),   w_j = neighbour_weight (density_field.h: the term density_at sums),
//   c_j = max(sum_k Y_k(-n) coeffs[j, k, :] + 0.5, 0)   (rasterize.py:38-39, :45; the bands <= degree)
//
// seen head-on: the direction is -n for all 16 neighbours, n the point's unit outward normal.
//
//   colors    one 16-lane row per point, lane j taking neighbour j: 4 points per wave, 16 per workgroup.  A lane loads
//             its neighbour's 40-byte record and the coefficients of the active bands (rows of colors_rest are 4-byte
//             aligned only: dword loads), evaluates the basis for the shared direction and forms w and w c; the four
//             sums go through a fixed xor butterfly inside the row (offsets 8, 4, 2, 1: float addition commutes, so
//             every lane of the row holds the same bits) and lane 0 stores 12 bytes.  A row's result is a function of
//             its point's inputs alone: not of m, of the chunk, or of the row's place in the wave.  The rows of the
//             last workgroup past m work on point m - 1 and store nothing: whole rows stay converged in the shuffles.
// Plain stores, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "density_field.h"
#include "host_util.h"
#include "splat_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / kK;        // 16 points per workgroup

template <int DEG>
__global__ __launch_bounds__(kThreads) void field_colors_kernel(int n, int m, int k_rest,
                                                                const float* __restrict__ points,
                                                                const float* __restrict__ normals,
                                                                const int32_t* __restrict__ knn,
                                                                const float* __restrict__ records,
                                                                const float* __restrict__ colors_dc,
                                                                const float* __restrict__ colors_rest,
                                                                float* __restrict__ colors) {
    constexpr int kBases = (DEG + 1) * (DEG + 1);
    const int slot = threadIdx.x & (kK - 1);        // the neighbour this lane takes
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 4);
    const bool live = row < m;
    const int64_t i = live ? row : (int64_t)m - 1;
    const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    // the direction -n; without a usable normal (absent, zero or not finite) only band 0, and sh_basis sees +z
    float d[3] = {0.f, 0.f, 1.f};
    bool bands = false;
    if (DEG > 0 && normals) {
        const float nx = normals[i * 3], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        bands = len > 0.f && isfinite(len);          // a NaN or infinite component makes len NaN or infinite
        if (bands) { d[0] = -nx; d[1] = -ny; d[2] = -nz; }
    }
    const int j = knn[i * kK + slot];
    const bool valid = j >= 0 && j < n;
    float w = 0.f, c[3] = {0.f, 0.f, 0.f};
    if (valid) {
        w = neighbour_weight(p, records, j);
        float Y[kBases];
        ts::sh_basis(DEG, d[0], d[1], d[2], Y);
        const float* dc = colors_dc + (int64_t)j * 3;
        for (int ch = 0; ch < 3; ++ch) c[ch] = Y[0] * dc[ch];
        if (DEG > 0 && bands) {
            const float* rest = colors_rest + (int64_t)j * k_rest * 3;
#pragma unroll
            for (int k = 1; k < kBases; ++k)
                for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] + Y[k] * rest[(k - 1) * 3 + ch];
        }
        for (int ch = 0; ch < 3; ++ch) c[ch] = fmaxf(c[ch] + 0.5f, 0.f);
    }
    float s[4] = {w, w * c[0], w * c[1], w * c[2]};
#pragma unroll
    for (int off = kK / 2; off >= 1; off >>= 1)
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = s[t] + __shfl_xor(s[t], off, kK);
    if (!live || slot != 0) return;
    // no positive finite weight (a point far from every Gaussian): the colour of the first listed neighbour, which is
    // the nearest (ts_knn lists ascending in (distance, index)) and this lane's own
    const bool weighed = s[0] > 0.f && isfinite(s[0]);
    for (int ch = 0; ch < 3; ++ch) {
        const float v = weighed ? s[1 + ch] / s[0] : c[ch];
        colors[row * 3 + ch] = v > 1.f ? 1.f : v;
    }
}

}  // namespace

extern "C" {

int ts_field_colors(int32_t n, int32_t m, const float* points, const float* normals, const int32_t* knn,
                    const float* records, const float* colors_dc, const float* colors_rest, int32_t k_rest,
                    int32_t degree, float* colors, void* stream) {
    if (n < 1 || m < 0 || k_rest < 0) return TS_E_BADARG;
    if (degree < 0 || degree > 3 || (degree + 1) * (degree + 1) > (int64_t)k_rest + 1) return TS_E_DEGREE;
    if (m == 0) return 0;
    if (!points || !knn || !records || !colors_dc || !colors || (degree > 0 && !colors_rest)) return TS_E_BADARG;
    const dim3 grid((unsigned)nblocks(m, kRowsPerBlock)), block(kThreads);
    hipStream_t s = (hipStream_t)stream;
#define TS_FIELD_COLORS(D)                                                                                          \
    hipLaunchKernelGGL(field_colors_kernel<D>, grid, block, 0, s, (int)n, (int)m, (int)k_rest, points, normals, knn, \
                       records, colors_dc, colors_rest, colors)
    switch (degree) {
        case 0: TS_FIELD_COLORS(0); break;
        case 1: TS_FIELD_COLORS(1); break;
        case 2: TS_FIELD_COLORS(2); break;
        default: TS_FIELD_COLORS(3); break;
    }
#undef TS_FIELD_COLORS
    return launch_status();
}

}  // extern "C"
