// extract.hip - SuGaR level-set surface points from depth renders (model_gaussian.py:401-460, scene.py:165-192),
// DESIGN.md section 6f.
//
//   pack      once per extraction, one thread per Gaussian: the 10-float record {mean, the six entries of the upper
//             triangular U with Sigma^-1 = U^T U, sigmoid(o)} and |exp(s)|.  Sigma^-1 = R diag(exp(-2 s)) R^T and its
//             Cholesky factor are evaluated in double and rounded once: q = |U (p - mu)|^2 has no cancellation between
//             large entries of a flat Gaussian's Sigma^-1 and cannot go negative.  The march gathers 40 B per
//             neighbour and rebuilds no rotation per pair.
//   rays      one thread per pixel: the reference's back-projection (z_ndc, inverse(P V), divide by w), a validity
//             flag and the unit ray direction.  An empty pixel gets the anchor (the first mean) as its point and a zero
//             direction: every value handed on to the neighbour search is finite and finds its neighbours in the
//             first grid cell instead of falling back to the brute-force search from far outside the model.
//   samples   after the k = 1 search: |exp(s)| of the nearest Gaussian and the S sample positions of every ray
//   march     a wave takes floor(64 / S) rays x S samples (3 x 21 = 63 lanes): each lane sums the density of one
//             sample over its 16 neighbours; one ballot of d > level gives every ray's first crossing from its S-bit
//             field, the two bracketing densities come by lane shuffle (no LDS, no second pass)
//   normals   one thread per surviving point: -grad d / |grad d| over the point's own 16 neighbours
// Plain stores, no atomics: every output is a fixed function of the inputs.  The record layout, pack's rotation and the
// march's density_at live in density_field.h, which mesh.hip shares.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "density_field.h"
#include "host_util.h"

#ifndef TS_PIX_OFF
#define TS_PIX_OFF 0.0f
#endif

namespace {

constexpr int kThreads = 256;

struct RayCam {
    float inv[16];      // inverse(P V), row-major
    float pos[3];       // camera position
    float p22, p23;
};

__global__ __launch_bounds__(kThreads) void pack_kernel(int n, const float* __restrict__ means,
                                                        const float* __restrict__ scales,
                                                        const float* __restrict__ quats, const float* __restrict__ opac,
                                                        float* __restrict__ records, float* __restrict__ pstd) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double R[3][3];
    quat_rotation(quats[i * 4], quats[i * 4 + 1], quats[i * 4 + 2], quats[i * 4 + 3], R);
    double iv[3];
    float es[3];
    for (int c = 0; c < 3; ++c) {
        const float s = scales[i * 3 + c];
        es[c] = expf(s);
        iv[c] = exp(-2.0 * (double)s);
    }
    double A[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            A[a][b] = (R[a][0] * iv[0]) * R[b][0] + (R[a][1] * iv[1]) * R[b][1] + (R[a][2] * iv[2]) * R[b][2];
    // A = U^T U, U upper triangular; a pivot that is not positive (a degenerate quaternion) zeroes its row
    double U[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
    for (int r = 0; r < 3; ++r) {
        double d = A[r][r];
        for (int k = 0; k < r; ++k) d -= U[k][r] * U[k][r];
        if (!(d > 0.) || !isfinite(d)) continue;
        const double u = sqrt(d);
        U[r][r] = u;
        for (int c = r + 1; c < 3; ++c) {
            double v = A[r][c];
            for (int k = 0; k < r; ++k) v -= U[k][r] * U[k][c];
            U[r][c] = v / u;
        }
    }
    float* rec = records + i * kRec;
    for (int c = 0; c < 3; ++c) rec[c] = means[i * 3 + c];
    rec[3] = (float)U[0][0]; rec[4] = (float)U[0][1]; rec[5] = (float)U[0][2];
    rec[6] = (float)U[1][1]; rec[7] = (float)U[1][2]; rec[8] = (float)U[2][2];
    rec[9] = 1.f / (1.f + expf(-opac[i]));
    pstd[i] = sqrtf((es[0] * es[0] + es[1] * es[1]) + es[2] * es[2]);    // exp(scales).norm(dim=-1)
}

__global__ __launch_bounds__(kThreads) void rays_kernel(int m, int H, int W, int convention, RayCam cam,
                                                        const int64_t* __restrict__ pixel_ids,
                                                        const float* __restrict__ depth,
                                                        const float* __restrict__ anchor, float* __restrict__ p_world,
                                                        float* __restrict__ dirs, int32_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const int64_t f = pixel_ids[i];
    const int64_t hw = (int64_t)H * W;
    bool ok = f >= 0 && f < hw;
    const float fill[3] = {anchor[0], anchor[1], anchor[2]};
    float p[3] = {fill[0], fill[1], fill[2]};
    float d[3] = {0.f, 0.f, 0.f};
    if (ok) {
        const float z = depth[f];
        ok = z > 0.f && isfinite(z);
        if (ok) {
            float nx, ny;
            if (convention == TS_EXTRACT_PIX_SCREEN) {
                const float col = (float)(f % W), row = (float)(f / W);
                nx = (((col + 0.5f) + TS_PIX_OFF) - (float)W / 2.f) * 2.f / (float)W;
                ny = (((row + 0.5f) + TS_PIX_OFF) - (float)H / 2.f) * 2.f / (float)H;
            } else {
                // model_gaussian.py:417-419 and scene.py:183-186 as they stand: x = f % H, y = f // H, x is divided by
                // the height and y by the width, c = size // 2
                const float px = (float)(f % H), py = (float)(f / H);
                nx = ((px + 0.5f) - (float)(W / 2)) / (float)H * 2.f;
                ny = ((py + 0.5f) - (float)(H / 2)) / (float)W * 2.f;
            }
            const float nz = (cam.p22 * z + cam.p23) / z;
            float h[4];
            for (int r = 0; r < 4; ++r)
                h[r] = ((cam.inv[r * 4] * nx + cam.inv[r * 4 + 1] * ny) + cam.inv[r * 4 + 2] * nz) + cam.inv[r * 4 + 3];
            const float wx = h[0] / h[3], wy = h[1] / h[3], wz = h[2] / h[3];
            ok = isfinite(wx) && isfinite(wy) && isfinite(wz);
            if (ok) {
                p[0] = wx; p[1] = wy; p[2] = wz;
                const float e0 = wx - cam.pos[0], e1 = wy - cam.pos[1], e2 = wz - cam.pos[2];
                const float len = fmaxf(sqrtf((e0 * e0 + e1 * e1) + e2 * e2), 1e-12f);     // F.normalize
                d[0] = e0 / len; d[1] = e1 / len; d[2] = e2 / len;
                ok = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
                if (!ok) {
                    for (int c = 0; c < 3; ++c) { p[c] = fill[c]; d[c] = 0.f; }
                }
            }
        }
    }
    for (int c = 0; c < 3; ++c) {
        p_world[i * 3 + c] = p[c];
        dirs[i * 3 + c] = d[c];
    }
    valid[i] = ok ? 1 : 0;
}

// torch.linspace(-e, e, S) in float32: from the start in the first half, from the end in the second
__device__ __forceinline__ float lin_at(int s, int S, float extent) {
    const float step = (extent - (-extent)) / (float)(S - 1);
    return s < S / 2 ? -extent + step * (float)s : extent - step * (float)(S - 1 - s);
}

__global__ __launch_bounds__(kThreads) void samples_kernel(int n, int m, int S, float extent,
                                                           const float* __restrict__ p_world,
                                                           const float* __restrict__ dirs,
                                                           const int32_t* __restrict__ nearest,
                                                           const float* __restrict__ pstd_table,
                                                           float* __restrict__ p_std, float* __restrict__ samples) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)m * S) return;
    const int64_t i = e / S;
    const int s = (int)(e - i * S);
    const int32_t j = nearest[i];
    const float sd = (j >= 0 && j < n) ? pstd_table[j] : 0.f;
    if (s == 0) p_std[i] = sd;
    const float t = lin_at(s, S, extent) * sd;
    for (int c = 0; c < 3; ++c) samples[e * 3 + c] = p_world[i * 3 + c] + t * dirs[i * 3 + c];
}

__global__ __launch_bounds__(kThreads) void march_kernel(int n, int m, int S, int rpw, float extent, float level,
                                                         const float* __restrict__ samples,
                                                         const int32_t* __restrict__ knn,
                                                         const float* __restrict__ records,
                                                         const float* __restrict__ p_world,
                                                         const float* __restrict__ dirs, const float* __restrict__ p_std,
                                                         const int32_t* __restrict__ valid, int32_t* __restrict__ keep,
                                                         int32_t* __restrict__ first, float* __restrict__ t_out,
                                                         float* __restrict__ points, float* __restrict__ density) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int slot = lane / S;                      // the wave's ray this lane works for
    const int s = lane - slot * S;
    const int64_t ray = wave * rpw + slot;
    const bool live = slot < rpw && ray < m;
    float d = 0.f;
    if (live) {
        const int64_t e = ray * S + s;
        const float p[3] = {samples[e * 3], samples[e * 3 + 1], samples[e * 3 + 2]};
        d = density_at(n, p, knn + e * kK, records);
        if (density) density[e] = d;
    }
    // every lane of the wave takes part in the ballot and the shuffles
    const unsigned long long above = __ballot(live && d > level);
    const int base = slot < rpw ? slot * S : 0;
    const unsigned long long mask = S >= 64 ? ~0ull : ((1ull << S) - 1ull);
    const unsigned long long field = (above >> base) & mask;
    const int fi = field ? __builtin_ctzll(field) : 0;          // torch max over bools: the first True, 0 if none
    const float d0 = __shfl(d, base);
    const float da = __shfl(d, base + fi);
    const float db = __shfl(d, base + (fi > 0 ? fi - 1 : 0));
    if (!live || s != 0) return;
    const bool kept = valid[ray] != 0 && d0 < level && fi >= 1;
    keep[ray] = kept ? 1 : 0;
    first[ray] = fi;
    float t = 0.f, pt[3] = {0.f, 0.f, 0.f};
    if (kept) {
        const float sd = p_std[ray];
        const float ta = lin_at(fi, S, extent) * sd, tb = lin_at(fi - 1, S, extent) * sd;
        t = (level - db) / (da - db) * (ta - tb) + tb;
        for (int c = 0; c < 3; ++c) pt[c] = p_world[ray * 3 + c] + t * dirs[ray * 3 + c];
    }
    t_out[ray] = t;
    for (int c = 0; c < 3; ++c) points[ray * 3 + c] = pt[c];
}

__global__ __launch_bounds__(kThreads) void normals_kernel(int n, int m, const float* __restrict__ points,
                                                           const int32_t* __restrict__ knn,
                                                           const float* __restrict__ records,
                                                           float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    float dsum = 0.f, g[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < kK; ++k) {
        const int j = knn[i * kK + k];
        if (j < 0 || j >= n) continue;
        const float* r = records + (int64_t)j * kRec;
        const float dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
        const float y0 = (r[3] * dx + r[4] * dy) + r[5] * dz;
        const float y1 = r[6] * dy + r[7] * dz;
        const float y2 = r[8] * dz;
        const float q = (y0 * y0 + y1 * y1) + y2 * y2;
        if (!(q == q)) continue;                    // as in the march: no contribution
        const float e = r[9] * expf(-0.5f * fminf(fmaxf(q, 0.f), 1e8f));
        dsum += e;
        if (q > 1e8f) continue;                     // the clamp passes no gradient outside [0, 1e8]
        // grad q = 2 U^T (U dl); d/dp of sigmoid(o) exp(-q / 2) = -e U^T y
        g[0] += -e * (r[3] * y0);
        g[1] += -e * (r[4] * y0 + r[6] * y1);
        g[2] += -e * ((r[5] * y0 + r[7] * y1) + r[8] * y2);
    }
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const bool zero = dsum > 1.f || !(len > 0.f) || !isfinite(len);
    for (int c = 0; c < 3; ++c) normals[i * 3 + c] = zero ? 0.f : -g[c] / len;
}

inline bool steps_ok(int32_t S) { return S >= 2 && S <= TS_EXTRACT_MAX_STEPS; }

}  // namespace

extern "C" {

int ts_extract_pack(int32_t n, const float* means, const float* scales, const float* quats, const float* opacities,
                    float* records, float* p_std, void* stream) {
    if (n < 1 || !means || !scales || !quats || !opacities || !records || !p_std) return TS_E_BADARG;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, means, scales, quats, opacities, records, p_std);
    return launch_status();
}

int ts_extract_rays(int32_t m, const int64_t* pixel_ids, int32_t height, int32_t width, const float* depth,
                    int32_t convention, const float* camera_host, const float* anchor, float* p_world, float* dirs,
                    int32_t* valid, void* stream) {
    if (m < 1 || height < 1 || width < 1 || (int64_t)height * width >= INT32_MAX) return TS_E_BADARG;
    if (convention != TS_EXTRACT_PIX_REFERENCE && convention != TS_EXTRACT_PIX_SCREEN) return TS_E_BADARG;
    if (!pixel_ids || !depth || !camera_host || !anchor || !p_world || !dirs || !valid) return TS_E_BADARG;
    RayCam cam;
    for (int c = 0; c < 16; ++c) cam.inv[c] = camera_host[c];
    for (int c = 0; c < 3; ++c) cam.pos[c] = camera_host[16 + c];
    cam.p22 = camera_host[19];
    cam.p23 = camera_host[20];
    for (int c = 0; c < TS_EXTRACT_CAMERA_FLOATS; ++c)
        if (!isfinite(camera_host[c])) return TS_E_BADARG;
    hipLaunchKernelGGL(rays_kernel, dim3((unsigned)nblocks(m, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)m, (int)height, (int)width, (int)convention, cam, pixel_ids, depth, anchor, p_world, dirs,
                       valid);
    return launch_status();
}

int ts_extract_samples(int32_t n, int32_t m, int32_t steps, float extent_sigmas, const float* p_world, const float* dirs,
                       const int32_t* nearest, const float* p_std_table, float* p_std, float* samples, void* stream) {
    if (n < 1 || m < 1 || !steps_ok(steps) || (int64_t)m * steps >= INT32_MAX) return TS_E_BADARG;
    if (!(extent_sigmas > 0.f) || !isfinite(extent_sigmas)) return TS_E_BADARG;
    if (!p_world || !dirs || !nearest || !p_std_table || !p_std || !samples) return TS_E_BADARG;
    hipLaunchKernelGGL(samples_kernel, dim3((unsigned)nblocks((int64_t)m * steps, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (int)n, (int)m, (int)steps, extent_sigmas, p_world, dirs, nearest, p_std_table,
                       p_std, samples);
    return launch_status();
}

int ts_extract_march(int32_t n, int32_t m, int32_t steps, float extent_sigmas, float level, const float* samples,
                     const int32_t* knn, const float* records, const float* p_world, const float* dirs,
                     const float* p_std, const int32_t* valid, int32_t* keep, int32_t* first, float* t, float* points,
                     float* density, void* stream) {
    if (n < 1 || m < 1 || !steps_ok(steps) || (int64_t)m * steps >= INT32_MAX) return TS_E_BADARG;
    if (!(extent_sigmas > 0.f) || !isfinite(extent_sigmas) || !isfinite(level)) return TS_E_BADARG;
    if (!samples || !knn || !records || !p_world || !dirs || !p_std || !valid || !keep || !first || !t || !points)
        return TS_E_BADARG;
    const int rpw = 64 / steps;
    const int64_t waves = ((int64_t)m + rpw - 1) / rpw;
    const int64_t blocks = (waves + kThreads / 64 - 1) / (kThreads / 64);
    hipLaunchKernelGGL(march_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (int)n, (int)m,
                       (int)steps, rpw, extent_sigmas, level, samples, knn, records, p_world, dirs, p_std, valid, keep,
                       first, t, points, density);
    return launch_status();
}

int ts_extract_normals(int32_t n, int32_t m, const float* points, const int32_t* knn, const float* records,
                       float* normals, void* stream) {
    if (n < 1 || m < 1 || !points || !knn || !records || !normals) return TS_E_BADARG;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)nblocks(m, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, (int)m, points, knn, records, normals);
    return launch_status();
}

int64_t ts_extract_chunk_bytes(int32_t n, int32_t rays, int32_t steps) {
    if (n < TS_EXTRACT_K || rays < 1 || !steps_ok(steps) || (int64_t)rays * steps >= INT32_MAX) return TS_E_BADARG;
    const int64_t knn_ws = ts_knn_ws_bytes(n, (int32_t)((int64_t)rays * steps), TS_EXTRACT_K);
    if (knn_ws < 0) return TS_E_BADARG;
    const int64_t r = rays, e = (int64_t)rays * steps;
    // p_world, dirs, points | valid, keep, first, nearest, p_std, t, nearest's distance | samples | knn dist, idx
    return knn_ws + 3 * align256(r * 12) + 7 * align256(r * 4) + align256(e * 12) +
           2 * align256(e * TS_EXTRACT_K * 4);
}

}  // extern "C"
