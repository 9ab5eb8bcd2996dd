// density.hip - the SuGaR density regulariser of the training loop (scripts/train.py:77-91,
// model_gaussian.py:244-326), DESIGN.md section 6e.
//
//   sample (update steps)   weights a_i = prod(exp(s_i)) (or their prefix sums, the reference's quirk), an
//                           inclusive prefix in double by a fixed tree (prefix_scan.h, shared with mcmc.hip),
//                           rows by binary search of caller-supplied uniforms, p = mu + R(q/|q|) (exp(s) * xi) from caller-supplied normals xi; the values
//                           the frozen backward needs (xi, exp(s), q) are kept per sample
//   pairs (active steps)    one thread per point, two passes over its K = 16 neighbours: the density
//                           d = sum sigmoid(o_j) exp(-q_j / 2), beta, the depth fetch, |d - approx| and, per
//                           (point, neighbour), the gradient row {mu, s, q, o} of that neighbour; per point, the
//                           gradient row of its sampling source and its four bilinear depth taps.  Plain stores,
//                           no float atomics; the masked |d - approx| and the count go to one double partial per
//                           workgroup, summed by a second one-workgroup launch
//   segment sum             rows sorted by key (Gaussian row or pixel) are summed per key in chunks of kChunk,
//                           chunk partials of a key that spans chunks are added in chunk order by its first
//                           chunk: long segments (the reference projection's one border pixel) stay parallel
// Every sum has a fixed order: results are bit-identical from run to run.  Sigma^-1 = R diag(exp(-2 s)) R^T
// (exact algebra) replaces the reference's float32 3x3 inverse.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "prefix_scan.h"

#ifndef TS_PIX_OFF
#define TS_PIX_OFF 0.0f
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kK = TS_DENSITY_K;
constexpr int kRow = TS_DENSITY_ROW;                // gradient row: mu xyz | s xyz | q wxyz | opacity
constexpr int kFrozen = TS_DENSITY_FROZEN;          // per sample: xi xyz | exp(s) xyz | q wxyz
constexpr int kChunk = 128;

struct Mats {
    float v[16];    // world -> camera, row-major
    float p[16];    // camera -> clip, row-major
};

__device__ __forceinline__ void tree_sum(double* part) {
    for (int step = kThreads / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
}

// quat_to_rot_tensor (utils.py:42-64) of q / max(|q|, 1e-12) (F.normalize)
__device__ __forceinline__ void quat_rot(const float* q, float* qn, float R[3][3]) {
    const float nrm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const float den = fmaxf(nrm, 1e-12f);
    for (int c = 0; c < 4; ++c) qn[c] = q[c] / den;
    const float w = qn[0], x = qn[1], y = qn[2], z = qn[3];
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - w * z); R[0][2] = 2.f * (x * z + w * y);
    R[1][0] = 2.f * (x * y + w * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - w * x);
    R[2][0] = 2.f * (x * z - w * y); R[2][1] = 2.f * (y * z + w * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// d/dq of <G, R(q / max(|q|, 1e-12))>
__device__ __forceinline__ void quat_rot_vjp(const float* q, const float* qn, const float G[3][3], float* gq) {
    const float w = qn[0], x = qn[1], y = qn[2], z = qn[3];
    float g[4];
    g[0] = 2.f * (((-z * G[0][1] + y * G[0][2]) + (z * G[1][0] - x * G[1][2])) + (-y * G[2][0] + x * G[2][1]));
    g[1] = 2.f * (((y * G[0][1] + z * G[0][2]) + (y * G[1][0] - 2.f * x * G[1][1] - w * G[1][2])) +
                  (z * G[2][0] + w * G[2][1] - 2.f * x * G[2][2]));
    g[2] = 2.f * (((-2.f * y * G[0][0] + x * G[0][1] + w * G[0][2]) + (x * G[1][0] + z * G[1][2])) +
                  (-w * G[2][0] + z * G[2][1] - 2.f * y * G[2][2]));
    g[3] = 2.f * (((-2.f * z * G[0][0] - w * G[0][1] + x * G[0][2]) + (w * G[1][0] - 2.f * z * G[1][1] + y * G[1][2])) +
                  (x * G[2][0] + y * G[2][1]));
    const float nrm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(nrm > 1e-12f)) {                          // F.normalize's clamp: q / 1e-12, a linear map
        for (int c = 0; c < 4; ++c) gq[c] = g[c] / 1e-12f;
        return;
    }
    const float dot = ((qn[0] * g[0] + qn[1] * g[1]) + qn[2] * g[2]) + qn[3] * g[3];
    for (int c = 0; c < 4; ++c) gq[c] = (g[c] - qn[c] * dot) / nrm;
}

// ------------------------------------------------------------------ sampling
__global__ __launch_bounds__(kThreads) void weights_kernel(int n, const float* __restrict__ scales, double* __restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float e0 = expf(scales[i * 3]), e1 = expf(scales[i * 3 + 1]), e2 = expf(scales[i * 3 + 2]);
    a[i] = (double)fabsf((e0 * e1) * e2);          // torch.prod(exp(scales), -1).abs() in float32
}

__global__ __launch_bounds__(kThreads) void sample_kernel(int n, int m, const double* __restrict__ cdf,
                                                          const float* __restrict__ uniforms,
                                                          const int32_t* __restrict__ rows_in,
                                                          const float* __restrict__ normals,
                                                          const float* __restrict__ means, const float* __restrict__ scales,
                                                          const float* __restrict__ quats, int32_t* __restrict__ rows,
                                                          float* __restrict__ points, float* __restrict__ frozen) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    int r;
    if (rows_in) {
        r = rows_in[i];
    } else {
        // first row whose inclusive prefix exceeds u * total (torch.multinomial's inverse CDF)
        const double target = (double)uniforms[i] * cdf[n - 1];
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (cdf[mid] > target) hi = mid; else lo = mid + 1;
        }
        r = lo;
    }
    float* f = frozen + i * kFrozen;
    float* pt = points + i * 3;
    if (r < 0 || r >= n) {                           // a caller row out of range: no read, the sample is NaN
        rows[i] = -1;
        for (int c = 0; c < 3; ++c) pt[c] = __int_as_float(0x7fc00000);
        for (int c = 0; c < kFrozen; ++c) f[c] = __int_as_float(0x7fc00000);
        return;
    }
    const int64_t ri = r;
    float q[4], qn[4], R[3][3], es[3], xi[3];
    for (int c = 0; c < 4; ++c) q[c] = quats[ri * 4 + c];
    quat_rot(q, qn, R);
    for (int c = 0; c < 3; ++c) {
        es[c] = expf(scales[ri * 3 + c]);
        xi[c] = normals[i * 3 + c];
    }
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = xi[c] * es[c];
    for (int a = 0; a < 3; ++a) pt[a] = means[ri * 3 + a] + ((R[a][0] * v[0] + R[a][1] * v[1]) + R[a][2] * v[2]);
    rows[i] = r;
    for (int c = 0; c < 3; ++c) {
        f[c] = xi[c];
        f[3 + c] = es[c];
    }
    for (int c = 0; c < 4; ++c) f[6 + c] = q[c];
}

// ------------------------------------------------------------------ the density term
struct Neighbour {
    float mu[3], es[3], w[3], q[4], qn[4], R[3][3], dl[3], y[3];
    float qq, g, sg;
    int amin;
};

__device__ __forceinline__ void load_neighbour(int64_t j, const float* p, const float* means, const float* scales,
                                               const float* quats, const float* opac, Neighbour& nb) {
    for (int c = 0; c < 3; ++c) {
        nb.mu[c] = means[j * 3 + c];
        const float s = scales[j * 3 + c];
        nb.es[c] = expf(s);
        nb.w[c] = expf(-2.f * s);                  // 1 / exp(s)^2: Sigma^-1 = R diag(w) R^T
    }
    for (int c = 0; c < 4; ++c) nb.q[c] = quats[j * 4 + c];
    quat_rot(nb.q, nb.qn, nb.R);
    for (int c = 0; c < 3; ++c) nb.dl[c] = p[c] - nb.mu[c];
    float qq = 0.f;
    for (int a = 0; a < 3; ++a) {
        nb.y[a] = (nb.R[0][a] * nb.dl[0] + nb.R[1][a] * nb.dl[1]) + nb.R[2][a] * nb.dl[2];
        qq += (nb.y[a] * nb.y[a]) * nb.w[a];
    }
    nb.qq = qq;
    nb.g = expf(-0.5f * fminf(fmaxf(qq, 0.f), 1e8f));
    nb.sg = 1.f / (1.f + expf(-opac[j]));
    nb.amin = 0;                                   // torch min(dim): the first of equal minima
    if (nb.es[1] < nb.es[nb.amin]) nb.amin = 1;
    if (nb.es[2] < nb.es[nb.amin]) nb.amin = 2;
}

__global__ __launch_bounds__(kThreads) void pairs_kernel(
    int n, int m, int H, int W, int mode, float znear, Mats mt, const float* __restrict__ points,
    const int32_t* __restrict__ rows, const float* __restrict__ frozen, const int32_t* __restrict__ knn,
    const float* __restrict__ means, const float* __restrict__ scales, const float* __restrict__ quats,
    const float* __restrict__ opac, const float* __restrict__ depth, float* __restrict__ dens_out,
    float* __restrict__ beta_out, float* __restrict__ approx_out, uint8_t* __restrict__ mask_out,
    float* __restrict__ grows, int32_t* __restrict__ tap_key, float* __restrict__ tap_val,
    double* __restrict__ partial) {
    __shared__ double part_l[kThreads];
    __shared__ double part_c[kThreads];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int32_t sentinel = H * W;                // validated < INT32_MAX on the host
    double acc_l = 0.0, acc_c = 0.0;
    if (i < m) {
        float p[3];
        for (int c = 0; c < 3; ++c) p[c] = points[i * 3 + c];
        // pass 1: density and beta
        float dsum = 0.f, bsum = 0.f;
        bool bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
        for (int k = 0; k < kK; ++k) {
            const int32_t j = knn[i * kK + k];
            if (j < 0 || j >= n) { bad = true; continue; }
            Neighbour nb;
            load_neighbour(j, p, means, scales, quats, opac, nb);
            dsum += nb.g * nb.sg;
            bsum += nb.es[nb.amin];
        }
        const float beta = bsum / (float)kK;
        const bool clamped = dsum > 1.f;
        const float d = clamped ? 1.f : dsum;     // 1 + 1e-12 is 1.0 in float32
        // camera space, projection, depth fetch (grid_sample: bilinear, border, align_corners=False)
        float pc[4], h[4];
        for (int r = 0; r < 4; ++r)
            pc[r] = ((mt.v[r * 4] * p[0] + mt.v[r * 4 + 1] * p[1]) + mt.v[r * 4 + 2] * p[2]) + mt.v[r * 4 + 3];
        for (int r = 0; r < 4; ++r)
            h[r] = ((mt.p[r * 4] * pc[0] + mt.p[r * 4 + 1] * pc[1]) + mt.p[r * 4 + 2] * pc[2]) + mt.p[r * 4 + 3] * pc[3];
        const float z = pc[2];
        float gx, gy;
        bool inside = z > znear;
        if (mode == TS_DENSITY_PROJ_SCREEN) {
            gx = h[0] / h[3];
            gy = h[1] / h[3];
            inside = inside && (-1.f <= gx) && (gx < 1.f) && (-1.f <= gy) && (gy < 1.f);
        } else {                                   // the reference: no perspective divide, grid not normalised
            gx = -(float)W * h[0];
            gy = -(float)H * h[1];
            inside = inside && (-(float)W < gx) && (gx <= 0.f) && (-(float)H < gy) && (gy <= 0.f);
        }
        const float off = mode == TS_DENSITY_PROJ_SCREEN ? TS_PIX_OFF : 0.f;
        float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f - off;
        float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f - off;
        bad = bad || !isfinite(ix) || !isfinite(iy);
        float mx = 1.f, my = 1.f;                  // clip_coordinates_set_grad: the borders count as outside
        if (ix <= 0.f) { ix = 0.f; mx = 0.f; } else if (ix >= (float)(W - 1)) { ix = (float)(W - 1); mx = 0.f; }
        if (iy <= 0.f) { iy = 0.f; my = 0.f; } else if (iy >= (float)(H - 1)) { iy = (float)(H - 1); my = 0.f; }
        if (bad) { ix = 0.f; iy = 0.f; inside = false; }
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;      // in [0, W-1] x [0, H-1] after the clip
        const int x1 = x0 + 1, y1 = y0 + 1;
        const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
        const bool in_x1 = x1 < W, in_y1 = y1 < H;
        const float v00 = depth[(int64_t)y0 * W + x0];
        const float v01 = in_x1 ? depth[(int64_t)y0 * W + x1] : 0.f;
        const float v10 = in_y1 ? depth[(int64_t)y1 * W + x0] : 0.f;
        const float v11 = (in_x1 && in_y1) ? depth[(int64_t)y1 * W + x1] : 0.f;
        const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
        const float zmap = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
        const float e = zmap - z;
        const float bb = beta * beta;
        const float approx = expf((-0.5f * (e * e)) / bb);
        const float diff = d - approx;
        if (inside) {
            acc_l = (double)fabsf(diff);
            acc_c = 1.0;
        }
        if (dens_out) {
            dens_out[i] = d;
            beta_out[i] = beta;
            approx_out[i] = bad ? __int_as_float(0x7fc00000) : approx;
            mask_out[i] = inside ? 1 : 0;
        }
        if (grows) {
            float* src = grows + ((int64_t)m * kK + i) * kRow;
            if (!inside) {
                for (int k = 0; k < kK; ++k)
                    for (int c = 0; c < kRow; ++c) grows[(i * kK + k) * kRow + c] = 0.f;
                for (int c = 0; c < kRow; ++c) src[c] = 0.f;
                for (int t = 0; t < 4; ++t) {
                    tap_key[i * 4 + t] = sentinel;
                    tap_val[i * 4 + t] = 0.f;
                }
            } else {
                const float gl = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                const float gd = clamped ? 0.f : gl;
                // approx = exp(u), u = (-0.5 e^2) / beta^2: autograd's chain
                const float gu = -gl * approx;
                const float gnum = gu / bb;
                const float gbb = -(gu * (-0.5f * (e * e))) / (bb * bb);
                const float gbeta = gbb * (2.f * beta);
                const float ge = (gnum * -0.5f) * (2.f * e);
                // depth taps and the grid's gradient
                const int32_t k00 = y0 * W + x0;
                tap_key[i * 4 + 0] = k00;
                tap_val[i * 4 + 0] = w00 * ge;
                tap_key[i * 4 + 1] = in_x1 ? k00 + 1 : sentinel;
                tap_val[i * 4 + 1] = in_x1 ? w01 * ge : 0.f;
                tap_key[i * 4 + 2] = in_y1 ? k00 + W : sentinel;
                tap_val[i * 4 + 2] = in_y1 ? w10 * ge : 0.f;
                tap_key[i * 4 + 3] = (in_x1 && in_y1) ? k00 + W + 1 : sentinel;
                tap_val[i * 4 + 3] = (in_x1 && in_y1) ? w11 * ge : 0.f;
                const float gix = ((-v00 * wy0 + v01 * wy0) - v10 * wy1 + v11 * wy1) * ge;
                const float giy = ((-v00 * wx0 - v01 * wx1) + v10 * wx0 + v11 * wx1) * ge;
                const float ggx = gix * (mx * ((float)W / 2.f));
                const float ggy = giy * (my * ((float)H / 2.f));
                float gh[4] = {0.f, 0.f, 0.f, 0.f};
                if (mode == TS_DENSITY_PROJ_SCREEN) {
                    gh[0] = ggx / h[3];
                    gh[1] = ggy / h[3];
                    gh[3] = -(ggx * h[0] + ggy * h[1]) / (h[3] * h[3]);
                } else {
                    gh[0] = ggx * -(float)W;
                    gh[1] = ggy * -(float)H;
                }
                float gpc[4];
                for (int c = 0; c < 4; ++c)
                    gpc[c] = ((gh[0] * mt.p[c] + gh[1] * mt.p[4 + c]) + gh[2] * mt.p[8 + c]) + gh[3] * mt.p[12 + c];
                gpc[2] += -ge;                     // e = z_map - z
                float gp[3];
                for (int b = 0; b < 3; ++b)
                    gp[b] = ((gpc[0] * mt.v[b] + gpc[1] * mt.v[4 + b]) + gpc[2] * mt.v[8 + b]) + gpc[3] * mt.v[12 + b];
                // pass 2: one gradient row per neighbour
                const float gbk = gbeta / (float)kK;
                for (int k = 0; k < kK; ++k) {
                    float* row = grows + (i * kK + k) * kRow;
                    const int32_t j = knn[i * kK + k];
                    Neighbour nb;
                    load_neighbour(j, p, means, scales, quats, opac, nb);
                    const float gg = gd * nb.sg;   // d = sum g_j sigmoid(o_j)
                    const float gsg = gd * nb.g;
                    const float go = gsg * (nb.sg * (1.f - nb.sg));
                    const float gq = (nb.qq >= 0.f && nb.qq <= 1e8f) ? (gg * nb.g) * -0.5f : 0.f;
                    float gy3[3], gs[3], gdl[3];
                    for (int a = 0; a < 3; ++a) {
                        gy3[a] = gq * (2.f * nb.y[a] * nb.w[a]);
                        gs[a] = ((gq * (nb.y[a] * nb.y[a])) * nb.w[a]) * -2.f;
                    }
                    gs[nb.amin] += gbk * nb.es[nb.amin];
                    float G[3][3];
                    for (int b = 0; b < 3; ++b) {
                        gdl[b] = (nb.R[b][0] * gy3[0] + nb.R[b][1] * gy3[1]) + nb.R[b][2] * gy3[2];
                        for (int a = 0; a < 3; ++a) G[b][a] = nb.dl[b] * gy3[a];
                        gp[b] += gdl[b];
                    }
                    float gq4[4];
                    quat_rot_vjp(nb.q, nb.qn, G, gq4);
                    for (int c = 0; c < 3; ++c) {
                        row[c] = -gdl[c];
                        row[3 + c] = gs[c];
                    }
                    for (int c = 0; c < 4; ++c) row[6 + c] = gq4[c];
                    row[10] = go;
                }
                // the point's gradient into its sampling source, through the values frozen at sampling time
                const float* f = frozen + i * kFrozen;
                float q0[4], qn0[4], R0[3][3], v[3];
                for (int c = 0; c < 4; ++c) q0[c] = f[6 + c];
                quat_rot(q0, qn0, R0);
                for (int c = 0; c < 3; ++c) v[c] = f[c] * f[3 + c];
                float G0[3][3];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) G0[a][b] = gp[a] * v[b];
                float gq0[4];
                quat_rot_vjp(q0, qn0, G0, gq0);
                for (int b = 0; b < 3; ++b) {
                    const float gv = (R0[0][b] * gp[0] + R0[1][b] * gp[1]) + R0[2][b] * gp[2];
                    src[b] = gp[b];
                    src[3 + b] = (gv * f[b]) * f[3 + b];
                }
                for (int c = 0; c < 4; ++c) src[6 + c] = gq0[c];
                src[10] = 0.f;
            }
        }
    }
    part_l[threadIdx.x] = acc_l;
    part_c[threadIdx.x] = acc_c;
    __syncthreads();
    tree_sum(part_l);
    tree_sum(part_c);
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 2] = part_l[0];
        partial[blockIdx.x * 2 + 1] = part_c[0];
    }
}

// one workgroup: out = {mean |d - approx| over the mask (NaN when empty), 1 / count (0 when empty), count}
__global__ __launch_bounds__(kThreads) void loss_reduce_kernel(int blocks, const double* __restrict__ partial,
                                                               float* __restrict__ out) {
    __shared__ double part_l[kThreads];
    __shared__ double part_c[kThreads];
    double l = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        l += partial[b * 2];
        c += partial[b * 2 + 1];
    }
    part_l[threadIdx.x] = l;
    part_c[threadIdx.x] = c;
    __syncthreads();
    tree_sum(part_l);
    tree_sum(part_c);
    if (threadIdx.x == 0) {
        const double cnt = part_c[0];
        out[0] = cnt > 0.0 ? (float)(part_l[0] / cnt) : __int_as_float(0x7fc00000);
        out[1] = cnt > 0.0 ? 1.0f / (float)cnt : 0.f;
        out[2] = (float)cnt;
    }
}

// ------------------------------------------------------------------ chunked segmented sums
constexpr int kOwn = 1;      // the chunk's last run starts here and continues into the next chunk
constexpr int kThrough = 2;  // the chunk is one run that came from the previous chunk and continues

template <int D>
__global__ __launch_bounds__(kThreads) void segment_local_kernel(int64_t T, int32_t num_keys,
                                                                 const int32_t* __restrict__ keys,
                                                                 const int64_t* __restrict__ perm,
                                                                 const float* __restrict__ vals,
                                                                 const float* __restrict__ scale, float* __restrict__ out,
                                                                 double* __restrict__ head, double* __restrict__ tail,
                                                                 int32_t* __restrict__ flags) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nchunks = (T + kChunk - 1) / kChunk;
    if (c >= nchunks) return;
    const int64_t i0 = c * kChunk, i1 = (i0 + kChunk < T) ? i0 + kChunk : T;
    const float sc = *scale;
    const int32_t key_before = c > 0 ? keys[i0 - 1] : -1;
    const int32_t key_after = i1 < T ? keys[i1] : -1;
    int fl = 0;
    double acc[D];
    int32_t cur = keys[i0];
    bool first = true;
    for (int d = 0; d < D; ++d) acc[d] = 0.0;
    for (int64_t i = i0; i <= i1; ++i) {
        const bool end = i == i1;
        const int32_t key = end ? -2 : keys[i];
        if (end || key != cur) {
            // the run of `cur` inside this chunk is complete
            const bool last = end;
            const bool cin = first && cur == key_before;
            const bool cout = last && cur == key_after;
            if (cur >= 0 && cur < num_keys) {
                if (!cin && !cout) {
                    for (int d = 0; d < D; ++d) out[(int64_t)cur * D + d] = (float)(acc[d] * (double)sc);
                } else if (cin) {
                    for (int d = 0; d < D; ++d) head[c * D + d] = acc[d];
                    if (cout) fl |= kThrough;
                } else {
                    for (int d = 0; d < D; ++d) tail[c * D + d] = acc[d];
                    fl |= kOwn;
                }
            }
            if (end) break;
            cur = key;
            first = false;
            for (int d = 0; d < D; ++d) acc[d] = 0.0;
        }
        const int64_t r = perm[i];
        for (int d = 0; d < D; ++d) acc[d] += (double)vals[r * D + d];
    }
    flags[c] = fl;
}

template <int D>
__global__ __launch_bounds__(kThreads) void segment_join_kernel(int64_t T, const int32_t* __restrict__ keys,
                                                                const float* __restrict__ scale, float* __restrict__ out,
                                                                const double* __restrict__ head,
                                                                const double* __restrict__ tail,
                                                                const int32_t* __restrict__ flags) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nchunks = (T + kChunk - 1) / kChunk;
    if (c >= nchunks || !(flags[c] & kOwn)) return;
    const int64_t i1 = (c + 1) * kChunk;           // < T: the run continues into chunk c + 1
    const int32_t key = keys[i1 - 1];
    double acc[D];
    for (int d = 0; d < D; ++d) acc[d] = tail[c * D + d];
    for (int64_t c2 = c + 1; c2 < nchunks; ++c2) {
        for (int d = 0; d < D; ++d) acc[d] += head[c2 * D + d];
        if (!(flags[c2] & kThrough)) break;
    }
    const float sc = *scale;
    for (int d = 0; d < D; ++d) out[(int64_t)key * D + d] = (float)(acc[d] * (double)sc);
}

inline int loss_blocks(int32_t m) { return (int)nblocks(m < 1 ? 1 : m, kThreads); }

}  // namespace

extern "C" {

int64_t ts_density_sample_ws_bytes(int32_t n) {
    if (n < 1) return TS_E_BADARG;
    return 2 * align256((int64_t)n * 8) + align256(scan_blocks(n) * 8);
}

int ts_density_sample(int32_t n, int32_t m, int32_t weights, const float* means, const float* scales, const float* quats,
                      const float* uniforms, const int32_t* rows_in, const float* normals, int32_t* rows, float* points,
                      float* frozen, void* ws, void* stream) {
    if (n < 1 || m < 0 || !means || !scales || !quats || !ws) return TS_E_BADARG;
    if (weights != TS_DENSITY_WEIGHTS_REFERENCE && weights != TS_DENSITY_WEIGHTS_AREA) return TS_E_BADARG;
    if (m > 0 && (!normals || !rows || !points || !frozen || (!uniforms && !rows_in))) return TS_E_BADARG;
    if (m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    double* a = (double*)ws;
    double* c = (double*)((char*)ws + align256((int64_t)n * 8));
    double* totals = (double*)((char*)ws + 2 * align256((int64_t)n * 8));
    const double* cdf = nullptr;
    if (!rows_in) {
        hipLaunchKernelGGL(weights_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, s, (int)n, scales,
                           a);
        scan(n, a, c, totals, s);                  // C_i = a_0 + ... + a_i
        if (weights == TS_DENSITY_WEIGHTS_REFERENCE) {
            scan(n, c, a, totals, s);              // the reference draws row i with weight C_i
            cdf = a;
        } else {
            cdf = c;
        }
    }
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)nblocks(m, kThreads)), dim3(kThreads), 0, s, (int)n, (int)m, cdf,
                       uniforms, rows_in, normals, means, scales, quats, rows, points, frozen);
    return launch_status();
}

int64_t ts_density_loss_ws_bytes(int32_t m) {
    if (m < 1) return TS_E_BADARG;
    return (int64_t)loss_blocks(m) * 2 * (int64_t)sizeof(double);
}

int ts_density_loss(int32_t n, int32_t m, const float* points, const int32_t* rows, const float* frozen,
                    const int32_t* knn, const float* means, const float* scales, const float* quats,
                    const float* opacities, int32_t height, int32_t width, const float* depth,
                    const float* view_proj_host, int32_t projection, float znear, float* out, float* density,
                    float* beta, float* approx, uint8_t* mask, float* grad_rows, int32_t* tap_keys, float* tap_vals,
                    void* ws, void* stream) {
    if (n < kK || m < 1 || height < 1 || width < 1 || (int64_t)height * width >= INT32_MAX) return TS_E_BADARG;
    if (!points || !rows || !frozen || !knn || !means || !scales || !quats || !opacities || !depth || !view_proj_host ||
        !out || !ws)
        return TS_E_BADARG;
    if (projection != TS_DENSITY_PROJ_REFERENCE && projection != TS_DENSITY_PROJ_SCREEN) return TS_E_BADARG;
    if ((density || beta || approx || mask) && !(density && beta && approx && mask)) return TS_E_BADARG;
    if ((grad_rows || tap_keys || tap_vals) && !(grad_rows && tap_keys && tap_vals)) return TS_E_BADARG;
    Mats mt;
    for (int c = 0; c < 16; ++c) {
        mt.v[c] = view_proj_host[c];
        mt.p[c] = view_proj_host[16 + c];
    }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = loss_blocks(m);
    double* partial = (double*)ws;
    hipLaunchKernelGGL(pairs_kernel, dim3(blocks), dim3(kThreads), 0, s, (int)n, (int)m, (int)height, (int)width,
                       (int)projection, znear, mt, points, rows, frozen, knn, means, scales, quats, opacities, depth,
                       density, beta, approx, mask, grad_rows, tap_keys, tap_vals, partial);
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(kThreads), 0, s, blocks, (const double*)partial, out);
    return launch_status();
}

int64_t ts_segment_sum_ws_bytes(int64_t entries, int32_t width) {
    if (entries < 1 || (width != 1 && width != kRow)) return TS_E_BADARG;
    const int64_t nchunks = (entries + kChunk - 1) / kChunk;
    return 2 * align256(nchunks * width * 8) + align256(nchunks * 4);
}

int ts_segment_sum(int64_t entries, int32_t width, int32_t num_keys, const int32_t* keys_sorted, const int64_t* perm,
                   const float* vals, const float* scale, float* out, void* ws, void* stream) {
    if (entries < 1 || num_keys < 1 || (width != 1 && width != kRow)) return TS_E_BADARG;
    if (!keys_sorted || !perm || !vals || !scale || !out || !ws) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nchunks = (entries + kChunk - 1) / kChunk;
    double* head = (double*)ws;
    double* tail = (double*)((char*)ws + align256(nchunks * width * 8));
    int32_t* flags = (int32_t*)((char*)ws + 2 * align256(nchunks * width * 8));
    hipError_t e = hipMemsetAsync(out, 0, (size_t)num_keys * (size_t)width * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)nblocks(nchunks, kThreads));
    if (width == 1) {
        hipLaunchKernelGGL(segment_local_kernel<1>, grid, dim3(kThreads), 0, s, entries, num_keys, keys_sorted, perm, vals,
                           scale, out, head, tail, flags);
        hipLaunchKernelGGL(segment_join_kernel<1>, grid, dim3(kThreads), 0, s, entries, keys_sorted, scale, out,
                           (const double*)head, (const double*)tail, (const int32_t*)flags);
    } else {
        hipLaunchKernelGGL(segment_local_kernel<kRow>, grid, dim3(kThreads), 0, s, entries, num_keys, keys_sorted, perm,
                           vals, scale, out, head, tail, flags);
        hipLaunchKernelGGL(segment_join_kernel<kRow>, grid, dim3(kThreads), 0, s, entries, keys_sorted, scale, out,
                           (const double*)head, (const double*)tail, (const int32_t*)flags);
    }
    return launch_status();
}

}  // extern "C"
