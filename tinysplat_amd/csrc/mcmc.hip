// mcmc.hip - budgeted densification (3DGS-MCMC: Kheradmand et al., NeurIPS 2024), DESIGN.md section 6r.  The per-row
// arithmetic is mcmc_math.h's; the prefix sum is prefix_scan.h's, the one density.hip draws its sample rows with.
//
//   every step      noise       means += scale * g(1 - o) * (Sigma z), z given or drawn in the kernel (Philox4x32-10)
//   every step      mean        mean(sigmoid(opacities)) / mean(exp(scales)): value and gradient, double sums in a fixed
//                               order (one partial per workgroup by a fixed tree, then one workgroup)
//   a refinement    weights     w = o as double (0 for a dead row on request) and the dead flags, in the encoding that
//                               lets ts_densify_plan list the dead rows in ascending order
//                   sample      the prefix, then one thread per draw: the row (bisection) and an integer atomic count
//                   rewrite     one thread per picked row: its own opacity and scales from their OLD values, its
//                               Adam moments zeroed
//                   copy        each destination row receives its (rewritten) source's row of every tensor, moments 0
// No float atomics, no allocation, no synchronisation.  Built with -ffp-contract=off (see _build.py).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "mcmc_math.h"
#include "prefix_scan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

struct RowTables {
    float* param[TS_GATHER_MAX_TENSORS];
    float* exp_avg[TS_GATHER_MAX_TENSORS];
    float* exp_avg_sq[TS_GATHER_MAX_TENSORS];
    int width[TS_GATHER_MAX_TENSORS];        // floats per row
    int num;
};

__device__ __forceinline__ void tree_sum(double* part) {
    for (int step = kThreads / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ noise
// A workgroup owns 256 consecutive rows.  The three-float rows (means, scales, a caller's z) are read as the 768
// consecutive dwords they are - every wave instruction covers 256 contiguous bytes - and handed to their rows through
// LDS (row r reads words 3r..3r+2: stride 3, no bank conflict); quaternions are one 16-byte load per row and opacities
// one dword.  The means go back the same way.  Nothing is read or written at or beyond element 3n.
__global__ __launch_bounds__(kThreads) void noise_kernel(int n, float scale, float* __restrict__ means,
                                                         const float* __restrict__ scales,
                                                         const float4* __restrict__ quats,
                                                         const float* __restrict__ opac, const float* __restrict__ z,
                                                         uint32_t seed_lo, uint32_t seed_hi, uint32_t step) {
    __shared__ float sm[3 * kThreads];
    __shared__ float ss[3 * kThreads];
    __shared__ float sz[3 * kThreads];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kThreads;
    const int64_t e0 = row0 * 3, total = (int64_t)n * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t e = e0 + k * kThreads + t;
        if (e < total) {
            sm[k * kThreads + t] = means[e];
            ss[k * kThreads + t] = scales[e];
            if (z) sz[k * kThreads + t] = z[e];
        }
    }
    __syncthreads();
    const int64_t i = row0 + t;
    if (i < n) {
        const float o = 1.0f / (1.0f + expf(-opac[i]));
        const float g = ts_mcmc_gate(o);
        if (g > 0.0f) {                              // g == 0 (and a NaN opacity): the row keeps its bits
            const float4 q4 = quats[i];
            const float q[4] = {q4.x, q4.y, q4.z, q4.w};
            const float s[3] = {ss[3 * t], ss[3 * t + 1], ss[3 * t + 2]};
            float zz[3], d[3];
            if (z) {
                zz[0] = sz[3 * t]; zz[1] = sz[3 * t + 1]; zz[2] = sz[3 * t + 2];
            } else {
                ts_mcmc_normals3(seed_lo, seed_hi, (uint32_t)i, step, zz);
            }
            ts_mcmc_sigma_z(q, s, zz, d);
            const float f = scale * g;
#pragma unroll
            for (int c = 0; c < 3; ++c) sm[3 * t + c] = sm[3 * t + c] + f * d[c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t e = e0 + k * kThreads + t;
        if (e < total) means[e] = sm[k * kThreads + t];
    }
}

__global__ __launch_bounds__(kThreads) void normals_kernel(int n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                           float* __restrict__ out) {
    __shared__ float sz[3 * kThreads];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kThreads;
    const int64_t i = row0 + t;
    if (i < n) ts_mcmc_normals3(seed_lo, seed_hi, (uint32_t)i, step, sz + 3 * t);
    __syncthreads();
    const int64_t e0 = row0 * 3, total = (int64_t)n * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t e = e0 + k * kThreads + t;
        if (e < total) out[e] = sz[k * kThreads + t];
    }
}

// ------------------------------------------------------------------ the regularisers
inline int mean_blocks(int64_t n) {
    const int64_t b = (n + kThreads * 4 - 1) / (kThreads * 4);
    return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : (int)b);
}

// kind TS_MCMC_MEAN_SIGMOID: f = sigmoid(x), f' = f (1 - f);  TS_MCMC_MEAN_EXP: f = f' = exp(x).  float32 per element,
// grad = scale * f' with scale = 1 / n
__global__ __launch_bounds__(kThreads) void mean_kernel(int64_t n, int kind, float scale, const float* __restrict__ x,
                                                        float* __restrict__ grad, double* __restrict__ partial) {
    __shared__ double part[kThreads];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        float f, df;
        if (kind == TS_MCMC_MEAN_SIGMOID) {
            f = 1.0f / (1.0f + expf(-x[i]));
            df = f * (1.0f - f);
        } else {
            f = expf(x[i]);
            df = f;
        }
        acc += (double)f;
        if (grad) grad[i] = scale * df;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    tree_sum(part);
    if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kThreads) void mean_reduce_kernel(int blocks, int64_t n, const double* __restrict__ partial,
                                                               float* __restrict__ out) {
    __shared__ double part[kThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) acc += partial[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    tree_sum(part);
    if (threadIdx.x == 0) out[0] = (float)(part[0] / (double)n);
}

// ------------------------------------------------------------------ refinement
// flags: a DEAD row is 0 and a live row TS_DENSIFY_PRUNE, so that the "kept" list of ts_densify_plan is the list of
// dead rows in ascending order and its first count their number
__global__ __launch_bounds__(kThreads) void weights_kernel(int n, const float* __restrict__ opac, float min_opacity,
                                                           int zero_dead, double* __restrict__ w,
                                                           uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float o = ts_mcmc_sigmoid(opac[i]);
    const bool dead = !(o > min_opacity);            // a NaN opacity is dead
    const bool none = (dead && zero_dead) || !(o > 0.0f);
    w[i] = none ? 0.0 : (double)o;
    if (flags) flags[i] = dead ? (uint8_t)0 : (uint8_t)TS_DENSIFY_PRUNE;
}

__global__ __launch_bounds__(kThreads) void draw_kernel(int n, int m, const double* __restrict__ prefix,
                                                        const double* __restrict__ w,
                                                        const float* __restrict__ uniforms, int32_t* __restrict__ picks,
                                                        int32_t* __restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const double target = (double)uniforms[j] * prefix[n - 1];
    const int32_t r = ts_mcmc_pick(n, prefix, w, target);
    picks[j] = r;
    if (r >= 0) atomicAdd(counts + r, 1);
}

__global__ __launch_bounds__(kThreads) void rewrite_kernel(int n, const int32_t* __restrict__ counts, float min_opacity,
                                                           float* __restrict__ opac, float* __restrict__ scales,
                                                           RowTables tb) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t c = counts[i];
    if (c <= 0) return;
    float logit, lc;
    ts_mcmc_relocate(ts_mcmc_sigmoid(opac[i]), c, min_opacity, &logit, &lc);
    opac[i] = logit;
    for (int a = 0; a < 3; ++a) scales[i * 3 + a] = scales[i * 3 + a] + lc;
    for (int k = 0; k < tb.num; ++k) {
        const int64_t b = i * tb.width[k];
        for (int e = 0; e < tb.width[k]; ++e) {
            tb.exp_avg[k][b + e] = 0.0f;
            tb.exp_avg_sq[k][b + e] = 0.0f;
        }
    }
}

// tensor blockIdx.y: param[dst[j], :] = param[src[j], :], both moments of row dst[j] = 0; a pair with a row outside
// [0, n) (a draw that found no row) is skipped
__global__ __launch_bounds__(kThreads) void copy_rows_kernel(RowTables tb, int n, int m, const int32_t* __restrict__ dst,
                                                             const int32_t* __restrict__ src) {
    const int k = blockIdx.y;
    const int w = tb.width[k];
    const int64_t total = (int64_t)m * w;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
        const int64_t j = e / w;
        const int c = (int)(e - j * w);
        const int32_t d = dst[j], s = src[j];
        if (d < 0 || d >= n || s < 0 || s >= n) continue;
        tb.param[k][(int64_t)d * w + c] = tb.param[k][(int64_t)s * w + c];
        if (tb.exp_avg[k]) tb.exp_avg[k][(int64_t)d * w + c] = 0.0f;
        if (tb.exp_avg_sq[k]) tb.exp_avg_sq[k][(int64_t)d * w + c] = 0.0f;
    }
}

// host tables -> the by-value kernel argument; false for a bad table
bool fill_tables(RowTables& tb, int32_t num, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                 const int32_t* widths, bool need_params, bool need_moments) {
    if (num < 0 || num > TS_GATHER_MAX_TENSORS) return false;
    if (num > 0 && (!widths || (need_params && !params) || (need_moments && (!exp_avg || !exp_avg_sq)))) return false;
    tb.num = 0;
    for (int k = 0; k < TS_GATHER_MAX_TENSORS; ++k) {
        tb.param[k] = nullptr; tb.exp_avg[k] = nullptr; tb.exp_avg_sq[k] = nullptr; tb.width[k] = 0;
    }
    for (int k = 0; k < num; ++k) {
        if (widths[k] < 0) return false;
        if (widths[k] == 0) continue;                                       // (colors_rest of an SH-0 model)
        const int at = tb.num++;
        tb.width[at] = widths[k];
        tb.param[at] = params ? params[k] : nullptr;
        tb.exp_avg[at] = exp_avg ? exp_avg[k] : nullptr;
        tb.exp_avg_sq[at] = exp_avg_sq ? exp_avg_sq[k] : nullptr;
        if (need_params && !tb.param[at]) return false;
        if (need_moments && (!tb.exp_avg[at] || !tb.exp_avg_sq[at])) return false;
        if ((tb.exp_avg[at] == nullptr) != (tb.exp_avg_sq[at] == nullptr)) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int ts_mcmc_noise(int32_t n, float* means, const float* scales, const float* quats, const float* opacities, float scale,
                  const float* z, uint64_t seed, uint32_t step, void* stream) {
    if (n < 1 || !means || !scales || !quats || !opacities || ((uintptr_t)quats & 15) != 0) return TS_E_BADARG;
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n,
                       scale, means, scales, (const float4*)quats, opacities, z, (uint32_t)seed, (uint32_t)(seed >> 32),
                       step);
    return launch_status();
}

int ts_mcmc_normals(int32_t n, uint64_t seed, uint32_t step, float* out, void* stream) {
    if (n < 1 || !out) return TS_E_BADARG;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n,
                       (uint32_t)seed, (uint32_t)(seed >> 32), step, out);
    return launch_status();
}

int64_t ts_mcmc_mean_ws_bytes(int64_t count) {
    if (count < 1) return TS_E_BADARG;
    return (int64_t)mean_blocks(count) * (int64_t)sizeof(double);
}

int ts_mcmc_mean(int32_t kind, int64_t count, const float* x, float* value, float* grad, void* ws, void* stream) {
    if (count < 1 || !x || !value || !ws) return TS_E_BADARG;
    if (kind != TS_MCMC_MEAN_SIGMOID && kind != TS_MCMC_MEAN_EXP) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = mean_blocks(count);
    double* partial = (double*)ws;
    hipLaunchKernelGGL(mean_kernel, dim3(blocks), dim3(kThreads), 0, s, count, (int)kind, (float)(1.0 / (double)count), x,
                       grad, partial);
    hipLaunchKernelGGL(mean_reduce_kernel, dim3(1), dim3(kThreads), 0, s, blocks, count, (const double*)partial, value);
    return launch_status();
}

int ts_mcmc_weights(int32_t n, const float* opacities, float min_opacity, int32_t zero_dead, double* weights,
                    uint8_t* flags, void* stream) {
    if (n < 1 || !opacities || !weights || !(min_opacity >= 0.0f)) return TS_E_BADARG;
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n,
                       opacities, min_opacity, (int)(zero_dead != 0), weights, flags);
    return launch_status();
}

int64_t ts_mcmc_sample_ws_bytes(int32_t n) {
    if (n < 1) return TS_E_BADARG;
    return align256((int64_t)n * 8) + align256(scan_blocks(n) * 8);
}

int ts_mcmc_sample_rows(int32_t n, int32_t m, const double* weights, const float* uniforms, int32_t* picks,
                        int32_t* counts, void* ws, void* stream) {
    if (n < 1 || m < 1 || !weights || !uniforms || !picks || !counts || !ws) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    double* prefix = (double*)ws;
    double* totals = (double*)((char*)ws + align256((int64_t)n * 8));
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    scan(n, weights, prefix, totals, s);
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)nblocks(m, kThreads)), dim3(kThreads), 0, s, (int)n, (int)m,
                       (const double*)prefix, weights, uniforms, picks, counts);
    return launch_status();
}

int ts_mcmc_rewrite(int32_t n, const int32_t* counts, float min_opacity, float* opacities, float* scales,
                    int32_t num_tensors, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                    const int32_t* row_floats_host, void* stream) {
    if (n < 1 || !counts || !opacities || !scales || !(min_opacity >= 0.0f)) return TS_E_BADARG;
    RowTables tb;
    if (!fill_tables(tb, num_tensors, nullptr, exp_avg_host, exp_avg_sq_host, row_floats_host, false, true))
        return TS_E_BADARG;
    hipLaunchKernelGGL(rewrite_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n,
                       counts, min_opacity, opacities, scales, tb);
    return launch_status();
}

int ts_mcmc_copy_rows(int32_t n, int32_t m, const int32_t* dst_rows, const int32_t* src_rows, int32_t num_tensors,
                      float* const* params_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                      const int32_t* row_floats_host, void* stream) {
    if (n < 1 || m < 1 || !dst_rows || !src_rows || num_tensors < 1) return TS_E_BADARG;
    RowTables tb;
    if (!fill_tables(tb, num_tensors, params_host, exp_avg_host, exp_avg_sq_host, row_floats_host, true, false))
        return TS_E_BADARG;
    if (tb.num == 0) return 0;
    int most = 0;
    for (int k = 0; k < tb.num; ++k) most = tb.width[k] > most ? tb.width[k] : most;
    int64_t blocks = nblocks((int64_t)m * most, kThreads);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)blocks, (unsigned)tb.num), dim3(kThreads), 0, (hipStream_t)stream,
                       tb, (int)n, (int)m, dst_rows, src_rows);
    return launch_status();
}

}  // extern "C"
