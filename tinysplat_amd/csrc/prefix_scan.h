// prefix_scan.h - the inclusive prefix sum of n doubles in a FIXED order, shared by density.hip (sample_points) and
// mcmc.hip (sample_rows): the same input gives the same bits on every run and in both files.
//
//   local    each workgroup scans kScanThreads * kScanItems = 2048 consecutive items: per-thread serial sums of
//            kScanItems items, then a Hillis-Steele tree over the 256 thread totals; it writes its total
//   totals   one workgroup turns the workgroup totals into exclusive offsets (serial runs per thread + the same tree)
//   add      every item gets its workgroup's offset
// A prefix is therefore not the running sum P[i-1] + w[i]: neighbours across a thread or workgroup border are
// associated differently and may differ from it in the last bit (tests/mcmc_oracle.py restates the order).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_util.h"

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;                       // per thread: one scan workgroup covers 2048 items

// inclusive scan, pass 1: each workgroup scans kScanThreads * kScanItems consecutive items (per-thread serial sums,
// then a fixed Hillis-Steele tree over the thread totals) and writes its total
__global__ __launch_bounds__(kScanThreads) void scan_local_kernel(int64_t n, const double* __restrict__ in,
                                                                  double* __restrict__ out,
                                                                  double* __restrict__ totals) {
    __shared__ double sh[kScanThreads];
    const int64_t base = (int64_t)blockIdx.x * (kScanThreads * kScanItems) + (int64_t)threadIdx.x * kScanItems;
    double loc[kScanItems];
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) {
        acc += (base + t < n) ? in[base + t] : 0.0;
        loc[t] = acc;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const double v = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0.0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    const double before = threadIdx.x > 0 ? sh[threadIdx.x - 1] : 0.0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t)
        if (base + t < n) out[base + t] = before + loc[t];
    if (threadIdx.x == kScanThreads - 1) totals[blockIdx.x] = sh[kScanThreads - 1];
}

// pass 2: one workgroup turns the workgroup totals into exclusive offsets (serial runs per thread + the same tree)
__global__ __launch_bounds__(kScanThreads) void scan_totals_kernel(int64_t nb, double* __restrict__ totals) {
    __shared__ double sh[kScanThreads];
    const int64_t per = (nb + kScanThreads - 1) / kScanThreads;
    const int64_t b0 = (int64_t)threadIdx.x * per;
    double acc = 0.0;
    for (int64_t b = b0; b < b0 + per && b < nb; ++b) acc += totals[b];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const double v = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0.0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    double run = threadIdx.x > 0 ? sh[threadIdx.x - 1] : 0.0;
    for (int64_t b = b0; b < b0 + per && b < nb; ++b) {
        const double t = totals[b];
        totals[b] = run;
        run += t;
    }
}

__global__ __launch_bounds__(kScanThreads) void scan_add_kernel(int64_t n, const double* __restrict__ offsets,
                                                                double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    if (i >= n) return;
    out[i] += offsets[i / (kScanThreads * kScanItems)];
}

inline int64_t scan_blocks(int64_t n) { return (n + kScanThreads * kScanItems - 1) / (kScanThreads * kScanItems); }

// out[i] = in[0] + ... + in[i]; totals: scan_blocks(n) doubles of scratch
inline void scan(int64_t n, const double* in, double* out, double* totals, hipStream_t s) {
    const int64_t nb = scan_blocks(n);
    hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, n, in, out, totals);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kScanThreads), 0, s, nb, totals);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nblocks(n, kScanThreads)), dim3(kScanThreads), 0, s, n,
                       (const double*)totals, out);
}

}  // namespace
