// pose.hip - the gradient of a loss with respect to a camera's pose from the gradient rows of the Gaussians' means and
// quaternions (the arithmetic and the order of the sum: pose_math.h).
//
// ts_pose_grad is a streaming reduction: 56 bytes read per Gaussian, 48 bytes written per workgroup.  A wave owns
// TS_POSE_WAVE_ROWS = 256 consecutive rows.  Their means and mean gradients are two contiguous blocks of 768 floats, which
// the wave reads as a flat stream (16 bytes a lane where the block starts on 16 bytes) into its own LDS rows; a lane then
// picks the three floats of its rows at a stride of three words, which no two lanes of a wave share a bank at.  The
// quaternions and their gradients are 16-byte rows and are loaded by the lane that uses them, before the wave waits for
// its blocks, so that all fourteen 16-byte loads of a lane are in flight together.  Lanes add their four rows in double, a
// fixed butterfly adds the lanes, the four waves' sums are added left to right into the workgroup's six doubles in the
// workspace, and a second launch of one workgroup adds the records in index order.  No atomics and no device query: the
// partition of the rows depends on n alone, so the 48 bytes are the same on every run, on every stream and for every
// size of the workspace.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "pose_math.h"

namespace {

constexpr int kWave = TS_POSE_LANES;
constexpr int kWaves = TS_POSE_BLOCK_WAVES;        // waves per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kLaneRows = TS_POSE_LANE_ROWS;
constexpr int kWaveRows = TS_POSE_WAVE_ROWS;
constexpr int kReduceThreads = TS_POSE_REDUCE_THREADS;

// TS_POSE_LDS_BUTTERFLY=1: the lanes are added through LDS instead of by shuffles - the same tree, the same bits.  Measured
// (tools/time_pose.py; 1 M rows): 20.8 - 21.7 us for the two launches against 18.3 - 18.7 us with
// the shuffles, which stay.
#ifndef TS_POSE_LDS_BUTTERFLY
#define TS_POSE_LDS_BUTTERFLY 0
#endif

#define TS_POSE_WAVE_SYNC()                                       \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

// lane 0 <- the sum over the wave's lanes by the tree s_l <- s_l + s_(l + d), d = 32, 16, .., 1 (what the butterfly
// s_l <- s_l + s_(l ^ d) leaves in lane 0)
__device__ __forceinline__ double wave_sum(double v, double* tree, int lane) {
#if TS_POSE_LDS_BUTTERFLY
    tree[lane] = v;
    TS_POSE_WAVE_SYNC();
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        if (lane < d) tree[lane] += tree[lane + d];
        TS_POSE_WAVE_SYNC();
    }
    v = tree[0];
    TS_POSE_WAVE_SYNC();
    return v;
#else
    (void)tree;
    (void)lane;
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
#endif
}

// the wave's block of `total` (<= 3 kWaveRows) floats from global memory into its LDS copy; lanes take consecutive
// addresses, 16 bytes each where `vec` (the block starts on 16 bytes), the tail and the rest 4 bytes each
__device__ __forceinline__ void load_block(const float* __restrict__ glob, float* rows, int total, int lane, bool vec) {
    int done = 0;
    if (vec) {
        const int quads = total >> 2;
#pragma unroll
        for (int k = 0; k < 3 * kWaveRows / 4 / kWave; ++k) {
            const int v = lane + k * kWave;
            if (v < quads) reinterpret_cast<float4*>(rows)[v] = reinterpret_cast<const float4*>(glob)[v];
        }
        done = 4 * quads;
    }
    for (int e = done + lane; e < total; e += kWave) rows[e] = glob[e];
}

__device__ __forceinline__ void load_row4(const float* __restrict__ base, long long row, bool vec, float* out) {
    if (vec) {
        const float4 v = reinterpret_cast<const float4*>(base)[row];
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
        for (int k = 0; k < 4; ++k) out[k] = base[4 * row + k];
    }
}

// records[6 b .. 6 b + 5] <- the six sums over the rows of workgroup b
__global__ __launch_bounds__(kThreads) void pose_grad_rows_kernel(int n, const ts_pose_view view,
                                                                  const float* __restrict__ means,
                                                                  const float* __restrict__ quats,
                                                                  const float* __restrict__ v_means,
                                                                  const float* __restrict__ v_quats, int vec_bits,
                                                                  double* __restrict__ records) {
    __shared__ __attribute__((aligned(16))) float lds[kWaves][2][3 * kWaveRows];
    __shared__ double sums[kWaves][TS_POSE_TERMS];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const long long first = ((long long)blockIdx.x * kWaves + wave) * kWaveRows;    // the wave's first row
    const int count = first >= n ? 0 : (n - first < kWaveRows ? (int)(n - first) : kWaveRows);
    float* const lm = lds[wave][0];
    float* const lg = lds[wave][1];
    float q[kLaneRows][4], h[kLaneRows][4];
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
        const int r = lane + j * kWave;
        if (r < count) {
            load_row4(quats, first + r, (vec_bits & 4) != 0, q[j]);
            load_row4(v_quats, first + r, (vec_bits & 8) != 0, h[j]);
        }
    }
    // a wave's block starts 3072 bytes after the one before it: on 16 bytes where the tensor does
    load_block(means + 3 * first, lm, 3 * count, lane, (vec_bits & 1) != 0);
    load_block(v_means + 3 * first, lg, 3 * count, lane, (vec_bits & 2) != 0);
    __syncthreads();
    double acc[TS_POSE_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
        const int r = lane + j * kWave;
        if (r < count) ts_pose_row_add(view, lm + 3 * r, q[j], lg + 3 * r, h[j], acc);
    }
#if TS_POSE_LDS_BUTTERFLY
    __shared__ double trees[kWaves][kWave];
    double* const tree = trees[wave];
#else
    double* const tree = nullptr;
#endif
#pragma unroll
    for (int k = 0; k < TS_POSE_TERMS; ++k) acc[k] = wave_sum(acc[k], tree, lane);
    if (lane == 0)
        for (int k = 0; k < TS_POSE_TERMS; ++k) sums[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < TS_POSE_TERMS) {                 // the waves' sums left to right; a wave past the last row holds +0.0
        double v = sums[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) v += sums[w][threadIdx.x];
        records[TS_POSE_TERMS * (long long)blockIdx.x + threadIdx.x] = v;
    }
}

// out[6] <- the sum of the workgroups' records: thread i adds the records i, i + 1024, ... in that order, then a binary tree
// over the 1024 threads - the same additions in the same order on every run; no records: six zeros
__global__ __launch_bounds__(kReduceThreads) void pose_grad_reduce_kernel(long long waves,
                                                                          const double* __restrict__ records,
                                                                          double* __restrict__ out) {
    __shared__ double part[TS_POSE_TERMS][kReduceThreads];
    double acc[TS_POSE_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < waves; i += kReduceThreads)
        for (int k = 0; k < TS_POSE_TERMS; ++k) acc[k] += records[TS_POSE_TERMS * i + k];
    for (int k = 0; k < TS_POSE_TERMS; ++k) part[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int step = kReduceThreads / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int k = 0; k < TS_POSE_TERMS; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x < TS_POSE_TERMS) out[threadIdx.x] = part[threadIdx.x][0];
}

}  // namespace

extern "C" {

int64_t ts_pose_ws_bytes(int32_t n) {
    return n <= 0 ? 0 : ts_pose_records(n) * TS_POSE_TERMS * (int64_t)sizeof(double);
}

int ts_pose_grad(int32_t n, const float* view34_host, const float* means, const float* quats, const float* v_means,
                 const float* v_quats, void* ws, double* out6, void* stream) {
    if (n < 0 || !view34_host || !out6 || (uintptr_t)out6 % sizeof(double)) return TS_E_BADARG;
    if (n > 0 && (!means || !quats || !v_means || !v_quats || !ws || (uintptr_t)ws % sizeof(double))) return TS_E_BADARG;
    const float* const rows[4] = {means, v_means, quats, v_quats};
    int vec_bits = 0;
    for (int k = 0; k < 4; ++k) {
        if (n > 0 && (uintptr_t)rows[k] % sizeof(float)) return TS_E_BADARG;
        if ((uintptr_t)rows[k] % 16 == 0) vec_bits |= 1 << k;
    }
    ts_pose_view view;
    for (int i = 0; i < 12; ++i) view.m[i] = view34_host[i];
    const hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = ts_pose_records(n);
    if (blocks > 0)
        hipLaunchKernelGGL(pose_grad_rows_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, (int)n, view, means, quats,
                           v_means, v_quats, vec_bits, (double*)ws);
    hipLaunchKernelGGL(pose_grad_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, s, (long long)blocks,
                       (const double*)ws, out6);
    return launch_status();
}

}  // extern "C"
