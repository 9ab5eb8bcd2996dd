// surface.hip - the opacity-entropy regulariser of the training loop (scripts/train.py:71-75):
//
//   o = sigmoid(x),  L_o = -mean(o log(o + 1e-10) + (1 - o) log(1 - o + 1e-10))   over all N opacity logits x
//
// ts_opacity_entropy writes dL_o/dx for every Gaussian and the value L_o, in two launches on one stream:
//   entropy   grid-stride over the logits: the gradient (the derivative of exactly the expression above,
//             the +1e-10 terms included) and one double partial sum of the entropy terms per workgroup,
//             summed inside the workgroup by a fixed tree
//   reduce    one workgroup sums the <= kMaxBlocks partials by a fixed tree, in double
// No atomics: the value and the gradient are one fixed function of the input (bit-identical from run to
// run).  The partials could be handed to a last-arriving workgroup in the same launch, but that needs a
// zeroed ticket per call (one memset node) and the agent-scope hand-off; the second launch is simpler at
// the same count of stream operations.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr float kEps = 1e-10f;

inline int entropy_blocks(int32_t n) {
    const int64_t b = ((int64_t)n + kThreads * 4 - 1) / (kThreads * 4);      // int64: no overflow near INT32_MAX
    return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : (int)b);
}

// fixed-shape tree over one double per thread; the sum lands in part[0]
__device__ __forceinline__ void tree_sum(double* part) {
    for (int step = kThreads / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
}

// Every product and sum is its own float32 operation (no fma contraction): sigmoid, the two products of the
// expression, then d/do of o log(o + eps) and (1 - o) log(1 - o + eps), times -1/N (the mean), times
// sigmoid' = (1 - o) o.  Autograd applies the same factors in another order (-1/N first, then log's and mul's
// backward), so the gradient agrees with it to a few float32 roundings, not bit for bit.
__global__ __launch_bounds__(kThreads) void entropy_kernel(int n, float scale, const float* __restrict__ x,
                                                           float* __restrict__ v_x, double* __restrict__ partial) {
    __shared__ double part[kThreads];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float o = 1.0f / (1.0f + expf(-x[i]));
        const float u = 1.0f - o;
        const float lo = logf(o + kEps), lu = logf(u + kEps);
        acc += (double)(o * lo + u * lu);
        if (v_x) {
            const float d_o = (lo + o / (o + kEps)) - (lu + u / (u + kEps));
            v_x[i] = (scale * d_o) * u * o;
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    tree_sum(part);
    if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kThreads) void entropy_reduce_kernel(int blocks, int n, const double* __restrict__ partial,
                                                                  float* __restrict__ out) {
    __shared__ double part[kThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) acc += partial[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    tree_sum(part);
    if (threadIdx.x == 0) out[0] = (float)(-part[0] / (double)n);
}

}  // namespace

extern "C" {

int64_t ts_opacity_entropy_ws_bytes(int32_t n) {
    if (n < 1) return TS_E_BADARG;
    return (int64_t)entropy_blocks(n) * (int64_t)sizeof(double);
}

int ts_opacity_entropy(int32_t n, const float* opacities, float* loss, float* v_opacities, void* ws, void* stream) {
    if (n < 1 || !opacities || !loss || !ws) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = entropy_blocks(n);
    double* partial = (double*)ws;
    hipLaunchKernelGGL(entropy_kernel, dim3(blocks), dim3(kThreads), 0, s, (int)n, (float)(-1.0 / (double)n), opacities,
                       v_opacities, partial);
    hipLaunchKernelGGL(entropy_reduce_kernel, dim3(1), dim3(kThreads), 0, s, blocks, (int)n, (const double*)partial, loss);
    return launch_status();
}

}  // extern "C"
