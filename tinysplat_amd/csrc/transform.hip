// transform.hip - a similarity transform of a model's Gaussians and the box test of a crop (the
// arithmetic: transform_math.h).
//
// ts_transform_gaussians is a stream: per Gaussian it reads and writes 12 + 12 + 16 bytes of mean, log-scale and
// quaternion and 12 k_rest bytes of colors_rest.  A wave owns 64 consecutive Gaussians.  Their colors_rest rows are one
// contiguous block of 64 * 3 k_rest floats, which the wave moves through LDS: lanes load consecutive addresses (16 bytes
// each where the block is 16-byte aligned) and store them at the row stride of the LDS copy, each lane then rotates the
// row of its own Gaussian in LDS, and the block goes back the way it came.  A row is 9 / 24 / 45 / 72 floats; the even
// ones are padded by one float so that the 64 lanes' rows start on distinct banks.  M, t, r, log s and the D_l are kernel
// arguments, the same for every lane.  One instantiation per number of bands; a partial last wave moves and rotates only
// the rows that exist; the grid covers every Gaussian (no cap, no grid stride).  No atomics: every value is written once
// by one lane, so the result is the same bits on every run.  A wave reads its whole block before it writes any of it
// and writes only its own rows, so every output may be its input.
//
// ts_box_mask: one thread per Gaussian, 12 bytes read and one written.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "transform_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;

struct ts_box_params {
    float a[9];
    float b[3];
};

// floats of a row in LDS: odd, so that consecutive rows start one bank apart modulo an odd step
constexpr int lds_stride(int row_floats) { return row_floats | 1; }

// the wave's block of `total` floats between global memory and its LDS rows (R floats a row, S apart); lanes take
// consecutive addresses, 16 bytes each where `vec` (the block starts on 16 bytes), the tail and the rest 4 bytes each
template <int R, int S, bool kStore>
__device__ __forceinline__ void move_block(float* glob, float* rows, int total, int lane, bool vec) {
    int done = 0;
    if (vec) {
        const int quads = total >> 2;
#pragma unroll 4
        for (int v = lane; v < quads; v += kWave) {
            const int e = 4 * v;
            if constexpr (kStore) {
                float4 x;
                x.x = rows[(e / R) * S + e % R];
                x.y = rows[((e + 1) / R) * S + (e + 1) % R];
                x.z = rows[((e + 2) / R) * S + (e + 2) % R];
                x.w = rows[((e + 3) / R) * S + (e + 3) % R];
                reinterpret_cast<float4*>(glob)[v] = x;
            } else {
                const float4 x = reinterpret_cast<const float4*>(glob)[v];
                rows[(e / R) * S + e % R] = x.x;
                rows[((e + 1) / R) * S + (e + 1) % R] = x.y;
                rows[((e + 2) / R) * S + (e + 2) % R] = x.z;
                rows[((e + 3) / R) * S + (e + 3) % R] = x.w;
            }
        }
        done = 4 * quads;
    }
    for (int e = done + lane; e < total; e += kWave) {
        if constexpr (kStore) glob[e] = rows[(e / R) * S + e % R];
        else rows[(e / R) * S + e % R] = glob[e];
    }
}

template <int BANDS>
__global__ __launch_bounds__(kThreads) void ts_transform_kernel(int n, const ts_xf_params p,
                                                                const uint8_t* __restrict__ mask,
                                                                const float* means, const float* scales,
                                                                const float* quats, const float* rest,
                                                                float* means_out, float* scales_out, float* quats_out,
                                                                float* rest_out) {
    constexpr int R = 3 * BANDS * (BANDS + 2);          // floats of a colors_rest row
    constexpr int S = lds_stride(R);
    __shared__ float lds[BANDS > 0 ? kWaves * kWave * S : 1];

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const long long first = ((long long)blockIdx.x * kWaves + wave) * kWave;   // the wave's first Gaussian
    const int count = first >= n ? 0 : (n - first < kWave ? (int)(n - first) : kWave);
    const long long g = first + lane;
    const bool mine = lane < count;
    const bool on = mine && (!mask || mask[g] != 0);

    // the small tensors: every input of the row is in registers before its outputs are stored
    float m[3], s[3], q[4];
    if (mine) {
        for (int k = 0; k < 3; ++k) m[k] = means[3 * g + k];
        for (int k = 0; k < 3; ++k) s[k] = scales[3 * g + k];
        for (int k = 0; k < 4; ++k) q[k] = quats[4 * g + k];
    }
    if constexpr (BANDS > 0) {
        float* rows = lds + wave * kWave * S;
        const long long base = first * R;
        const int total = count * R;
        const bool vec = (((uintptr_t)(rest + base) | (uintptr_t)(rest_out + base)) & 15u) == 0;
        move_block<R, S, false>(const_cast<float*>(rest) + base, rows, total, lane, vec);
        __syncthreads();
        if (on) ts_xf_sh_row<BANDS>(p.sh, rows + lane * S);
        __syncthreads();
        move_block<R, S, true>(rest_out + base, rows, total, lane, vec);
    }
    if (on) {
        ts_xf_mean(p.m, p.t, m, m);
        ts_xf_scale(p.log_scale, s, s);
        ts_xf_quat(p.r, q, q);
    }
    if (mine) {
        for (int k = 0; k < 3; ++k) means_out[3 * g + k] = m[k];
        for (int k = 0; k < 3; ++k) scales_out[3 * g + k] = s[k];
        for (int k = 0; k < 4; ++k) quats_out[4 * g + k] = q[k];
    }
}

__global__ __launch_bounds__(kThreads) void ts_box_mask_kernel(int n, const ts_box_params p,
                                                               const float* __restrict__ means,
                                                               uint8_t* __restrict__ inside) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    inside[i] = ts_xf_inside(p.a, p.b, m) ? 1 : 0;
}

inline bool all_finite(const float* v, int count) {
    for (int i = 0; i < count; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

template <int BANDS>
void launch_transform(int32_t n, const ts_xf_params& p, const uint8_t* mask, const float* means, const float* scales,
                      const float* quats, const float* rest, float* means_out, float* scales_out, float* quats_out,
                      float* rest_out, hipStream_t stream) {
    hipLaunchKernelGGL(ts_transform_kernel<BANDS>, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, stream,
                       (int)n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out);
}

}  // namespace

extern "C" {

int ts_transform_gaussians(int32_t n, int32_t k_rest, const float* xform_host, const float* quat_host, float log_scale,
                           const float* sh_host, const uint8_t* mask, const float* means, const float* scales,
                           const float* quats, const float* colors_rest, float* means_out, float* scales_out,
                           float* quats_out, float* colors_rest_out, void* stream) {
    const int bands = ts_xf_bands(k_rest);
    if (n < 0 || bands < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!xform_host || !quat_host || (bands > 0 && !sh_host)) return TS_E_BADARG;
    if (!means || !scales || !quats || !means_out || !scales_out || !quats_out) return TS_E_BADARG;
    if (bands > 0 && (!colors_rest || !colors_rest_out)) return TS_E_BADARG;
    const int sh_floats = bands > 0 ? ts_xf_sh_offset(bands) + (2 * bands + 1) * (2 * bands + 1) : 0;
    if (!all_finite(xform_host, 12) || !all_finite(quat_host, 4) || !isfinite(log_scale) ||
        !all_finite(sh_host, sh_floats))
        return TS_E_BADARG;
    ts_xf_params p = {};
    for (int i = 0; i < 9; ++i) p.m[i] = xform_host[i];
    for (int i = 0; i < 3; ++i) p.t[i] = xform_host[9 + i];
    for (int i = 0; i < 4; ++i) p.r[i] = quat_host[i];
    p.log_scale = log_scale;
    for (int i = 0; i < sh_floats; ++i) p.sh[i] = sh_host[i];
    const hipStream_t st = (hipStream_t)stream;
    switch (bands) {
        case 0: launch_transform<0>(n, p, mask, means, scales, quats, colors_rest, means_out, scales_out, quats_out,
                                    colors_rest_out, st); break;
        case 1: launch_transform<1>(n, p, mask, means, scales, quats, colors_rest, means_out, scales_out, quats_out,
                                    colors_rest_out, st); break;
        case 2: launch_transform<2>(n, p, mask, means, scales, quats, colors_rest, means_out, scales_out, quats_out,
                                    colors_rest_out, st); break;
        case 3: launch_transform<3>(n, p, mask, means, scales, quats, colors_rest, means_out, scales_out, quats_out,
                                    colors_rest_out, st); break;
        default: launch_transform<4>(n, p, mask, means, scales, quats, colors_rest, means_out, scales_out, quats_out,
                                     colors_rest_out, st); break;
    }
    return launch_status();
}

int ts_box_mask(int32_t n, const float* box_host, const float* means, uint8_t* inside, void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!box_host || !means || !inside || !all_finite(box_host, 12)) return TS_E_BADARG;
    ts_box_params p;
    for (int i = 0; i < 9; ++i) p.a[i] = box_host[i];
    for (int i = 0; i < 3; ++i) p.b[i] = box_host[9 + i];
    hipLaunchKernelGGL(ts_box_mask_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, p, means, inside);
    return launch_status();
}

}  // extern "C"
