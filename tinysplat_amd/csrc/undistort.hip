// undistort.hip - undistorts, recentres and downscales one uint8 RGB image (the arithmetic:
// undistort_math.h).
//
// One thread owns 4 consecutive pixels of the flat [H' W'] output order (a group may straddle a row end: every pixel
// derives its own (u, v)), so its 12 output bytes - or 48, for the float32 output - start on a multiple of 4 (16) bytes
// whatever the width, and leave as one three-dword store (three four-dword stores).  The last H' W' mod 4 pixels are
// written channel by channel by the thread that owns them.  The source is read by byte gathers, four taps of three bytes
// per sub-sample: neighbouring lanes read neighbouring source pixels, so the taps are served by the caches; nothing is
// staged in LDS.  No atomics, no LDS, no transcendentals; per output pixel the kernel writes 3 (12) bytes and the launch
// reads the part of the source the map covers once from memory.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "undistort_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 4;          // output pixels per thread

struct alignas(4) dword3 {
    uint32_t a, b, c;
};

template <bool kFloat>
__global__ __launch_bounds__(kThreads) void ts_undistort_kernel(ts_undistort_params p, const uint8_t* __restrict__ src,
                                                                void* __restrict__ out) {
    const int32_t total = p.out_h * p.out_w;                 // < 2^31: checked by the entry
    const int64_t group = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t first = group * kGroup;
    if (first >= total) return;
    if (first + kGroup <= total) {
        float lv[3 * kGroup];
        for (int k = 0; k < kGroup; ++k) ts_undistort_pixel(p, src, (int32_t)first + k, lv + 3 * k);
        if (kFloat) {
            float4* o = (float4*)out + 3 * group;
            o[0] = make_float4(lv[0] / 255.0f, lv[1] / 255.0f, lv[2] / 255.0f, lv[3] / 255.0f);
            o[1] = make_float4(lv[4] / 255.0f, lv[5] / 255.0f, lv[6] / 255.0f, lv[7] / 255.0f);
            o[2] = make_float4(lv[8] / 255.0f, lv[9] / 255.0f, lv[10] / 255.0f, lv[11] / 255.0f);
        } else {
            uint32_t w[3] = {0u, 0u, 0u};
            for (int k = 0; k < 3 * kGroup; ++k) w[k >> 2] |= ts_undistort_byte(lv[k]) << (8 * (k & 3));
            ((dword3*)out)[group] = dword3{w[0], w[1], w[2]};
        }
        return;
    }
    for (int64_t i = first; i < total; ++i) {                // the tail: fewer than 4 pixels, one thread of the launch
        float lv[3];
        ts_undistort_pixel(p, src, (int32_t)i, lv);
        for (int c = 0; c < 3; ++c) {
            if (kFloat) ((float*)out)[3 * i + c] = lv[c] / 255.0f;
            else ((uint8_t*)out)[3 * i + c] = (uint8_t)ts_undistort_byte(lv[c]);
        }
    }
}

}  // namespace

extern "C" {

int ts_undistort_image(const uint8_t* src, int32_t src_h, int32_t src_w, const float* src_k, const float* dst_k,
                       const float* dist, int32_t out_h, int32_t out_w, int32_t out_float, void* out, void* stream) {
    if (!src || !src_k || !dst_k || !dist || !out) return TS_E_BADARG;
    if (src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return TS_E_BADARG;
    if ((int64_t)src_h * src_w >= (int64_t)1 << 31 || (int64_t)out_h * out_w >= (int64_t)1 << 31) return TS_E_BADARG;
    if (((uintptr_t)out & 15u) != 0) return TS_E_BADARG;     // the vector stores
    ts_undistort_params p;
    for (int i = 0; i < 4; ++i) {
        p.src_k[i] = src_k[i];
        p.dst_k[i] = dst_k[i];
    }
    for (int i = 0; i < 8; ++i) p.d[i] = dist[i];
    p.src_h = src_h;
    p.src_w = src_w;
    p.out_h = out_h;
    p.out_w = out_w;
    p.n = ts_undistort_supersample(src_w, src_h, out_w, out_h);
    const int64_t groups = ((int64_t)out_h * out_w + kGroup - 1) / kGroup;
    const dim3 grid((unsigned)nblocks(groups, kThreads)), block(kThreads);
    if (out_float)
        hipLaunchKernelGGL(ts_undistort_kernel<true>, grid, block, 0, (hipStream_t)stream, p, src, out);
    else
        hipLaunchKernelGGL(ts_undistort_kernel<false>, grid, block, 0, (hipStream_t)stream, p, src, out);
    return launch_status();
}

}  // extern "C"
