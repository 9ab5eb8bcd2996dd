// splatfile.hip - the 32-byte .splat record of the WebGL viewers (the arithmetic: splat_record.h).
//
// Export: ts_splat_keys writes every Gaussian's importance, the host sorts them (formats.py: splat_order), and
// ts_splat_pack runs one thread per OUTPUT record: lane i gathers Gaussian order[i] from the five tensors (56 bytes in
// five places, the scattered side) and stores record i as two 16-byte words, so a wave writes 2 KiB of the buffer end to
// end.  Import: ts_splat_unpack, one thread per record, two 16-byte loads and the five tensors' rows written in place.
// No atomics, no LDS, no scratch; per record 56 B read + 8 B of index + 32 B written.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "splat_record.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void ts_splat_keys_kernel(long long n, const float* __restrict__ scales,
                                                                 const float* __restrict__ opacities,
                                                                 float* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    keys[i] = ts_splat_key(s, opacities[i]);
}

__global__ __launch_bounds__(kThreads) void ts_splat_pack_kernel(long long n, long long m,
                                                                 const float* __restrict__ means,
                                                                 const float* __restrict__ scales,
                                                                 const float* __restrict__ dc,
                                                                 const float* __restrict__ opacities,
                                                                 const float* __restrict__ quats,
                                                                 const long long* __restrict__ order,
                                                                 uint4* __restrict__ records) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const long long g = order ? order[i] : i;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (g >= 0 && g < n) {                      // an index outside the model: a record of zeros, nothing is read
        const float p[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
        const float s[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
        const float c[3] = {dc[3 * g], dc[3 * g + 1], dc[3 * g + 2]};
        const float q[4] = {quats[4 * g], quats[4 * g + 1], quats[4 * g + 2], quats[4 * g + 3]};
        const ts_splat_words r = ts_splat_encode(p, s, c, opacities[g], q);
        lo = make_uint4(r.lo[0], r.lo[1], r.lo[2], r.lo[3]);
        hi = make_uint4(r.hi[0], r.hi[1], r.hi[2], r.hi[3]);
    }
    records[2 * i] = lo;
    records[2 * i + 1] = hi;
}

__global__ __launch_bounds__(kThreads) void ts_splat_unpack_kernel(long long n, const uint4* __restrict__ records,
                                                                   float* __restrict__ means, float* __restrict__ scales,
                                                                   float* __restrict__ dc, float* __restrict__ opacities,
                                                                   float* __restrict__ quats) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 lo = records[2 * i], hi = records[2 * i + 1];
    const ts_splat_words r{{lo.x, lo.y, lo.z, lo.w}, {hi.x, hi.y, hi.z, hi.w}};
    float p[3], s[3], c[3], o, q[4];
    ts_splat_decode(r, p, s, c, &o, q);
    for (int k = 0; k < 3; ++k) {
        means[3 * i + k] = p[k];
        scales[3 * i + k] = s[k];
        dc[3 * i + k] = c[k];
    }
    opacities[i] = o;
    for (int k = 0; k < 4; ++k) quats[4 * i + k] = q[k];
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int ts_splat_keys(int32_t n, const float* scales, const float* opacities, float* keys, void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!scales || !opacities || !keys) return TS_E_BADARG;
    hipLaunchKernelGGL(ts_splat_keys_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (long long)n, scales, opacities, keys);
    return launch_status();
}

int ts_splat_pack(int32_t n, int32_t m, const float* means, const float* scales, const float* colors_dc,
                  const float* opacities, const float* quats, const int64_t* order, void* records, void* stream) {
    if (n < 0 || m < 0 || (!order && m > n)) return TS_E_BADARG;
    if (m == 0) return 0;
    if (!means || !scales || !colors_dc || !opacities || !quats || !records || !aligned16(records))
        return TS_E_BADARG;
    hipLaunchKernelGGL(ts_splat_pack_kernel, dim3((unsigned)nblocks(m, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (long long)n, (long long)m, means, scales, colors_dc, opacities, quats,
                       (const long long*)order, (uint4*)records);
    return launch_status();
}

int ts_splat_unpack(int32_t n, const void* records, float* means, float* scales, float* colors_dc, float* opacities,
                    float* quats, void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!records || !aligned16(records) || !means || !scales || !colors_dc || !opacities || !quats)
        return TS_E_BADARG;
    hipLaunchKernelGGL(ts_splat_unpack_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (long long)n, (const uint4*)records, means, scales, colors_dc, opacities,
                       quats);
    return launch_status();
}

}  // extern "C"
