// depth_prior.hip - depth priors: the scale matching of tinysplat/depth.py for all cameras of a
// dataset in one batch.  The arithmetic of a point, a key and a sample is depth_prior_math.h's.
//
//   project   one thread per (camera, visible point): the point's pixel as a 64-bit sort key, its depth z and its weight
//             1 / error.  The keys are sorted outside (torch.sort); a dropped point sorts behind its camera's kept ones, so
//             a camera's entries stay in its span of the list
//   mark      one thread per sorted entry: 1 for the last entry of a (camera, pixel) run - the point the reference's
//             lil_matrix keeps - 0 for the others and for dropped points.  The flags are summed outside (torch.cumsum)
//   gather    one thread per sorted entry: a survivor moves to the slot its running count names, with the dense map's value
//             at its pixel; the survivors are then in the reference's order (tocoo(): row-major)
//   fit       one workgroup per camera, double throughout: minimises f(s, t) = (1/m) sum w_i |y_i - s x_i - t| exactly.
//             For a slope s the best t is the lower weighted median of the residuals r_i = y_i - s x_i (one fma each, so
//             that rounding never inverts the order of two residuals), found by a radix select over the order-preserving
//             integer images of the r_i: 64 passes of one bit, each a block-wide sum of weights - no storage proportional
//             to m, no limit on m.  The one-sided derivatives of g(s) = min_t f(s, t) at s then say whether the optimum
//             lies left or right or here; the search brackets from the weighted least-squares slope and bisects down to
//             adjacent doubles.
//   apply     one thread per 4 pixels: target = float32(double(s) * sample + double(t)), or its reciprocal in disparity
//             space; s and t are read from the fit's row on the device.
//
// No atomics; every sum has a fixed order (a thread's elements in index order, the wave by xor butterfly, the four waves
// in index order), so the same inputs give the same bytes on every run and in every batch.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "depth_prior_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kGroup = 4;                  // target pixels per thread
constexpr int kMaxDoublings = 128;         // of the bracket's step: 2^-10 max(|s0|, 1) .. 2^118 max(|s0|, 1)

__global__ __launch_bounds__(kThreads) void depth_project_kernel(int32_t cameras, int64_t n, int64_t points,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const int64_t* __restrict__ indices,
                                                                 const float* __restrict__ xyz,
                                                                 const double* __restrict__ errors,
                                                                 const float* __restrict__ cam_f,
                                                                 const int32_t* __restrict__ cam_size,
                                                                 int64_t* __restrict__ keys, float* __restrict__ z_out,
                                                                 double* __restrict__ w_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int32_t lo = 0, hi = cameras;                             // the camera c with offsets[c] <= i < offsets[c + 1]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int32_t c = lo;
    const int32_t position = (int32_t)(i - offsets[c]);
    const int64_t p = indices[i];
    float z = 0.0f;
    double w = 0.0;
    int64_t pixel = TS_DEPTH_NO_PIXEL;
    if (p >= 0 && p < points) {
        const double e = errors[p];
        pixel = ts_depth_project(cam_f + (int64_t)TS_DEPTH_CAM_FLOATS * c, cam_size[2 * c], cam_size[2 * c + 1],
                                 xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], e, &z);
        w = 1.0 / e;
    }
    keys[i] = ts_depth_key(c, pixel, position);
    z_out[i] = z;
    w_out[i] = pixel == TS_DEPTH_NO_PIXEL ? 0.0 : w;
}

__global__ __launch_bounds__(kThreads) void depth_mark_kernel(int64_t n, const int64_t* __restrict__ sorted_keys,
                                                              int64_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t key = sorted_keys[i];
    const bool kept = ts_depth_key_pixel(key) != TS_DEPTH_NO_PIXEL;
    const bool last = i == n - 1 || ts_depth_key_run(sorted_keys[i + 1]) != ts_depth_key_run(key);
    flags[i] = kept && last ? 1 : 0;
}

// maps: NULL, or one device address per camera (0: no map, x = NaN) with map_size[2 c] = {rows, columns}
__global__ __launch_bounds__(kThreads) void depth_gather_kernel(int64_t n, const int64_t* __restrict__ sorted_keys,
                                                                const int64_t* __restrict__ order,
                                                                const int64_t* __restrict__ flags,
                                                                const int64_t* __restrict__ running,
                                                                const float* __restrict__ z_in,
                                                                const double* __restrict__ w_in,
                                                                const int64_t* __restrict__ maps,
                                                                const int32_t* __restrict__ map_size,
                                                                const int32_t* __restrict__ cam_size,
                                                                int32_t* __restrict__ pixel_out, float* __restrict__ z_out,
                                                                double* __restrict__ w_out, float* __restrict__ x_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || flags[i] == 0) return;
    const int64_t slot = running[i] - 1;                      // inclusive count of survivors up to i: 1 <= running[i] <= n
    const int64_t key = sorted_keys[i], src = order[i];       // order: a permutation of 0 .. n - 1
    const int32_t c = ts_depth_key_camera(key);
    const int64_t pixel = ts_depth_key_pixel(key);
    pixel_out[slot] = (int32_t)pixel;
    z_out[slot] = z_in[src];
    w_out[slot] = w_in[src];
    if (maps) {
        const float* map = reinterpret_cast<const float*>(maps[c]);
        const int32_t width = cam_size[2 * c], height = cam_size[2 * c + 1];
        x_out[slot] = map ? ts_depth_sample_dense(map, map_size[2 * c], map_size[2 * c + 1], height, width,
                                                  (int32_t)(pixel % width), (int32_t)(pixel / width))
                          : __builtin_nanf("");
    }
}

// ---------------------------------------------------------------------------------------------------------------- fit
struct SumOp { __device__ double operator()(double a, double b) const { return a + b; } };
struct MinOp { __device__ double operator()(double a, double b) const { return b < a ? b : a; } };

// every thread leaves with the block's result; slots are double-buffered, so one barrier per reduction is enough
struct Reducer {
    double (*slots)[kFitWaves][5];
    int phase;
    template <int N, typename Op>
    __device__ void run(double (&v)[N], Op op) {
        static_assert(N <= 5, "slots");
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = op(v[k], __shfl_xor(v[k], d, 64));
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < N; ++k) slots[phase][wave][k] = v[k];
        __syncthreads();
        for (int k = 0; k < N; ++k) {
            double r = slots[phase][0][k];
            for (int q = 1; q < kFitWaves; ++q) r = op(r, slots[phase][q][k]);
            v[k] = r;
        }
        phase ^= 1;
    }
};

struct FitData {
    const float* x;
    const float* z;
    const double* w;
    int64_t m;
    int disparity;
    __device__ double xv(int64_t i) const { return (double)x[i]; }
    __device__ double yv(int64_t i) const { return disparity ? 1.0 / (double)z[i] : (double)z[i]; }
    __device__ double residual(double s, int64_t i) const { return __builtin_fma(-s, xv(i), yv(i)) + 0.0; }
};

struct Eval {
    double t, f, G, slack;
};

// t(s), f(s, t(s)) and the two sums of the derivative test
__device__ Eval evaluate(const FitData& d, double s, double half_w, Reducer& red) {
    uint64_t prefix = 0;
    double below = 0.0;
    for (int bit = 63; bit >= 0; --bit) {
        const uint64_t decided = bit == 63 ? 0ull : ~0ull << (bit + 1), b = 1ull << bit;
        double v[3] = {0.0, 0.0, 0.0};                        // weight and number with the bit clear, number with it set
        for (int64_t i = threadIdx.x; i < d.m; i += kFitThreads) {
            const uint64_t key = ts_depth_order_key(d.residual(s, i));
            if ((key & decided) != prefix) continue;
            if (key & b) v[2] += 1.0;
            else { v[0] += d.w[i]; v[1] += 1.0; }
        }
        red.run(v, SumOp());
        // the median is among the candidates with the bit clear if their weight reaches the half; a branch without
        // candidates is never taken, whatever rounding did to the sums
        const bool clear = v[2] == 0.0 || (v[1] > 0.0 && below + v[0] >= half_w);
        if (!clear) { below += v[0]; prefix |= b; }
    }
    Eval e;
    e.t = ts_depth_order_value(prefix);
    double first[1] = {(double)d.m};
    for (int64_t i = threadIdx.x; i < d.m; i += kFitThreads)
        if (ts_depth_order_key(d.residual(s, i)) == prefix) { first[0] = (double)i; break; }
    red.run(first, MinOp());
    // < m: the prefix is the image of a residual (the clamp keeps a read in bounds should that ever fail)
    const int64_t k = first[0] < (double)d.m ? (int64_t)first[0] : d.m - 1;
    const double xk = d.xv(k);
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < d.m; i += kFitThreads) {
        const double r = d.residual(s, i), w = d.w[i], dx = d.xv(i) - xk;
        if (r > e.t) v[0] -= w * dx;
        else if (r < e.t) v[0] += w * dx;
        else if (i != k) v[1] += w * fabs(dx);
        v[2] += w * fabs(r - e.t);
    }
    red.run(v, SumOp());
    e.G = v[0];
    e.slack = v[1];
    e.f = v[2] / (double)d.m;
    return e;
}

// -1: the optimum lies at smaller s; +1: at larger s; 0: here
__device__ int direction(const Eval& e) { return e.G > e.slack ? -1 : (e.G < -e.slack ? 1 : 0); }

__global__ __launch_bounds__(kFitThreads) void depth_fit_kernel(const int64_t* __restrict__ offsets,
                                                                const float* __restrict__ x, const float* __restrict__ z,
                                                                const double* __restrict__ w, int disparity,
                                                                double* __restrict__ fits) {
    __shared__ double slots[2][kFitWaves][5];
    Reducer red{slots, 0};
    const int c = blockIdx.x;
    const int64_t begin = offsets[c];
    FitData d{x + begin, z + begin, w + begin, offsets[c + 1] - begin, disparity};
    double* out = fits + (int64_t)TS_DEPTH_FIT_DOUBLES * c;
    const double nan = __builtin_nan("");
    auto write = [&](double s, double t, double f, int evals, int status) {
        if (threadIdx.x == 0) {
            out[0] = s; out[1] = t; out[2] = f; out[3] = (double)d.m; out[4] = (double)evals; out[5] = (double)status;
        }
    };
    if (d.m <= 0) { write(nan, nan, nan, 0, TS_DEPTH_FIT_NO_POINTS); return; }

    double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};               // w, w x, w y, w x x, w x y
    double ext[2] = {(double)INFINITY, (double)INFINITY};     // min x, min -x
    for (int64_t i = threadIdx.x; i < d.m; i += kFitThreads) {
        const double wi = d.w[i], xi = d.xv(i), yi = d.yv(i);
        sums[0] += wi; sums[1] += wi * xi; sums[2] += wi * yi; sums[3] += wi * xi * xi; sums[4] += wi * xi * yi;
        ext[0] = xi < ext[0] ? xi : ext[0];
        ext[1] = -xi < ext[1] ? -xi : ext[1];
    }
    red.run(sums, SumOp());
    red.run(ext, MinOp());
    bool finite = true;
    for (int k = 0; k < 5; ++k) finite = finite && fabs(sums[k]) <= 1.7976931348623157e308;
    if (!finite) { write(nan, nan, nan, 0, TS_DEPTH_FIT_NOT_FINITE); return; }
    const double half_w = 0.5 * sums[0];
    if (ext[0] == -ext[1]) {
        const Eval e = evaluate(d, 1.0, half_w, red);
        write(1.0, e.t, e.f, 1, TS_DEPTH_FIT_EQUAL_X);
        return;
    }
    double s = (sums[0] * sums[4] - sums[1] * sums[2]) / (sums[0] * sums[3] - sums[1] * sums[1]);
    if (!(fabs(s) <= 1.7976931348623157e308)) s = 1.0;
    Eval e = evaluate(d, s, half_w, red);
    int evals = 1, status = TS_DEPTH_FIT_OK;
    const int dir = direction(e);
    if (dir != 0) {
        double step = fmax(fabs(s), 1.0) * 0x1p-10, lo = 0.0, hi = 0.0;
        Eval elo = e, ehi = e;
        bool bracketed = false, stopped = false;
        for (int k = 0; k < kMaxDoublings; ++k) {
            const double next = s + (double)dir * step;
            const Eval en = evaluate(d, next, half_w, red);
            ++evals;
            const int dn = direction(en);
            if (dn == 0) { s = next; e = en; stopped = true; break; }
            if (dn != dir) {
                if (dir < 0) { lo = next; elo = en; hi = s; ehi = e; }
                else { lo = s; elo = e; hi = next; ehi = en; }
                bracketed = true;
                break;
            }
            s = next; e = en; step *= 2.0;
        }
        if (!stopped && !bracketed) status = TS_DEPTH_FIT_BRACKET_CAP;
        while (bracketed) {
            const double mid = lo + (hi - lo) * 0.5;
            if (!(mid > lo && mid < hi)) {                    // adjacent doubles: the better end
                if (ehi.f < elo.f) { s = hi; e = ehi; } else { s = lo; e = elo; }
                status = TS_DEPTH_FIT_ADJACENT;
                break;
            }
            const Eval em = evaluate(d, mid, half_w, red);
            ++evals;
            const int dm = direction(em);
            if (dm == 0) { s = mid; e = em; break; }
            if (dm < 0) { hi = mid; ehi = em; } else { lo = mid; elo = em; }
        }
    }
    write(s, e.t, e.f, evals, status);
}

// -------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(kThreads) void depth_apply_kernel(const float* __restrict__ map, int32_t h, int32_t w,
                                                               int32_t height, int32_t width,
                                                               const double* __restrict__ fit, int32_t disparity,
                                                               float* __restrict__ out) {
    const int64_t total = (int64_t)height * width;            // < 2^28: checked by the entry
    const int64_t first = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kGroup;
    if (first >= total) return;
    const double s = fit[0], t = fit[1];
    float v[kGroup];
    const int count = total - first < kGroup ? (int)(total - first) : kGroup;
    for (int k = 0; k < count; ++k) {
        const int64_t p = first + k;
        v[k] = ts_depth_apply(s, t, ts_depth_sample_dense(map, h, w, height, width, (int32_t)(p % width), (int32_t)(p / width)),
                              disparity);
    }
    if (count == kGroup) *reinterpret_cast<float4*>(out + first) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; k < count; ++k) out[first + k] = v[k];
}

}  // namespace

extern "C" {

int ts_depth_prior_project(int32_t cameras, int64_t n, int64_t points, const int64_t* offsets, const int64_t* indices,
                           const float* xyz, const double* errors, const float* cam_f, const int32_t* cam_size,
                           int64_t* keys, float* z, double* w, void* stream) {
    if (cameras < 0 || cameras > (1 << TS_DEPTH_CAMERA_BITS) || n < 0 || points < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (cameras == 0 || !offsets || !indices || !cam_f || !cam_size || !keys || !z || !w) return TS_E_BADARG;
    if (points > 0 && (!xyz || !errors)) return TS_E_BADARG;
    const int64_t blocks = nblocks(n, kThreads);
    if (blocks > INT32_MAX) return TS_E_BADARG;
    hipLaunchKernelGGL(depth_project_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, cameras, n,
                       points, offsets, indices, xyz, errors, cam_f, cam_size, keys, z, w);
    return launch_status();
}

int ts_depth_prior_mark(int64_t n, const int64_t* sorted_keys, int64_t* flags, void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!sorted_keys || !flags) return TS_E_BADARG;
    const int64_t blocks = nblocks(n, kThreads);
    if (blocks > INT32_MAX) return TS_E_BADARG;
    hipLaunchKernelGGL(depth_mark_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, n, sorted_keys,
                       flags);
    return launch_status();
}

int ts_depth_prior_gather(int64_t n, const int64_t* sorted_keys, const int64_t* order, const int64_t* flags,
                          const int64_t* running, const float* z_in, const double* w_in, const int64_t* maps,
                          const int32_t* map_size, const int32_t* cam_size, int32_t* pixel, float* z, double* w, float* x,
                          void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!sorted_keys || !order || !flags || !running || !z_in || !w_in || !cam_size || !pixel || !z || !w) return TS_E_BADARG;
    if (maps && (!map_size || !x)) return TS_E_BADARG;
    const int64_t blocks = nblocks(n, kThreads);
    if (blocks > INT32_MAX) return TS_E_BADARG;
    hipLaunchKernelGGL(depth_gather_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, n, sorted_keys,
                       order, flags, running, z_in, w_in, maps, map_size, cam_size, pixel, z, w, x);
    return launch_status();
}

int ts_depth_prior_fit(int32_t cameras, const int64_t* offsets, const float* x, const float* z, const double* w,
                       int32_t disparity, double* fits, void* stream) {
    if (cameras < 0) return TS_E_BADARG;
    if (cameras == 0) return 0;
    if (!offsets || !fits || (uintptr_t)fits % sizeof(double) || (uintptr_t)w % sizeof(double)) return TS_E_BADARG;
    hipLaunchKernelGGL(depth_fit_kernel, dim3((unsigned)cameras), dim3(kFitThreads), 0, (hipStream_t)stream, offsets, x, z,
                       w, (int)(disparity != 0), fits);
    return launch_status();
}

int ts_depth_prior_apply(const float* map, int32_t map_h, int32_t map_w, int32_t height, int32_t width, const double* fit,
                         int32_t disparity, float* out, void* stream) {
    if (!map || !fit || !out || map_h < 1 || map_w < 1 || height < 1 || width < 1) return TS_E_BADARG;
    if ((int64_t)height * width >= TS_DEPTH_NO_PIXEL || (int64_t)map_h * map_w >= (int64_t)1 << 31) return TS_E_BADARG;
    if (((uintptr_t)out & 15u) != 0 || (uintptr_t)fit % sizeof(double)) return TS_E_BADARG;
    const int64_t groups = ((int64_t)height * width + kGroup - 1) / kGroup;
    hipLaunchKernelGGL(depth_apply_kernel, dim3((unsigned)nblocks(groups, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, map, map_h, map_w, height, width, fit, (int)(disparity != 0), out);
    return launch_status();
}

}  // extern "C"
