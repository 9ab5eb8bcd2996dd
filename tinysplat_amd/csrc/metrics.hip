// metrics.hip - the quality of one rendered image against one target: mean squared error, mean
// absolute error, SSIM and PSNR as four device doubles.  What the reference prints per epoch (scripts/train.py:108-119:
// model.psnr = torchmetrics' PeakSignalNoiseRatio(data_range=1.0), the L1 and SSIM parts of its loss), here for views
// held out of training.
//
// One launch reads the image (12 or 16 bytes per pixel) and the target (3 bytes per pixel as uint8, 12 as float32) and
// writes three doubles per wave; a second launch of one workgroup sums them in a fixed order.  No map is written: the
// training loss's forward (train.hip, ssim_fwd_rows_kernel) stores three derivative maps for its backward pass, 36 bytes
// per map location, which an evaluation has no use for.  The window walk is that kernel's: one wave per 64 map columns,
// channel and `seg` map rows, a pixel row filtered horizontally through a wave-private LDS line, the eleven most recent
// filtered rows of the five maps in a register ring.  The squared and absolute errors are summed per lane in double; a
// lane's SSIM terms (at most 64 values of magnitude <= 1) in float32, as the training kernel sums them, and in double
// from the wave's sum on.
//
// The result is a function of the two images alone: the segmentation comes from (H, W) (metrics_math.h), every wave
// writes its own slot, and the reduction reads the slots in index order - no atomics, no device query.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "gauss_window.h"
#include "metrics_math.h"
#include "mask_math.h"

#include <type_traits>

namespace {

constexpr int kWin = TS_METRICS_WIN, kHalo = TS_METRICS_HALO, kCols = TS_METRICS_COLS, kWaves = TS_METRICS_CHANNELS;
constexpr int kLine = kCols + 16;          // LDS line: 74 pixels used
constexpr int kReduceThreads = 256;

#define TS_METRICS_WAVE_SYNC()                                    \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <typename T>
struct RowRegs { float xm, xe; T ym, ye; };            // one pixel row of a wave: main / extra columns of X and Y
template <typename T>
struct RowRegsMasked : RowRegs<T> { uint8_t mm, me; }; // ... and their mask bytes

// T: the target's element, float or uint8_t (a byte becomes lut[b] = b / 255.0f, one division per value and workgroup).
// X has `xs` floats per pixel (channel 3 of the compositing kernels' RGB + depth output is never read).
// partials[3 * wave]: {sum of S over the wave's map locations, sum of (x - y)^2, sum of |x - y|}; every element's error
// is counted by exactly one wave: its own rows and main columns, the last segment / column block also the ten trailing
// rows / columns nobody else starts at.
//
// kMasked: M is a uint8 [H, W] mask of weights m = byte / 255 (the target bytes' table: the same
// quotient).  The errors become m (x - y)^2 and m |x - y|, the SSIM term is taken on the substituted image
// X' = blend(X, Y, m) (mask_math.h) and weighed by the weight m_c of its window's centre pixel, and a wave writes
// TS_METRICS_MASKED_PARTIALS doubles: behind the three sums, the sum of m over the pixels it owns and the sum of m_c over
// its map locations - both by the first channel's wave alone, the other two write zeros.  The centre weights come from a
// ring of the wave's last twelve mask rows in LDS: the centre row of map row t - 10 was fetched five rows ago.
template <typename T, bool kMasked>
__device__ __forceinline__ void image_metrics_rows_body(int H, int W, int xs, int seg,
                                                        const float* __restrict__ X,
                                                        const T* __restrict__ Y,
                                                        const uint8_t* __restrict__ M,
                                                        double* __restrict__ partials) {
    constexpr bool kBytes = sizeof(T) == 1;
    constexpr int kCentre = kHalo / 2;                         // the window's centre: five rows and columns in
    __shared__ float line[kWaves][2][2][kLine];                // [channel wave][parity][X | Y][column]
    __shared__ float lut[256];
    constexpr float g[kWin] = {TS_GAUSS_WINDOW};
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (kBytes || kMasked) {
        for (int i = threadIdx.x; i < 256; i += 64 * kWaves) lut[i] = ts_metrics_byte_to_float((uint8_t)i);
        __syncthreads();
    }
    auto value = [&](T v) -> float {
        if constexpr (kBytes) return lut[v]; else return v;
    };
    const int Ho = H - kHalo, Wo = W - kHalo;
    const int x0 = blockIdx.x * kCols, o0 = blockIdx.y * seg;
    const int rows = min(seg, Ho - o0);                        // map rows of this wave (>= 1)
    const bool last_block = blockIdx.x == gridDim.x - 1, last_seg = blockIdx.y == gridDim.y - 1;
    const int xa = x0 + lane, xb = x0 + kCols + lane;
    const bool in_a = xa < W, in_b = lane < kHalo && xb < W;
    const size_t slot = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kWaves + c;
    // branch-free loads (columns beyond the image read the last pixel of the row and are zeroed where they are used)
    const int xa_c = min(xa, W - 1), xb_c = min(xb, W - 1);
    // the lane's part of every address is a 32-bit byte offset inside the row (a row has fewer than 2^31 bytes: the
    // entry checks); the row's base is wave-uniform and stays in scalar registers
    const unsigned xa_o = 4u * (unsigned)(xa_c * xs + c), xb_o = 4u * (unsigned)(xb_c * xs + c);
    const unsigned ya_o = (unsigned)sizeof(T) * (unsigned)(xa_c * 3 + c), yb_o = (unsigned)sizeof(T) * (unsigned)(xb_c * 3 + c);
    using Regs = std::conditional_t<kMasked, RowRegsMasked<T>, RowRegs<T>>;
    auto fetch = [&](int y) -> Regs {
        const char* const xr = reinterpret_cast<const char*>(X + (size_t)y * W * xs);
        const char* const yr = reinterpret_cast<const char*>(Y + (size_t)y * W * 3);
        Regs r;
        r.xm = *reinterpret_cast<const float*>(xr + xa_o); r.ym = *reinterpret_cast<const T*>(yr + ya_o);
        r.xe = *reinterpret_cast<const float*>(xr + xb_o); r.ye = *reinterpret_cast<const T*>(yr + yb_o);
        if constexpr (kMasked) {                               // the same clamped columns
            const uint8_t* const mr = M + (size_t)y * W;
            r.mm = mr[(unsigned)xa_c]; r.me = mr[(unsigned)xb_c];
        }
        return r;
    };

    const int total = rows + kHalo;                            // pixel rows o0 .. o0 + total - 1 (all < H)
    // rows are fetched kBatch at a time into registers with static indices: the row loop is unrolled by kRing = 12, one
    // batch being filtered and one in flight (train.hip has the measurements behind this shape)
    constexpr int kBatch = 6, kRing = kWin + 1;
    static_assert(kRing == 2 * kBatch, "two batches per unrolled body");
    Regs rb[2 * kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) rb[i] = fetch(o0 + min(i, total - 1));
    float ring[5][kRing];
    float ssim_sum = 0.0f;                                     // (in double it costs the register that spills at three waves per SIMD)
    double se_sum = 0.0, ae_sum = 0.0;
    float (*mring)[kLine] = nullptr;                           // masked: this wave's last kRing rows of weights
    float mc_sum = 0.0f;                                       // (a lane's centre weights: at most 64 values <= 1, as its SSIM terms)
    double mp_sum = 0.0;
    if constexpr (kMasked) {
        __shared__ float mask_lines[kWaves][kRing][kLine];
        mring = mask_lines[c];
    }
    for (int base = 0; base < total; base += kRing) {
#pragma unroll
        for (int s = 0; s < kRing; ++s) {
            const int t = base + s;
            if (t >= total) continue;                          // wave-uniform (no break: the unrolled body keeps static ring indices)
            const Regs cur = rb[s];
            float xm = in_a ? cur.xm : 0.0f, ym = in_a ? value(cur.ym) : 0.0f;
            float xe = in_b ? cur.xe : 0.0f, ye = in_b ? value(cur.ye) : 0.0f;
            if constexpr (kMasked) {
                const float wm = in_a ? lut[cur.mm] : 0.0f, we = in_b ? lut[cur.me] : 0.0f;
                if (t < rows || last_seg) {                    // the errors of the image itself, weighed
                    const float dm = xm - ym, de = last_block ? xe - ye : 0.0f;
                    const double wmd = (double)wm, wed = last_block ? (double)we : 0.0;
                    ae_sum += wmd * (double)fabsf(dm) + wed * (double)fabsf(de);
                    se_sum = __builtin_fma(wed * (double)de, (double)de, __builtin_fma(wmd * (double)dm, (double)dm, se_sum));
                    if (c == 0) mp_sum += wmd + wed;
                }
                mring[s][lane] = wm;
                if (lane < 16) mring[s][kCols + lane] = we;
                // the SSIM reads the substituted image (columns outside the image stay zero)
                xm = in_a ? ts_mask_blend_value(xm, ym, cur.mm, wm) : 0.0f;
                xe = in_b ? ts_mask_blend_value(xe, ye, cur.me, we) : 0.0f;
            } else if (t < rows || last_seg) {
                const float dm = xm - ym, de = last_block ? xe - ye : 0.0f;
                ae_sum += (double)fabsf(dm) + (double)fabsf(de);
                se_sum = __builtin_fma((double)de, (double)de, __builtin_fma((double)dm, (double)dm, se_sum));
            }
            float* lx = line[c][t & 1][0];
            float* ly = line[c][t & 1][1];
            lx[lane] = xm; ly[lane] = ym;
            if (lane < 16) { lx[kCols + lane] = xe; ly[kCols + lane] = ye; }
            if (s % kBatch == 0 && t + kBatch < total) {       // the batch after this one, into the other half of rb
#pragma unroll
                for (int i = 0; i < kBatch; ++i) rb[(s + kBatch + i) % kRing] = fetch(o0 + min(t + kBatch + i, total - 1));
            }
            TS_METRICS_WAVE_SYNC();
            float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float a = lx[lane + k], b = ly[lane + k];
                const float wa = g[k] * a, wb = g[k] * b;
                h0 += wa; h1 += wb;
                h2 = __builtin_fmaf(wa, a, h2); h3 = __builtin_fmaf(wb, b, h3); h4 = __builtin_fmaf(wa, b, h4);
            }
            ring[0][s] = h0; ring[1][s] = h1; ring[2][s] = h2; ring[3][s] = h3; ring[4][s] = h4;
            if (t >= kHalo) {
                // map row t - 10 of this wave: the pixel rows t - 10 .. t sit in ring slots (s + 2 + k) % 12
                float f[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    float v = 0.f;
#pragma unroll
                    for (int k = 0; k < kWin; ++k) v = __builtin_fmaf(g[k], ring[m][(s + 2 + k) % kRing], v);
                    f[m] = v;
                }
                if constexpr (kMasked) {
                    if (xa < Wo) {                             // centre pixel: row t - 5 (ring slot (s + 7) % 12), column xa + 5
                        const float mc = mring[(s + kRing - kCentre) % kRing][lane + kCentre];
                        ssim_sum += mc * ts_metrics_ssim_term(f[0], f[1], f[2], f[3], f[4]);
                        if (c == 0) mc_sum += mc;
                    }
                } else {
                    if (xa < Wo) ssim_sum += ts_metrics_ssim_term(f[0], f[1], f[2], f[3], f[4]);
                }
            }
        }
    }
    const double ts = wave_sum((double)ssim_sum), te = wave_sum(se_sum), ta = wave_sum(ae_sum);
    if constexpr (kMasked) {
        const double tp = wave_sum(mp_sum), tc = wave_sum((double)mc_sum);
        if (lane == 0) {
            double* const o = partials + TS_METRICS_MASKED_PARTIALS * slot;
            o[0] = ts; o[1] = te; o[2] = ta; o[3] = tp; o[4] = tc;
        }
    } else if (lane == 0) {
        partials[TS_METRICS_PARTIALS * slot] = ts;
        partials[TS_METRICS_PARTIALS * slot + 1] = te;
        partials[TS_METRICS_PARTIALS * slot + 2] = ta;
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves, 3) void image_metrics_rows_kernel(int H, int W, int xs, int seg,
                                                                          const float* __restrict__ X,
                                                                          const T* __restrict__ Y,
                                                                          double* __restrict__ partials) {
    image_metrics_rows_body<T, false>(H, W, xs, seg, X, Y, nullptr, partials);
}

// (two waves per SIMD: at three the mask bytes in flight spill 136 bytes per lane)
template <typename T>
__global__ __launch_bounds__(64 * kWaves, 2) void image_metrics_rows_masked_kernel(int H, int W, int xs, int seg,
                                                                                 const float* __restrict__ X,
                                                                                 const T* __restrict__ Y,
                                                                                 const uint8_t* __restrict__ M,
                                                                                 double* __restrict__ partials) {
    image_metrics_rows_body<T, true>(H, W, xs, seg, X, Y, M, partials);
}

// {mse, l1, ssim, psnr} from the waves' partial sums: thread i adds the waves i, i + 256, ... in that order, then a
// binary tree over the 256 threads - the same additions in the same order on every run and every device
// kPartials: the doubles per wave, TS_METRICS_PARTIALS or, masked, TS_METRICS_MASKED_PARTIALS - then the means run over
// the weights' sums in slots 3 and 4 (three channels each) instead of the element counts; sums of zero give NaN
template <int kPartials>
__device__ __forceinline__ void image_metrics_reduce_body(int H, int W, int waves,
                                                          const double* __restrict__ partials,
                                                          double* __restrict__ out) {
    __shared__ double part[kPartials][kReduceThreads];
    double acc[kPartials] = {};
    for (int i = threadIdx.x; i < waves; i += kReduceThreads)
        for (int k = 0; k < kPartials; ++k) acc[k] += partials[(size_t)kPartials * i + k];
    for (int k = 0; k < kPartials; ++k) part[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int step = kReduceThreads / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int k = 0; k < kPartials; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double n_map = 3.0 * (double)(H - kHalo) * (double)(W - kHalo), n_img = 3.0 * (double)H * (double)W;
        if constexpr (kPartials == TS_METRICS_MASKED_PARTIALS) { n_img = 3.0 * part[3][0]; n_map = 3.0 * part[4][0]; }
        const double mse = part[1][0] / n_img;
        out[0] = mse;
        out[1] = part[2][0] / n_img;
        out[2] = part[0][0] / n_map;
        out[3] = ts_metrics_psnr(mse);
    }
}

__global__ __launch_bounds__(kReduceThreads) void image_metrics_reduce_kernel(int H, int W, int waves,
                                                                              const double* __restrict__ partials,
                                                                              double* __restrict__ out) {
    image_metrics_reduce_body<TS_METRICS_PARTIALS>(H, W, waves, partials, out);
}

__global__ __launch_bounds__(kReduceThreads) void image_metrics_masked_reduce_kernel(int H, int W, int waves,
                                                                                     const double* __restrict__ partials,
                                                                                     double* __restrict__ out) {
    image_metrics_reduce_body<TS_METRICS_MASKED_PARTIALS>(H, W, waves, partials, out);
}

}  // namespace

extern "C" {

int64_t ts_image_metrics_ws_bytes(int32_t height, int32_t width) {
    return ts_metrics_waves(height, width) * TS_METRICS_PARTIALS * (int64_t)sizeof(double);
}

int ts_image_metrics(int32_t height, int32_t width, int32_t pixel_floats, const float* image, const void* target,
                     int32_t target_is_u8, void* ws, double* out4, void* stream) {
    if (height <= kHalo || width <= kHalo) return TS_E_BADARG;
    if (pixel_floats != 3 && pixel_floats != 4) return TS_E_BADARG;
    if (!image || !target || !ws || !out4) return TS_E_BADARG;
    if ((uintptr_t)ws % sizeof(double) || (uintptr_t)out4 % sizeof(double) || (uintptr_t)image % sizeof(float)) return TS_E_BADARG;
    if (!target_is_u8 && (uintptr_t)target % sizeof(float)) return TS_E_BADARG;
    if ((int64_t)width * 16 > INT32_MAX) return TS_E_BADARG;  // a lane's byte offset inside a row is 32 bits
    const int64_t waves = ts_metrics_waves(height, width);
    if (waves > INT32_MAX) return TS_E_BADARG;
    const int ho = height - kHalo, wo = width - kHalo;
    const int seg = ts_metrics_segment_rows(ho, wo);
    const dim3 grid((wo + kCols - 1) / kCols, (ho + seg - 1) / seg);
    if (grid.y > 65535u) return TS_E_BADARG;                  // (more than four million rows)
    hipStream_t s = (hipStream_t)stream;
    if (target_is_u8)
        hipLaunchKernelGGL(image_metrics_rows_kernel<uint8_t>, grid, dim3(64 * kWaves), 0, s, (int)height, (int)width,
                           (int)pixel_floats, seg, image, (const uint8_t*)target, (double*)ws);
    else
        hipLaunchKernelGGL(image_metrics_rows_kernel<float>, grid, dim3(64 * kWaves), 0, s, (int)height, (int)width,
                           (int)pixel_floats, seg, image, (const float*)target, (double*)ws);
    hipLaunchKernelGGL(image_metrics_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, s, (int)height, (int)width,
                       (int)waves, (const double*)ws, out4);
    return launch_status();
}

int64_t ts_image_metrics_masked_ws_bytes(int32_t height, int32_t width) {
    return ts_metrics_waves(height, width) * TS_METRICS_MASKED_PARTIALS * (int64_t)sizeof(double);
}

int ts_image_metrics_masked(int32_t height, int32_t width, int32_t pixel_floats, const float* image, const void* target,
                            int32_t target_is_u8, const uint8_t* mask, void* ws, double* out4, void* stream) {
    if (height <= kHalo || width <= kHalo) return TS_E_BADARG;
    if (pixel_floats != 3 && pixel_floats != 4) return TS_E_BADARG;
    if (!image || !target || !mask || !ws || !out4) return TS_E_BADARG;
    if ((uintptr_t)ws % sizeof(double) || (uintptr_t)out4 % sizeof(double) || (uintptr_t)image % sizeof(float)) return TS_E_BADARG;
    if (!target_is_u8 && (uintptr_t)target % sizeof(float)) return TS_E_BADARG;
    if ((int64_t)width * 16 > INT32_MAX) return TS_E_BADARG;  // a lane's byte offset inside a row is 32 bits
    const int64_t waves = ts_metrics_waves(height, width);
    if (waves > INT32_MAX) return TS_E_BADARG;
    const int ho = height - kHalo, wo = width - kHalo;
    const int seg = ts_metrics_segment_rows(ho, wo);
    const dim3 grid((wo + kCols - 1) / kCols, (ho + seg - 1) / seg);
    if (grid.y > 65535u) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (target_is_u8)
        hipLaunchKernelGGL(image_metrics_rows_masked_kernel<uint8_t>, grid, dim3(64 * kWaves), 0, s, (int)height,
                           (int)width, (int)pixel_floats, seg, image, (const uint8_t*)target, mask, (double*)ws);
    else
        hipLaunchKernelGGL(image_metrics_rows_masked_kernel<float>, grid, dim3(64 * kWaves), 0, s, (int)height,
                           (int)width, (int)pixel_floats, seg, image, (const float*)target, mask, (double*)ws);
    hipLaunchKernelGGL(image_metrics_masked_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, s, (int)height, (int)width,
                       (int)waves, (const double*)ws, out4);
    return launch_status();
}

}  // extern "C"
