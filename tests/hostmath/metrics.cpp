// Host build of csrc/metrics_math.h for tests/test_metrics_cpu.py: the byte conversion, the SSIM term and the PSNR formula
// that the kernels of csrc/metrics.hip call, behind a C interface, around a plain sequential float32 filter with the
// window of csrc/gauss_window.h (compiled with -ffp-contract=off, as the kernels are) and double sums.
#include "../../tinysplat_amd/csrc/gauss_window.h"
#include "../../tinysplat_amd/csrc/metrics_math.h"

#include <vector>

extern "C" {

float mh_byte_to_float(int b) { return ts_metrics_byte_to_float((uint8_t)b); }
float mh_ssim_term(float m1, float m2, float q1, float q2, float r12) { return ts_metrics_ssim_term(m1, m2, q1, q2, r12); }
double mh_psnr(double mse) { return ts_metrics_psnr(mse); }
int64_t mh_waves(int height, int width) { return ts_metrics_waves(height, width); }
int mh_segment_rows(int ho, int wo) { return ts_metrics_segment_rows(ho, wo); }

// image: float32 [height, width, pixel_floats]; target: [height, width, 3], float32 or uint8 -> out4 {mse, l1, ssim, psnr}
int mh_image_metrics(int height, int width, int pixel_floats, const float* image, const void* target, int target_is_u8,
                     double* out4) {
    if (height <= TS_METRICS_HALO || width <= TS_METRICS_HALO || (pixel_floats != 3 && pixel_floats != 4)) return -1;
    const float g[TS_METRICS_WIN] = {TS_GAUSS_WINDOW};
    const int ho = height - TS_METRICS_HALO, wo = width - TS_METRICS_HALO;
    auto x_at = [&](int y, int x, int c) { return image[((size_t)y * width + x) * pixel_floats + c]; };
    auto y_at = [&](int y, int x, int c) {
        const size_t i = ((size_t)y * width + x) * 3 + c;
        return target_is_u8 ? ts_metrics_byte_to_float(((const uint8_t*)target)[i]) : ((const float*)target)[i];
    };
    double se = 0.0, ae = 0.0, ss = 0.0;
    std::vector<float> rows((size_t)5 * height * wo);          // the five maps after the horizontal pass
    for (int c = 0; c < 3; ++c) {
        for (int y = 0; y < height; ++y) {
            for (int x = 0; x < width; ++x) {
                const float d = x_at(y, x, c) - y_at(y, x, c);
                se += (double)d * (double)d;
                ae += (double)fabsf(d);
            }
            for (int x = 0; x < wo; ++x) {
                float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < TS_METRICS_WIN; ++k) {
                    const float a = x_at(y, x + k, c), b = y_at(y, x + k, c);
                    h[0] += g[k] * a; h[1] += g[k] * b;
                    h[2] += g[k] * a * a; h[3] += g[k] * b * b; h[4] += g[k] * a * b;
                }
                for (int m = 0; m < 5; ++m) rows[((size_t)m * height + y) * wo + x] = h[m];
            }
        }
        for (int y = 0; y < ho; ++y)
            for (int x = 0; x < wo; ++x) {
                float f[5];
                for (int m = 0; m < 5; ++m) {
                    float v = 0.f;
                    for (int k = 0; k < TS_METRICS_WIN; ++k) v += g[k] * rows[((size_t)m * height + y + k) * wo + x];
                    f[m] = v;
                }
                ss += (double)ts_metrics_ssim_term(f[0], f[1], f[2], f[3], f[4]);
            }
    }
    const double n_img = 3.0 * height * width, n_map = 3.0 * ho * wo;
    out4[0] = se / n_img;
    out4[1] = ae / n_img;
    out4[2] = ss / n_map;
    out4[3] = ts_metrics_psnr(out4[0]);
    return 0;
}

}  // extern "C"
