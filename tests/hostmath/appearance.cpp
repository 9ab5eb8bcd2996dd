// Host build of csrc/appearance_math.h for tests/test_appearance_cpu.py and tests/test_gpu_appearance.py: the per-pixel
// forward and backward of the bilateral-grid colour model in plain sequential loops, and the total variation and the
// affine fit's sums with the partition and the summation order of csrc/appearance.hip (thread t takes the elements
// t, t + 1024, ...; a binary tree over the threads; a wave's 64 lanes are summed by the xor butterfly), so that the device
// results can be compared bit for bit.  Compiled with -ffp-contract=off, as the kernels are.
#include "../../tinysplat_amd/csrc/appearance_math.h"

#include <vector>

namespace {

void pixel_levels(int h, int w, int L, int Gh, int Gw, const float* grid, int x, int y, float r, float g, float b,
                  TsAppLevel* z, float* A0, float* A1) {
    const TsAppAxis ax = ts_app_axis(x, w, Gw), ay = ts_app_axis(y, h, Gh);
    *z = ts_app_level(ts_app_gray(r, g, b), L);
    ts_app_level_matrix(grid, Gh, Gw, z->l0, ax, ay, A0);
    ts_app_level_matrix(grid, Gh, Gw, z->l1, ax, ay, A1);
}

double tree(std::vector<double>& part) {               // appearance.hip: tree_sum
    for (int step = TS_APP_REDUCE_THREADS / 2; step >= 1; step >>= 1)
        for (int t = 0; t < step; ++t) part[t] += part[t + step];
    return part[0];
}

double butterfly(double* lanes) {                      // appearance.hip: wave_sum
    for (int d = 32; d >= 1; d >>= 1) {
        double next[64];
        for (int i = 0; i < 64; ++i) next[i] = lanes[i] + lanes[i ^ d];
        for (int i = 0; i < 64; ++i) lanes[i] = next[i];
    }
    return lanes[0];
}

}  // namespace

extern "C" {

void ah_axis(int p, int P, int G, int* i0, int* i1, float* t) {
    const TsAppAxis a = ts_app_axis(p, P, G);
    *i0 = a.i0; *i1 = a.i1; *t = a.t;
}

void ah_level(float r, float g, float b, int L, int* l0, int* l1, float* t, int* inside) {
    const TsAppLevel z = ts_app_level(ts_app_gray(r, g, b), L);
    *l0 = z.l0; *l1 = z.l1; *t = z.t; *inside = z.inside;
}

int64_t ah_ws_bytes(int h, int w, int L, int Gh, int Gw) {
    return ts_app_tiles(h, w) * ts_app_slab_doubles(h, w, L, Gh, Gw) * (int64_t)sizeof(double);
}

void ah_fwd(int h, int w, int L, int Gh, int Gw, const float* image, const float* grid, float* out) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t at = ((size_t)y * w + x) * 3;
            TsAppLevel z;
            float A0[TS_APP_ENTRIES], A1[TS_APP_ENTRIES];
            pixel_levels(h, w, L, Gh, Gw, grid, x, y, image[at], image[at + 1], image[at + 2], &z, A0, A1);
            ts_app_pixel_fwd(A0, A1, z.t, image[at], image[at + 1], image[at + 2], out + at);
        }
}

// v_grid: the pixels added in row-major order in double, rounded once (the device adds them in another fixed order)
void ah_bwd(int h, int w, int L, int Gh, int Gw, const float* image, const float* grid, const float* v_out, float* v_image,
            float* v_grid) {
    std::vector<double> acc((size_t)L * Gh * Gw * TS_APP_ENTRIES, 0.0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t at = ((size_t)y * w + x) * 3;
            const float r = image[at], g = image[at + 1], b = image[at + 2];
            TsAppLevel z;
            float A0[TS_APP_ENTRIES], A1[TS_APP_ENTRIES], vA[TS_APP_ENTRIES];
            pixel_levels(h, w, L, Gh, Gw, grid, x, y, r, g, b, &z, A0, A1);
            ts_app_pixel_bwd(A0, A1, z, L, r, g, b, v_out + at, vA, v_image + at);
            const TsAppAxis ax = ts_app_axis(x, w, Gw), ay = ts_app_axis(y, h, Gh);
            for (int l = z.l0; l <= z.l1; ++l)
                for (int j = ay.i0; j <= ay.i1; ++j)
                    for (int i = ax.i0; i <= ax.i1; ++i) {
                        const double f = (double)ts_app_hat(l, z.l0, z.l1, z.t) * (double)ts_app_hat(j, ay.i0, ay.i1, ay.t) *
                                         (double)ts_app_hat(i, ax.i0, ax.i1, ax.t);
                        double* dst = acc.data() + ts_app_vertex(Gh, Gw, l, j, i);
                        for (int c = 0; c < TS_APP_ENTRIES; ++c) dst[c] += f * (double)vA[c];
                    }
        }
    for (size_t e = 0; e < acc.size(); ++e) v_grid[e] = (float)acc[e];
}

void ah_tv(int L, int Gh, int Gw, const float* grid, float weight, const float* v_in, double* value, float* v_out) {
    const int T = TS_APP_REDUCE_THREADS;
    double n[3];
    ts_app_tv_counts(L, Gh, Gw, n);
    const int total = L * Gh * Gw * TS_APP_ENTRIES;
    std::vector<double> part[3] = {std::vector<double>(T), std::vector<double>(T), std::vector<double>(T)};
    for (int t = 0; t < T; ++t) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int e = t; e < total; e += T) {
            const float g = (float)ts_app_tv_element(grid, L, Gh, Gw, e, n, acc);
            v_out[e] = (v_in ? v_in[e] : 0.0f) + weight * g;
        }
        for (int a = 0; a < 3; ++a) part[a][t] = acc[a];
    }
    const double sums[3] = {tree(part[0]), tree(part[1]), tree(part[2])};
    value[0] = ts_app_tv_value(sums, n);
}

void ah_fit_sums(int h, int w, const float* image, const void* target, int target_is_u8, double* out22) {
    const int T = TS_APP_REDUCE_THREADS;
    const int64_t N = (int64_t)h * w, waves = ts_app_fit_waves(N);
    std::vector<double> partials((size_t)waves * TS_APP_FIT_SUMS);
    for (int64_t wave = 0; wave < waves; ++wave) {
        const int64_t first = wave * 64 * TS_APP_FIT_LANE_PIXELS;
        std::vector<double> lanes((size_t)64 * TS_APP_FIT_SUMS, 0.0);         // [lane][sum]
        for (int lane = 0; lane < 64; ++lane)
            for (int m = 0; m < TS_APP_FIT_LANE_PIXELS; ++m) {
                const int64_t p = first + lane + 64 * (int64_t)m;
                if (p >= N) break;
                float t[3];
                for (int c = 0; c < 3; ++c)
                    t[c] = target_is_u8 ? ts_app_byte_to_float(((const uint8_t*)target)[3 * p + c])
                                        : ((const float*)target)[3 * p + c];
                ts_app_fit_pixel(image[3 * p], image[3 * p + 1], image[3 * p + 2], t[0], t[1], t[2],
                                 lanes.data() + (size_t)lane * TS_APP_FIT_SUMS);
            }
        for (int s = 0; s < TS_APP_FIT_SUMS; ++s) {
            double column[64];
            for (int lane = 0; lane < 64; ++lane) column[lane] = lanes[(size_t)lane * TS_APP_FIT_SUMS + s];
            partials[(size_t)wave * TS_APP_FIT_SUMS + s] = butterfly(column);
        }
    }
    for (int s = 0; s < TS_APP_FIT_SUMS; ++s) {
        std::vector<double> part(T, 0.0);
        for (int t = 0; t < T; ++t)
            for (int64_t i = t; i < waves; i += T) part[t] += partials[(size_t)i * TS_APP_FIT_SUMS + s];
        out22[s] = tree(part);
    }
}

}  // extern "C"
