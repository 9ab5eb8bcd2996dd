// Host build of csrc/transform_math.h for tests/test_transform_cpu.py and tests/test_gpu_transform.py: the functions the
// kernels of csrc/transform.hip call, behind a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/transform_math.h"

namespace {

template <int BANDS>
void rows(int64_t n, const ts_xf_params& p, const uint8_t* mask, const float* means, const float* scales,
          const float* quats, const float* rest, float* means_out, float* scales_out, float* quats_out, float* rest_out) {
    constexpr int R = 3 * BANDS * (BANDS + 2);
    for (int64_t g = 0; g < n; ++g) {
        float m[3], s[3], q[4], row[R > 0 ? R : 1];
        for (int k = 0; k < 3; ++k) m[k] = means[3 * g + k];
        for (int k = 0; k < 3; ++k) s[k] = scales[3 * g + k];
        for (int k = 0; k < 4; ++k) q[k] = quats[4 * g + k];
        for (int k = 0; k < R; ++k) row[k] = rest[R * g + k];
        if (!mask || mask[g]) {
            ts_xf_mean(p.m, p.t, m, m);
            ts_xf_scale(p.log_scale, s, s);
            ts_xf_quat(p.r, q, q);
            ts_xf_sh_row<BANDS>(p.sh, row);
        }
        for (int k = 0; k < 3; ++k) means_out[3 * g + k] = m[k];
        for (int k = 0; k < 3; ++k) scales_out[3 * g + k] = s[k];
        for (int k = 0; k < 4; ++k) quats_out[4 * g + k] = q[k];
        for (int k = 0; k < R; ++k) rest_out[R * g + k] = row[k];
    }
}

}  // namespace

extern "C" {

// the arguments of ts_transform_gaussians with every pointer on the host; -1 for a k_rest that is none of 0 3 8 15 24
int xh_transform(int64_t n, int k_rest, const float* xform, const float* quat, float log_scale, const float* sh,
                 const uint8_t* mask, const float* means, const float* scales, const float* quats, const float* rest,
                 float* means_out, float* scales_out, float* quats_out, float* rest_out) {
    const int bands = ts_xf_bands(k_rest);
    if (bands < 0) return -1;
    ts_xf_params p = {};
    for (int i = 0; i < 9; ++i) p.m[i] = xform[i];
    for (int i = 0; i < 3; ++i) p.t[i] = xform[9 + i];
    for (int i = 0; i < 4; ++i) p.r[i] = quat[i];
    p.log_scale = log_scale;
    const int sh_floats = bands > 0 ? ts_xf_sh_offset(bands) + (2 * bands + 1) * (2 * bands + 1) : 0;
    for (int i = 0; i < sh_floats; ++i) p.sh[i] = sh[i];
    switch (bands) {
        case 0: rows<0>(n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out); break;
        case 1: rows<1>(n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out); break;
        case 2: rows<2>(n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out); break;
        case 3: rows<3>(n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out); break;
        default: rows<4>(n, p, mask, means, scales, quats, rest, means_out, scales_out, quats_out, rest_out); break;
    }
    return 0;
}

// box [12]: A then b; means [n,3] -> inside [n]
void xh_box_mask(int64_t n, const float* box, const float* means, uint8_t* inside) {
    for (int64_t i = 0; i < n; ++i) inside[i] = ts_xf_inside(box, box + 9, means + 3 * i) ? 1 : 0;
}

}  // extern "C"
