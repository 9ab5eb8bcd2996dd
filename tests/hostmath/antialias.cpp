// Host build of csrc/antialias_math.h for tests/test_antialias_cpu.py and tests/test_gpu_antialias.py: the per-Gaussian
// functions the kernels of csrc/antialias.hip call, behind a C interface (compiled with -ffp-contract=off, as the kernels
// are).
#include "../../tinysplat_amd/csrc/antialias_math.h"

#include <stdint.h>

namespace {

// cam10: fx, fy, cx, cy, width, height, tile bounds x, tile bounds y, glob_scale, clip_thresh
ts::Cam make_cam(const float* view34, const float* cam10) {
    ts::Cam C;
    for (int i = 0; i < 12; ++i) C.v[i] = view34[i];
    for (int i = 0; i < 16; ++i) C.p[i] = 0.0f;
    C.fx = cam10[0]; C.fy = cam10[1]; C.cx = cam10[2]; C.cy = cam10[3];
    C.W = (int)cam10[4]; C.H = (int)cam10[5]; C.tbx = (int)cam10[6]; C.tby = (int)cam10[7];
    C.row0 = 0; C.rows = C.tby; C.gs = cam10[8]; C.clip = cam10[9];
    return C;
}

}  // namespace

extern "C" {

// comp[n] and G[n, 3] of n triples (a_o, b, c_o) with upstream gradients v[n]
void ah_triples(int64_t n, const float* triples, const float* v, float* comp, float* G) {
    for (int64_t i = 0; i < n; ++i) {
        comp[i] = ts::compensation(triples[3 * i], triples[3 * i + 1], triples[3 * i + 2]);
        ts::compensation_vjp(triples[3 * i], triples[3 * i + 1], triples[3 * i + 2], v[i], G + 3 * i);
    }
}

void ah_exp(int64_t n, const float* x, float* y, float* sig) {
    for (int64_t i = 0; i < n; ++i) { y[i] = ts::aa_exp(x[i]); sig[i] = ts::aa_sigmoid(x[i]); }
}

// ts_antialias_fwd with every pointer on the host; comp, o_eff, rows all written (opacity may be null: o_eff untouched)
void ah_fwd(int64_t n, const float* means, const float* scales, const float* quats, const float* view34,
            const float* cam10, int project_flags, const float* opacity, int raster_flags, float* comp, float* o_eff,
            float* rows) {
    const ts::Cam C = make_cam(view34, cam10);
    for (int64_t i = 0; i < n; ++i) {
        float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        float q[4] = {quats[4 * i], quats[4 * i + 1], quats[4 * i + 2], quats[4 * i + 3]};
        const ts::AaRow r = ts::aa_forward_row(C, project_flags, means + 3 * i, s, q);
        rows[4 * i] = r.ao; rows[4 * i + 1] = r.b; rows[4 * i + 2] = r.co; rows[4 * i + 3] = r.comp;
        comp[i] = r.comp;
        if (opacity) o_eff[i] = ts::aa_opacity(raster_flags, opacity[i]) * r.comp;
    }
}

// ts_antialias_bwd with every pointer on the host: v_opacity and v_conic updated in place where radii > 0
void ah_bwd(int64_t n, const int32_t* radii, const float* rows, const float* opacity, int raster_flags, float* v_opacity,
            float* v_conic) {
    for (int64_t i = 0; i < n; ++i) {
        if (radii[i] <= 0) continue;
        const ts::AaRow r{rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]};
        float v_op, G[3];
        ts::aa_backward_row(r, raster_flags, opacity[i], v_opacity[i], v_op, G);
        v_opacity[i] = v_op;
        for (int k = 0; k < 3; ++k) v_conic[3 * i + k] = v_conic[3 * i + k] + G[k];
    }
}

// ts_compensation_bwd with every pointer on the host
void ah_comp_bwd(int64_t n, const float* means, const float* scales, const float* quats, const float* view34,
                 const float* cam10, int project_flags, const float* v_comp, float* v_means, float* v_scales,
                 float* v_quats) {
    const ts::Cam C = make_cam(view34, cam10);
    for (int64_t i = 0; i < n; ++i) {
        float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        float q[4] = {quats[4 * i], quats[4 * i + 1], quats[4 * i + 2], quats[4 * i + 3]};
        ts::ProjGrad g;
        ts::aa_comp_backward_row(C, project_flags, means + 3 * i, s, q, v_comp[i], g);
        for (int k = 0; k < 3; ++k) { v_means[3 * i + k] = g.v_mean[k]; v_scales[3 * i + k] = g.v_scale[k]; }
        for (int k = 0; k < 4; ++k) v_quats[4 * i + k] = g.v_quat[k];
    }
}

}  // extern "C"
