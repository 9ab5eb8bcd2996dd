// Host-side checker of tinysplat_amd/csrc/splat_math.h.  TEST INFRASTRUCTURE: compiles the very
// same per-Gaussian math header the HIP kernels use with g++ (no FMA contraction), so the CPU test
// suite can compare it with the oracle without a GPU.  Never loaded by the product.
#include "../../tinysplat_amd/csrc/splat_math.h"

extern "C" {

struct hm_camera {
    float fx, fy, cx, cy;
    int W, H, tbx, tby, row0, rows;
    float gs, clip;
};

static ts::Cam make_cam(const float* viewmat, const float* projmat, const hm_camera* c) {
    ts::Cam C;
    for (int i = 0; i < 12; ++i) C.v[i] = viewmat[i];
    for (int i = 0; i < 16; ++i) C.p[i] = projmat[i];
    C.fx = c->fx; C.fy = c->fy; C.cx = c->cx; C.cy = c->cy;
    C.W = c->W; C.H = c->H; C.tbx = c->tbx; C.tby = c->tby; C.row0 = c->row0; C.rows = c->rows;
    C.gs = c->gs; C.clip = c->clip;
    return C;
}

void hm_project_fwd(int n, const float* means, const float* scales, const float* quats,
                    const float* viewmat, const float* projmat, const hm_camera* cam, float* xys,
                    float* depths, int* radii, float* conics, int* nth, float* cov3d) {
    const ts::Cam C = make_cam(viewmat, projmat, cam);
    for (int i = 0; i < n; ++i) {
        ts::ProjOut o;
        ts::project_one(C, means + 3 * i, scales + 3 * i, quats + 4 * i, o);
        xys[2 * i] = o.x; xys[2 * i + 1] = o.y; depths[i] = o.depth; radii[i] = o.radius;
        for (int k = 0; k < 3; ++k) conics[3 * i + k] = o.conic[k];
        nth[i] = o.tiles;
        for (int k = 0; k < 6; ++k) cov3d[6 * i + k] = o.cov3d[k];
    }
}

void hm_project_bwd(int n, const float* means, const float* scales, const float* quats,
                    const float* viewmat, const float* projmat, const hm_camera* cam,
                    const int* radii, const float* v_xy, const float* v_depth, const float* v_conic,
                    const float* v_cov3d, float* v_means, float* v_scales, float* v_quats) {
    const ts::Cam C = make_cam(viewmat, projmat, cam);
    for (int i = 0; i < n; ++i) {
        ts::ProjGrad g;
        for (int k = 0; k < 3; ++k) { g.v_mean[k] = 0; g.v_scale[k] = 0; }
        for (int k = 0; k < 4; ++k) g.v_quat[k] = 0;
        if (radii[i] > 0)
            ts::project_one_vjp(C, means + 3 * i, scales + 3 * i, quats + 4 * i, v_xy + 2 * i,
                                v_depth[i], v_conic + 3 * i, v_cov3d ? v_cov3d + 6 * i : nullptr, g);
        for (int k = 0; k < 3; ++k) { v_means[3 * i + k] = g.v_mean[k]; v_scales[3 * i + k] = g.v_scale[k]; }
        for (int k = 0; k < 4; ++k) v_quats[4 * i + k] = g.v_quat[k];
    }
}

void hm_sh_basis(int n, int degree, const float* dirs, float* Y) {
    const int nb = ts::sh_num_bases(degree);
    for (int i = 0; i < n; ++i)
        ts::sh_basis(degree, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], Y + (size_t)nb * i);
}

void hm_tile_bbox(int n, const float* xys, const float* radii, int tbx, int tby, int row0, int rows,
                  int* out4) {
    for (int i = 0; i < n; ++i) {
        const ts::TileBox b = ts::tile_bbox(xys[2 * i], xys[2 * i + 1], radii[i], tbx, tby, row0, rows);
        out4[4 * i] = b.minx; out4[4 * i + 1] = b.miny; out4[4 * i + 2] = b.maxx; out4[4 * i + 3] = b.maxy;
    }
}

// ---- the two alpha culls, with exactly the operands the kernels hand them ------------------------------------------
// records: 6 floats per case, the packed record's words x, y, opacity, conic.xx, conic.xy, conic.yy.

// raster.hip: stage_splat for ONE block rectangle per case.  rects: {x0, x1, y0, y1} inclusive sample positions.
// out[i]: 1 = the block is kept, 0 = rejected (the opacity gate of stage_splat included: op <= 0, tau < -0.02).
// The gate is a hand-written MIRROR of stage_splat's (op > 0, tau >= -0.02, geometric cull only for hA, hC > 0): a change
// there must be repeated here.  tests/test_gpu_cull.py composites the same cases on the device, which binds the two.
void hm_rect_may_contribute(int n, const float* records, const float* rects, int* out) {
    for (int i = 0; i < n; ++i) {
        const float* q = records + 6 * i;
        const float* r = rects + 4 * i;
        const float gx = q[0], gy = q[1], op = q[2];
        const float hA = 0.5f * ts::kLog2e * q[3], B = ts::kLog2e * q[4], hC = 0.5f * ts::kLog2e * q[5];
        out[i] = 0;
        if (!(op > 0.0f)) continue;
        const float tau = ts::fast_log2(op) + ts::kLog2_255;
        if (!(tau >= -0.02f)) continue;
        if (hA > 0.0f && hC > 0.0f)
            out[i] = ts::rect_may_contribute(hA, B, hC, 0.5f / hA, 0.5f / hC, tau, gx, gy, r[0], r[1], r[2], r[3]) ? 1 : 0;
        else
            out[i] = 1;                                   // not a PSD conic: no geometric cull
    }
}

// forms: hA, B, hC (log2 domain, hA, hC > 0); rects: xlo, xhi, ylo, yhi (offsets centre - sample)
void hm_min_form_on_rect(int n, const float* forms, const float* rects, float* out) {
    for (int i = 0; i < n; ++i) {
        const float* f = forms + 3 * i;
        const float* r = rects + 4 * i;
        out[i] = ts::min_form_on_rect(f[0], f[1], f[2], 0.5f / f[0], 0.5f / f[2], r[0], r[1], r[2], r[3]);
    }
}

// binning.hip: walk_chunk for one Gaussian per case.  boxes: minx, miny, maxx, maxy of ts::tile_bbox; rows of the box
// are written to lo / hi at row_off[i] + (ty - miny): the kept tiles of tile row ty are [lo, hi) (hi <= lo: none;
// cull_all: every row empty).
void hm_tight_rows(int n, const float* records, const int* radii, const int* boxes, const int64_t* row_off,
                   int* lo, int* hi) {
    for (int i = 0; i < n; ++i) {
        const float* q = records + 6 * i;
        const int* b = boxes + 4 * i;
        const ts::TightTest t(true, q[0], q[1], q[2], q[3], q[4], q[5], (float)radii[i]);
        for (int ty = b[1]; ty < b[3]; ++ty) {
            const int64_t k = row_off[i] + (ty - b[1]);
            if (t.cull_all) { lo[k] = b[0]; hi[k] = b[0]; continue; }
            t.row_range(ty, b[0], b[2], lo[k], hi[k]);
        }
    }
}

}  // extern "C"
