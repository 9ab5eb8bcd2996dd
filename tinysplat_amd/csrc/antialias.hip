// antialias.hip - opacity compensation for the 2D low-pass (the arithmetic: antialias_math.h).
//
// Three streaming launches, one lane per Gaussian, no atomics and no LDS; a result depends on its own row alone, so the
// bytes are the same on every run and equal the host build of antialias_math.h (tests/hostmath/antialias.cpp).
//   ts_antialias_fwd      44 bytes read (means, scales 12 each, quats 16, opacity 4), 20 to 24 written: comp and / or o_eff
//                         and the 16-byte record (a_o, b, c_o, comp) the backward launch reads instead of projecting again
//   ts_antialias_bwd      40 bytes read (radii, record, opacity, v_opacity, v_conic), 16 written in place
//   ts_compensation_bwd   the stand-alone op: projects again and runs project_one_vjp on the compensation's gradient alone
// Quaternions and records move as 16 bytes a lane.  The [n, 3] rows (means, scales, v_conic, v_means, v_scales) do NOT: a
// lane reads and writes its row as three 4-byte accesses, as project.hip does - a deliberate choice, not the 16-byte
// form.  A wave's footprint is still one contiguous 768-byte span and every fetched line is used whole, and 16-byte
// accesses to 12-byte rows would need pose.hip's staging of the block through LDS, which the measurements do not ask for:
// the backward launch runs at 0.93 of the streaming rate and the forward launch is bound by its arithmetic.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "antialias_math.h"

static_assert(ts::kAaLogScales == TS_PROJECT_LOG_SCALES && ts::kAaRawQuats == TS_PROJECT_RAW_QUATS &&
                  ts::kAaLogitOpacity == TS_RASTER_LOGIT_OPACITY,
              "antialias_math.h restates the flag bits of tinysplat_hip.h");

namespace {

constexpr int kThreads = 256;

// the projection's camera block without proj @ view, which nothing here reads for a result (zeros)
__device__ __forceinline__ ts::Cam load_view_cam(const float* __restrict__ viewmat, const ts_camera c) {
    ts::Cam C;
#pragma unroll
    for (int i = 0; i < 12; ++i) C.v[i] = viewmat[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) C.p[i] = 0.0f;
    C.fx = c.fx; C.fy = c.fy; C.cx = c.cx; C.cy = c.cy;
    C.W = c.img_width; C.H = c.img_height; C.tbx = c.tile_bounds_x; C.tby = c.tile_bounds_y;
    C.row0 = c.tile_row0; C.rows = c.tile_rows; C.gs = c.glob_scale; C.clip = c.clip_thresh;
    return C;
}

__global__ __launch_bounds__(kThreads) void antialias_fwd_kernel(
    int n, const float* __restrict__ means3d, const float* __restrict__ scales, const float* __restrict__ quats,
    const float* __restrict__ viewmat, const ts_camera cam, const int project_flags,
    const float* __restrict__ opacity, const int raster_flags, float* __restrict__ comp, float* __restrict__ o_eff,
    float4* __restrict__ rows) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const ts::Cam C = load_view_cam(viewmat, cam);
    const float m[3] = {means3d[3 * i], means3d[3 * i + 1], means3d[3 * i + 2]};
    float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float4 qv = reinterpret_cast<const float4*>(quats)[i];
    float q[4] = {qv.x, qv.y, qv.z, qv.w};
    const float op = o_eff ? opacity[i] : 0.0f;
    const ts::AaRow r = ts::aa_forward_row(C, project_flags, m, s, q);
    if (rows) rows[i] = make_float4(r.ao, r.b, r.co, r.comp);
    if (comp) comp[i] = r.comp;
    if (o_eff) o_eff[i] = ts::aa_opacity(raster_flags, op) * r.comp;
}

__global__ __launch_bounds__(kThreads) void antialias_bwd_kernel(
    int n, const int* __restrict__ radii, const float4* __restrict__ rows, const float* __restrict__ opacity,
    const int raster_flags, float* __restrict__ v_opacity, float* __restrict__ v_conic) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (radii[i] <= 0) return;               // culled: the zeros ts_reduce_partials wrote stay
    const float4 rv = rows[i];
    const ts::AaRow r{rv.x, rv.y, rv.z, rv.w};
    float v_op, G[3];
    ts::aa_backward_row(r, raster_flags, opacity[i], v_opacity[i], v_op, G);
    v_opacity[i] = v_op;
    v_conic[3 * i] = v_conic[3 * i] + G[0];
    v_conic[3 * i + 1] = v_conic[3 * i + 1] + G[1];
    v_conic[3 * i + 2] = v_conic[3 * i + 2] + G[2];
}

__global__ __launch_bounds__(kThreads) void compensation_bwd_kernel(
    int n, const float* __restrict__ means3d, const float* __restrict__ scales, const float* __restrict__ quats,
    const float* __restrict__ viewmat, const ts_camera cam, const int project_flags,
    const float* __restrict__ v_comp, float* __restrict__ v_means3d, float* __restrict__ v_scales,
    float* __restrict__ v_quats) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const ts::Cam C = load_view_cam(viewmat, cam);
    const float m[3] = {means3d[3 * i], means3d[3 * i + 1], means3d[3 * i + 2]};
    float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float4 qv = reinterpret_cast<const float4*>(quats)[i];
    float q[4] = {qv.x, qv.y, qv.z, qv.w};
    ts::ProjGrad g;
    ts::aa_comp_backward_row(C, project_flags, m, s, q, v_comp[i], g);
    v_means3d[3 * i] = g.v_mean[0]; v_means3d[3 * i + 1] = g.v_mean[1]; v_means3d[3 * i + 2] = g.v_mean[2];
    v_scales[3 * i] = g.v_scale[0]; v_scales[3 * i + 1] = g.v_scale[1]; v_scales[3 * i + 2] = g.v_scale[2];
    reinterpret_cast<float4*>(v_quats)[i] = make_float4(g.v_quat[0], g.v_quat[1], g.v_quat[2], g.v_quat[3]);
}

inline bool misaligned(const void* p, uintptr_t to) { return p && ((uintptr_t)p % to) != 0; }

}  // namespace

extern "C" {

int ts_antialias_fwd(int32_t n, const float* means3d, const float* scales, const float* quats, const float* viewmat,
                     const ts_camera* cam, int32_t project_flags, const float* opacity, int32_t raster_flags, float* comp,
                     float* o_eff, float* rows, void* stream) {
    if (n < 0 || !cam || (project_flags & ~3) || (raster_flags & ~TS_RASTER_LOGIT_OPACITY)) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!means3d || !scales || !quats || !viewmat || (!comp && !o_eff && !rows) || (o_eff && !opacity)) return TS_E_BADARG;
    if (misaligned(quats, 16) || misaligned(rows, 16) || misaligned(means3d, 4) || misaligned(scales, 4) ||
        misaligned(opacity, 4) || misaligned(comp, 4) || misaligned(o_eff, 4))
        return TS_E_BADARG;
    hipLaunchKernelGGL(antialias_fwd_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, means3d, scales, quats, viewmat, *cam, (int)project_flags, opacity, (int)raster_flags, comp,
                       o_eff, reinterpret_cast<float4*>(rows));
    return launch_status();
}

int ts_antialias_bwd(int32_t n, const int32_t* radii, const float* rows, const float* opacity, int32_t raster_flags,
                     float* v_opacity, float* v_conic, void* stream) {
    if (n < 0 || (raster_flags & ~TS_RASTER_LOGIT_OPACITY)) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!radii || !rows || !opacity || !v_opacity || !v_conic) return TS_E_BADARG;
    if (misaligned(rows, 16) || misaligned(radii, 4) || misaligned(opacity, 4) || misaligned(v_opacity, 4) ||
        misaligned(v_conic, 4))
        return TS_E_BADARG;
    hipLaunchKernelGGL(antialias_bwd_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, radii, reinterpret_cast<const float4*>(rows), opacity, (int)raster_flags, v_opacity, v_conic);
    return launch_status();
}

int ts_compensation_bwd(int32_t n, const float* means3d, const float* scales, const float* quats, const float* viewmat,
                        const ts_camera* cam, int32_t project_flags, const float* v_comp, float* v_means3d,
                        float* v_scales, float* v_quats, void* stream) {
    if (n < 0 || !cam || (project_flags & ~3)) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!means3d || !scales || !quats || !viewmat || !v_comp || !v_means3d || !v_scales || !v_quats) return TS_E_BADARG;
    if (misaligned(quats, 16) || misaligned(v_quats, 16) || misaligned(means3d, 4) || misaligned(scales, 4) ||
        misaligned(v_comp, 4) || misaligned(v_means3d, 4) || misaligned(v_scales, 4))
        return TS_E_BADARG;
    hipLaunchKernelGGL(compensation_bwd_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (int)n, means3d, scales, quats, viewmat, *cam, (int)project_flags, v_comp,
                       v_means3d, v_scales, v_quats);
    return launch_status();
}

}  // extern "C"
