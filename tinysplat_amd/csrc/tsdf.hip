// tsdf.hip - truncated signed distance fusion of depth maps on the mesher's brick grid: the field
// that ts_mesh_count_observed / ts_mesh_emit_observed (mesh.hip) mesh at level 0.
//
//   mark       one thread per (pixel, camera): a pixel with a depth d <= depth_max flags every brick that touches the box
//              of its frustum piece - the four rays through (px +- 0.5, py +- 0.5) at the view depths d and d + trunc,
//              unprojected in double (tsdf_math.h) - widened by one cell edge and rounded outwards to float32.  Plain byte
//              stores of 1: idempotent, no atomics.
//   integrate  one workgroup of 256 threads per brick; a thread owns the corners tid, tid + 256, tid + 512 of the brick's
//              729 (x fastest: neighbouring lanes read neighbouring pixels) and keeps their double sums and counts in
//              registers over the cameras [c0, c1), in list order.  The camera index is the same in every lane, so the
//              table is read through uniform addresses; a camera whose frustum the brick's bounding sphere misses
//              (ts_tsdf_cull) is skipped by the whole workgroup before any corner is projected: 64 cameras are tested at
//              a time, one per lane, and the ballot is the list the workgroup walks.  No atomics: a corner belongs to
//              one thread.
//   field      one thread per corner: F = -(float)(sum / count), NaN below min_observations.
// Plain stores only: every output is a fixed function of the inputs.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "mesh_cells.h"
#include "tsdf_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBrick = TS_MESH_BRICK;
constexpr int kCorners = TS_MESH_BRICK_CORNERS;
constexpr int kOwned = (kCorners + kThreads - 1) / kThreads;        // 3
constexpr int64_t kMaxBricks = (int64_t)INT32_MAX / kCorners;       // corners stay below 2^31

struct Grid {
    float lo[3];
    float h;
    int32_t n[3];       // cells per axis
};

__global__ __launch_bounds__(kThreads) void mark_kernel(Grid g, const ts_tsdf_camera* __restrict__ cameras, float trunc,
                                                        float depth_max, uint8_t* __restrict__ flags) {
    const ts_tsdf_camera& cam = cameras[blockIdx.y];
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= (int64_t)cam.width * cam.height) return;
    const float d = cam.depth[f];
    if (!ts_tsdf_valid_depth(d) || d > depth_max) return;
    const int32_t px = (int32_t)(f % cam.width), py = (int32_t)(f / cam.width);
    const int32_t nb[3] = {(g.n[0] + kBrick - 1) / kBrick, (g.n[1] + kBrick - 1) / kBrick,
                           (g.n[2] + kBrick - 1) / kBrick};
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool whole = false;                                 // a ray that cannot be unprojected reaches everywhere
    for (int k = 0; k < 8 && !whole; ++k) {
        const double u = (double)px + ((k & 1) ? 0.5 : -0.5), v = (double)py + ((k & 2) ? 0.5 : -0.5);
        const double z = (k & 4) ? (double)d + (double)trunc : (double)d;
        double x[3];
        if (!ts_tsdf_unproject(cam, u, v, z, x)) {
            whole = true;
            break;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], x[a]);
            hi[a] = fmax(hi[a], x[a]);
        }
    }
    int32_t b0[3], b1[3];
    for (int a = 0; a < 3; ++a) {
        b0[a] = 0;
        b1[a] = nb[a] - 1;
        if (whole) continue;
        // widened by one cell edge and a sixteenth (section 6p: the float32 rounding of the pair's own arithmetic),
        // rounded to float32 and moved one step outwards
        const double wide = (double)g.h * 1.0625;
        const float flo = nextafterf((float)(lo[a] - wide), -INFINITY), fhi = nextafterf((float)(hi[a] + wide), INFINITY);
        const double edge = (double)g.h * kBrick;
        const double x0 = floor(((double)flo - (double)g.lo[a]) / edge), x1 = floor(((double)fhi - (double)g.lo[a]) / edge);
        if (x1 < 0.0 || x0 > (double)(nb[a] - 1)) return;           // wholly outside on this axis
        b0[a] = (int32_t)fmax(x0, 0.0);
        b1[a] = (int32_t)fmin(x1, (double)(nb[a] - 1));
    }
    for (int32_t bz = b0[2]; bz <= b1[2]; ++bz)
        for (int32_t by = b0[1]; by <= b1[1]; ++by)
            for (int32_t bx = b0[0]; bx <= b1[0]; ++bx) flags[((int64_t)bz * nb[1] + by) * nb[0] + bx] = 1;
}

__global__ __launch_bounds__(kThreads) void integrate_kernel(Grid g, const int64_t* __restrict__ bricks,
                                                             const ts_tsdf_camera* __restrict__ cameras, int32_t c0,
                                                             int32_t c1, float trunc, float znear, float depth_max,
                                                             int cull, double* __restrict__ sum,
                                                             int32_t* __restrict__ count) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t brick = bricks[b];
    const int64_t nbx = (g.n[0] + kBrick - 1) / kBrick, nby = (g.n[1] + kBrick - 1) / kBrick;
    const int32_t bc[3] = {(int32_t)(brick % nbx), (int32_t)((brick / nbx) % nby), (int32_t)(brick / (nbx * nby))};
    // the sphere around the brick's corners that lie inside the grid: centre and half diagonal from the float32 corner
    // positions, the radius a sixteenth of a cell larger than the double half diagonal
    float centre[3];
    double r2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const int32_t i0 = bc[a] * kBrick, i1 = i0 + kBrick < g.n[a] ? i0 + kBrick : g.n[a];
        const float p0 = ts_mesh_corner_pos(g.lo[a], g.h, i0), p1 = ts_mesh_corner_pos(g.lo[a], g.h, i1);
        centre[a] = 0.5f * (p0 + p1);
        const double half = fmax((double)p1 - (double)centre[a], (double)centre[a] - (double)p0);
        r2 += half * half;
    }
    const float radius = (float)(sqrt(r2) + 0.0625 * (double)g.h) * 1.000001f;
    float x[kOwned][3];
    bool live[kOwned];
    double acc[kOwned];
    int32_t cnt[kOwned];
#pragma unroll
    for (int j = 0; j < kOwned; ++j) {
        const int l = tid + j * kThreads;
        const int li[3] = {l % 9, (l / 9) % 9, l / 81};
        live[j] = l < kCorners;
        for (int a = 0; a < 3; ++a) {
            const int32_t i = bc[a] * kBrick + li[a];
            live[j] = live[j] && i <= g.n[a];                       // a corner beyond the last cell observes nothing
            x[j][a] = ts_mesh_corner_pos(g.lo[a], g.h, i < g.n[a] ? i : g.n[a]);
        }
        acc[j] = (l < kCorners) ? sum[b * kCorners + l] : 0.0;
        cnt[j] = (l < kCorners) ? count[b * kCorners + l] : 0;
    }
    // 64 cameras at a time: lane i tests the brick against camera base + i, and the ballot is the list of cameras the
    // whole workgroup then walks in ascending order (every wave computes the same mask from the same inputs)
    const int lane = tid & 63;
    for (int32_t base = c0; base < c1; base += 64) {
        const int32_t mine = base + lane;
        const bool keep = mine < c1 && !(cull && ts_tsdf_cull(cameras[mine], centre, radius, znear));
        unsigned long long todo = __ballot(keep);
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const ts_tsdf_camera& cam = cameras[base + i];                       // a uniform address
#pragma unroll
            for (int j = 0; j < kOwned; ++j) {
                if (!live[j]) continue;
                float z, t;
                const int64_t pixel = ts_tsdf_pixel(cam, x[j], znear, &z);
                if (pixel < 0) continue;
                if (!ts_tsdf_observe(cam.depth[pixel], z, trunc, depth_max, &t)) continue;
                acc[j] += (double)t;
                cnt[j] += 1;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kOwned; ++j) {
        const int l = tid + j * kThreads;
        if (l < kCorners) {
            sum[b * kCorners + l] = acc[j];
            count[b * kCorners + l] = cnt[j];
        }
    }
}

__global__ __launch_bounds__(kThreads) void field_kernel(int64_t total, const double* __restrict__ sum,
                                                         const int32_t* __restrict__ count, int32_t min_observations,
                                                         float* __restrict__ field) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int32_t n = count[e];
    field[e] = n >= min_observations ? -(float)(sum[e] / (double)n) : __builtin_nanf("");
}

bool read_grid(const float* grid_host, const int32_t* cells_host, Grid* g) {
    if (!grid_host || !cells_host) return false;
    for (int c = 0; c < 4; ++c)
        if (!isfinite(grid_host[c])) return false;
    if (!(grid_host[3] > 0.f)) return false;
    double ids = 8.0;
    for (int a = 0; a < 3; ++a) {
        if (cells_host[a] < 1 || cells_host[a] == INT32_MAX) return false;
        ids *= (double)cells_host[a] + 1.0;
    }
    if (ids >= 9.2e18) return false;                    // as mesh.hip: corner id * 8 + direction must fit int64
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = grid_host[a];
        g->n[a] = cells_host[a];
    }
    g->h = grid_host[3];
    return true;
}

inline bool bricks_ok(int32_t bricks) { return bricks >= 1 && bricks <= kMaxBricks; }
inline bool positive_finite(float v) { return v > 0.f && isfinite(v); }

}  // namespace

extern "C" {

int32_t ts_tsdf_camera_bytes(void) { return (int32_t)sizeof(ts_tsdf_camera); }

int ts_tsdf_mark(int32_t cameras, const void* camera_table, int64_t max_pixels, const float* grid_host,
                 const int32_t* cells_host, float trunc, float depth_max, uint8_t* flags, void* stream) {
    Grid g;
    if (cameras < 1 || cameras > 65535 || !camera_table || !flags || !read_grid(grid_host, cells_host, &g))
        return TS_E_BADARG;
    if (max_pixels < 1 || max_pixels > (int64_t)INT32_MAX || !positive_finite(trunc) || !(depth_max > 0.f))
        return TS_E_BADARG;
    hipLaunchKernelGGL(mark_kernel, dim3((unsigned)nblocks(max_pixels, kThreads), (unsigned)cameras), dim3(kThreads), 0,
                       (hipStream_t)stream, g, (const ts_tsdf_camera*)camera_table, trunc, depth_max, flags);
    return launch_status();
}

int64_t ts_tsdf_chunk_bytes(int32_t bricks) {
    if (!bricks_ok(bricks)) return TS_E_BADARG;
    const int64_t q = (int64_t)bricks * kCorners;
    // sums (double) | counts (int32) | field (float32) | per brick: triangle count (int32), offset (int64)
    return align256(q * 8) + 2 * align256(q * 4) + align256((int64_t)bricks * 4) + align256((int64_t)bricks * 8);
}

int ts_tsdf_integrate(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                      const void* camera_table, int32_t c0, int32_t c1, float trunc, float znear, float depth_max,
                      int32_t flags, double* sum, int32_t* count, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !brick_ids || !camera_table || !sum || !count || !read_grid(grid_host, cells_host, &g))
        return TS_E_BADARG;
    if (c0 < 0 || c1 < c0 || !positive_finite(trunc) || !isfinite(znear) || !(depth_max > 0.f)) return TS_E_BADARG;
    if ((flags & ~TS_TSDF_NO_CULL) != 0 || ((uintptr_t)sum & 7) != 0) return TS_E_BADARG;
    if (c1 == c0) return 0;
    hipLaunchKernelGGL(integrate_kernel, dim3((unsigned)bricks), dim3(kThreads), 0, (hipStream_t)stream, g, brick_ids,
                       (const ts_tsdf_camera*)camera_table, c0, c1, trunc, znear, depth_max,
                       (flags & TS_TSDF_NO_CULL) ? 0 : 1, sum, count);
    return launch_status();
}

int ts_tsdf_field(int32_t bricks, const double* sum, const int32_t* count, int32_t min_observations, float* field,
                  void* stream) {
    if (!bricks_ok(bricks) || !sum || !count || !field || min_observations < 1) return TS_E_BADARG;
    const int64_t total = (int64_t)bricks * kCorners;
    hipLaunchKernelGGL(field_kernel, dim3((unsigned)nblocks(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       total, sum, count, min_observations, field);
    return launch_status();
}

}  // extern "C"
