// mesh.hip - sparse-grid iso-surface mesh of the SuGaR density: marching tetrahedra over the
// bricks (8^3 cells) that a Gaussian's box reaches, on top of ts_knn and ts_extract_pack's records.
//
//   boxes     one thread per Gaussian: mean -+ extent * sqrt(Sigma_aa) per world axis, Sigma = R diag(exp(2 s)) R^T in
//             double (quat_rotation of density_field.h: the R the records are packed from), rounded outwards.  A point
//             outside the box has Mahalanobis q > extent^2 to that Gaussian ((e_a . x)^2 <= Sigma_aa x^T Sigma^-1 x),
//             so outside every box d <= 16 exp(-extent^2 / 2).
//   mark      one thread per Gaussian: the flag of every brick holding a cell with a corner inside the box.  The corner
//             range is found on the float32 corner positions themselves (ts_mesh_corner_pos), starting two corners
//             wide and narrowing: never too small.  Plain byte stores of 1: idempotent, no atomics.
//   corners   one thread per corner of a listed brick (9^3 each): its position.  A corner beyond the grid's last cell
//             takes the position of the last corner of its axis: a finite query next to real ones, d = 0 regardless.
//   density   one thread per corner: the 16-neighbour density (density_at of density_field.h).
//   count     one workgroup per brick, one thread per cell: the brick's 729 densities in LDS, the cell's triangle count
//   emit      (mesh_cells.h), an exclusive prefix over the workgroup (ballots of the count's four bits inside a wave,
//             LDS across the eight waves); count stores the brick total, emit the triangles at offsets[brick] + prefix:
//             three edge keys and three interpolated positions each, in (brick, cell, tetrahedron, triangle) order.
//   observed  count and emit over a field with NaN corners (section 6p, tsdf.hip): a cell with one emits nothing.
// Plain stores only: every output is a fixed function of the inputs.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "density_field.h"
#include "host_util.h"
#include "mesh_cells.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBrick = TS_MESH_BRICK;
constexpr int kCorners = TS_MESH_BRICK_CORNERS;
constexpr int kCells = TS_MESH_BRICK_CELLS;
constexpr int64_t kMaxBricks = (int64_t)INT32_MAX / ((int64_t)kCorners * kK);   // corners * 16 stays below 2^31

struct Grid {
    float lo[3];
    float h;
    int32_t n[3];       // cells per axis
};

__device__ __forceinline__ void brick_coords(const Grid& g, int64_t brick, int32_t b[3]) {
    const int64_t nbx = (g.n[0] + kBrick - 1) / kBrick, nby = (g.n[1] + kBrick - 1) / kBrick;
    b[0] = (int32_t)(brick % nbx);
    b[1] = (int32_t)((brick / nbx) % nby);
    b[2] = (int32_t)(brick / (nbx * nby));
}

__global__ __launch_bounds__(kThreads) void boxes_kernel(int n, float extent, const float* __restrict__ means,
                                                         const float* __restrict__ scales,
                                                         const float* __restrict__ quats, float* __restrict__ boxes) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double R[3][3];
    quat_rotation(quats[i * 4], quats[i * 4 + 1], quats[i * 4 + 2], quats[i * 4 + 3], R);
    double var[3];
    for (int c = 0; c < 3; ++c) var[c] = exp(2.0 * (double)scales[i * 3 + c]);
    for (int a = 0; a < 3; ++a) {
        const double saa = (R[a][0] * R[a][0] * var[0] + R[a][1] * R[a][1] * var[1]) + R[a][2] * R[a][2] * var[2];
        const double half = (double)extent * sqrt(saa);
        const double m = (double)means[i * 3 + a];
        // rounded to float32 and moved one step outwards: the float32 box contains the exact one
        boxes[i * 6 + a] = nextafterf((float)(m - half), -INFINITY);
        boxes[i * 6 + 3 + a] = nextafterf((float)(m + half), INFINITY);
    }
}

__global__ __launch_bounds__(kThreads) void mark_kernel(int n, Grid g, const float* __restrict__ boxes,
                                                        uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int32_t b0[3], b1[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = boxes[i * 6 + a], hi = boxes[i * 6 + 3 + a];
        const int32_t last = g.n[a];                    // corners 0..n
        int32_t c0 = 0, c1 = last;
        if (lo == lo && hi == hi) {                     // a box that is not a number reaches everywhere
            if (lo > hi) return;
            // two corners wide of the double estimate, clamped while still a double, then narrowed on the float32
            // corner positions: the range ends up exact, or too wide by what the four steps could not take back
            const double x0 = floor(((double)lo - (double)g.lo[a]) / (double)g.h) - 2.0;
            const double x1 = ceil(((double)hi - (double)g.lo[a]) / (double)g.h) + 2.0;
            if (x0 > (double)last || x1 < 0.0) return;  // wholly outside on this axis
            c0 = (int32_t)fmax(x0, 0.0);
            c1 = (int32_t)fmin(x1, (double)last);
            for (int s = 0; s < 4 && c0 <= last && ts_mesh_corner_pos(g.lo[a], g.h, c0) < lo; ++s) ++c0;
            for (int s = 0; s < 4 && c1 >= 0 && ts_mesh_corner_pos(g.lo[a], g.h, c1) > hi; ++s) --c1;
            if (c0 > c1) return;                        // no corner inside: nothing to mark
        }
        // the cells with a corner in c0..c1, clipped to the grid, and their bricks
        const int32_t cell0 = c0 > 0 ? c0 - 1 : 0, cell1 = c1 < last - 1 ? c1 : last - 1;
        b0[a] = cell0 / kBrick;
        b1[a] = cell1 / kBrick;
    }
    const int64_t nbx = (g.n[0] + kBrick - 1) / kBrick, nby = (g.n[1] + kBrick - 1) / kBrick;
    for (int32_t bz = b0[2]; bz <= b1[2]; ++bz)
        for (int32_t by = b0[1]; by <= b1[1]; ++by)
            for (int32_t bx = b0[0]; bx <= b1[0]; ++bx) flags[((int64_t)bz * nby + by) * nbx + bx] = 1;
}

__global__ __launch_bounds__(kThreads) void corners_kernel(int64_t total, Grid g, const int64_t* __restrict__ bricks,
                                                           float* __restrict__ corners) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t b = e / kCorners;
    const int l = (int)(e - b * kCorners);
    int32_t bc[3];
    brick_coords(g, bricks[b], bc);
    const int li[3] = {l % 9, (l / 9) % 9, l / 81};
    for (int a = 0; a < 3; ++a) {
        int32_t i = bc[a] * kBrick + li[a];
        if (i > g.n[a]) i = g.n[a];
        corners[e * 3 + a] = ts_mesh_corner_pos(g.lo[a], g.h, i);
    }
}

__global__ __launch_bounds__(kThreads) void density_kernel(int n, int64_t total, Grid g,
                                                           const int64_t* __restrict__ bricks,
                                                           const float* __restrict__ corners,
                                                           const int32_t* __restrict__ knn,
                                                           const float* __restrict__ records,
                                                           float* __restrict__ density) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t b = e / kCorners;
    const int l = (int)(e - b * kCorners);
    int32_t bc[3];
    brick_coords(g, bricks[b], bc);
    const bool inside = bc[0] * kBrick + l % 9 <= g.n[0] && bc[1] * kBrick + (l / 9) % 9 <= g.n[1] &&
                        bc[2] * kBrick + l / 81 <= g.n[2];
    float d = 0.f;
    if (inside) {
        const float p[3] = {corners[e * 3], corners[e * 3 + 1], corners[e * 3 + 2]};
        d = density_at(n, p, knn + e * kK, records);
    }
    density[e] = d;
}

// kObserved (section 6p): the field may hold NaN (a corner nothing observed), and a cell with such a corner emits nothing
template <bool kEmit, bool kObserved = false>
__global__ __launch_bounds__(kCells) void cells_kernel(Grid g, float level, const int64_t* __restrict__ bricks,
                                                       const float* __restrict__ density, int32_t* __restrict__ counts,
                                                       const int64_t* __restrict__ offsets, int64_t* __restrict__ keys,
                                                       float* __restrict__ positions, int64_t* __restrict__ cells) {
    __shared__ float sd[kCorners];
    __shared__ int wave_total[kCells / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = tid; i < kCorners; i += kCells) sd[i] = density[b * kCorners + i];
    __syncthreads();
    int32_t bc[3];
    brick_coords(g, bricks[b], bc);
    const int l[3] = {tid & 7, (tid >> 3) & 7, tid >> 6};
    const int32_t c[3] = {bc[0] * kBrick + l[0], bc[1] * kBrick + l[1], bc[2] * kBrick + l[2]};
    const bool inside = c[0] < g.n[0] && c[1] < g.n[1] && c[2] < g.n[2];
    auto corner_d = [&](int k) { return sd[(l[2] + (k >> 2)) * 81 + (l[1] + ((k >> 1) & 1)) * 9 + l[0] + (k & 1)]; };
    unsigned above = 0;
    if (inside) {
#pragma unroll
        for (int k = 0; k < 8; ++k) above |= (corner_d(k) > level ? 1u : 0u) << k;
        if (kObserved) {
            bool unseen = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) unseen = unseen || corner_d(k) != corner_d(k);
            if (unseen) above = 0u;
        }
    }
    const int cnt = (above != 0u && above != 255u) ? ts_mesh_cell_count(above) : 0;        // 0..12: four bits
    // exclusive prefix of cnt over the workgroup, in thread order
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int prefix = 0, total = 0;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) {
        const unsigned long long bal = __ballot((cnt >> bit) & 1);
        prefix += __popcll(bal & below) << bit;
        total += __popcll(bal) << bit;
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    int base = 0, brick_total = 0;
#pragma unroll
    for (int w = 0; w < kCells / 64; ++w) {
        const int t = wave_total[w];
        if (w < wave) base += t;
        brick_total += t;
    }
    if (!kEmit) {
        if (tid == 0) counts[b] = brick_total;
        return;
    }
    if (cnt == 0) return;
    int64_t at = offsets[b] + base + prefix;
    const int64_t sx = (int64_t)g.n[0] + 1, sy = (int64_t)g.n[1] + 1;
    const int64_t id0 = ((int64_t)c[2] * sy + c[1]) * sx + c[0];
    const int64_t cell = ((int64_t)c[2] * g.n[1] + c[1]) * g.n[0] + c[0];
    for (int t = 0; t < 6; ++t) {
        uint8_t ends[6];
        const int m = ts_mesh_tet(t, above, ends);
        for (int j = 0; j < m; ++j, ++at) {
            for (int k = 0; k < 3; ++k) {
                const int a = ends[3 * j + k] & 7, z = ends[3 * j + k] >> 3;
                const int64_t id = id0 + (a & 1) + ((a >> 1) & 1) * sx + (a >> 2) * sx * sy;
                float pa[3], pz[3], out[3];
                for (int x = 0; x < 3; ++x) {
                    pa[x] = ts_mesh_corner_pos(g.lo[x], g.h, c[x] + ((a >> x) & 1));
                    pz[x] = ts_mesh_corner_pos(g.lo[x], g.h, c[x] + ((z >> x) & 1));
                }
                ts_mesh_interp(level, corner_d(a), corner_d(z), pa, pz, out);
                keys[at * 3 + k] = id * 8 + (a ^ z);
                for (int x = 0; x < 3; ++x) positions[(at * 3 + k) * 3 + x] = out[x];
            }
            if (cells) cells[at] = cell;
        }
    }
}

// host float[4] {lo, h} and int32[3] cells per axis -> Grid; false for anything a kernel must not see
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
    if (ids >= 9.2e18) return false;                    // corner id * 8 + direction must fit int64
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = grid_host[a];
        g->n[a] = cells_host[a];
    }
    g->h = grid_host[3];
    return true;
}

inline bool bricks_ok(int32_t bricks) { return bricks >= 1 && bricks <= kMaxBricks; }

}  // namespace

extern "C" {

int ts_mesh_boxes(int32_t n, const float* means, const float* scales, const float* quats, float extent_sigmas,
                  float* boxes, void* stream) {
    if (n < 1 || !means || !scales || !quats || !boxes) return TS_E_BADARG;
    if (!(extent_sigmas > 0.f) || !isfinite(extent_sigmas)) return TS_E_BADARG;
    hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, extent_sigmas, means, scales, quats, boxes);
    return launch_status();
}

int ts_mesh_mark(int32_t n, const float* boxes, const float* grid_host, const int32_t* cells_host, uint8_t* flags,
                 void* stream) {
    Grid g;
    if (n < 1 || !boxes || !flags || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    hipLaunchKernelGGL(mark_kernel, dim3((unsigned)nblocks(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, g, boxes, flags);
    return launch_status();
}

int64_t ts_mesh_chunk_bytes(int32_t n, int32_t bricks) {
    if (n < TS_EXTRACT_K || !bricks_ok(bricks)) return TS_E_BADARG;
    const int64_t q = (int64_t)bricks * kCorners;
    const int64_t knn_ws = ts_knn_ws_bytes(n, (int32_t)q, TS_EXTRACT_K);
    if (knn_ws < 0) return TS_E_BADARG;
    // corners | k-NN distances, indices | densities | per brick: count (int32), offset (int64), k-NN stats (int32[2])
    return knn_ws + align256(q * 12) + 2 * align256(q * TS_EXTRACT_K * 4) + align256(q * 4) +
           align256((int64_t)bricks * 4) + 2 * align256((int64_t)bricks * 8);
}

int ts_mesh_corners(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                    float* corners, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !brick_ids || !corners || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    const int64_t total = (int64_t)bricks * kCorners;
    hipLaunchKernelGGL(corners_kernel, dim3((unsigned)nblocks(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       total, g, brick_ids, corners);
    return launch_status();
}

int ts_mesh_density(int32_t n, int32_t bricks, const int64_t* brick_ids, const float* grid_host,
                    const int32_t* cells_host, const float* corners, const int32_t* knn, const float* records,
                    float* density, void* stream) {
    Grid g;
    if (n < TS_EXTRACT_K || !bricks_ok(bricks) || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!brick_ids || !corners || !knn || !records || !density) return TS_E_BADARG;
    const int64_t total = (int64_t)bricks * kCorners;
    hipLaunchKernelGGL(density_kernel, dim3((unsigned)nblocks(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (int)n, total, g, brick_ids, corners, knn, records, density);
    return launch_status();
}

int ts_mesh_count(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                  float level, const float* density, int32_t* counts, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !isfinite(level) || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!brick_ids || !density || !counts) return TS_E_BADARG;
    hipLaunchKernelGGL(cells_kernel<false>, dim3((unsigned)bricks), dim3(kCells), 0, (hipStream_t)stream, g, level,
                       brick_ids, density, counts, (const int64_t*)nullptr, (int64_t*)nullptr, (float*)nullptr,
                       (int64_t*)nullptr);
    return launch_status();
}

int ts_mesh_emit(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                 float level, const float* density, const int64_t* offsets, int64_t* keys, float* positions,
                 int64_t* cells, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !isfinite(level) || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!brick_ids || !density || !offsets || !keys || !positions) return TS_E_BADARG;
    hipLaunchKernelGGL(cells_kernel<true>, dim3((unsigned)bricks), dim3(kCells), 0, (hipStream_t)stream, g, level,
                       brick_ids, density, (int32_t*)nullptr, offsets, keys, positions, cells);
    return launch_status();
}

int ts_mesh_count_observed(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                           float level, const float* field, int32_t* counts, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !isfinite(level) || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!brick_ids || !field || !counts) return TS_E_BADARG;
    hipLaunchKernelGGL((cells_kernel<false, true>), dim3((unsigned)bricks), dim3(kCells), 0, (hipStream_t)stream, g, level,
                       brick_ids, field, counts, (const int64_t*)nullptr, (int64_t*)nullptr, (float*)nullptr,
                       (int64_t*)nullptr);
    return launch_status();
}

int ts_mesh_emit_observed(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                          float level, const float* field, const int64_t* offsets, int64_t* keys, float* positions,
                          int64_t* cells, void* stream) {
    Grid g;
    if (!bricks_ok(bricks) || !isfinite(level) || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!brick_ids || !field || !offsets || !keys || !positions) return TS_E_BADARG;
    hipLaunchKernelGGL((cells_kernel<true, true>), dim3((unsigned)bricks), dim3(kCells), 0, (hipStream_t)stream, g, level,
                       brick_ids, field, (int32_t*)nullptr, offsets, keys, positions, cells);
    return launch_status();
}

}  // extern "C"
