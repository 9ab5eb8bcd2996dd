// The mesher's per-cell routine (tinysplat_amd/csrc/mesh_cells.h) compiled for the host, for tests/test_mesh_cpu.py.
#include <stdint.h>

#include "../../tinysplat_amd/csrc/mesh_cells.h"

extern "C" {

// One cell: d[8], id[8] -> the number of triangles; keys[n][3], lo[n][3], hi[n][3] (room for 12 triangles each).
int mc_cell(const float* d, float level, const int64_t* id, int64_t* keys, int32_t* lo, int32_t* hi) {
    return ts_mesh_cell(d, level, id, reinterpret_cast<int64_t(*)[3]>(keys), reinterpret_cast<int32_t(*)[3]>(lo),
                        reinterpret_cast<int32_t(*)[3]>(hi));
}

int mc_cell_count(unsigned above8) { return ts_mesh_cell_count(above8); }

float mc_corner_pos(float lo, float h, int32_t i) { return ts_mesh_corner_pos(lo, h, i); }

// A block of nx * ny * nz cells over the corner field d[(k (ny + 1) + j)(nx + 1) + i], corners at lo + (i, j, k) * h:
// triangles in (cell, tetrahedron, triangle) order, cells x fastest -> their number; keys[t][3], positions[t][3][3]
// and cells[t] are written up to `room` triangles (the count goes on).
int64_t mc_block(int32_t nx, int32_t ny, int32_t nz, const float* d, float level, const float* lo, float h,
                 int64_t room, int64_t* keys, float* positions, int64_t* cells) {
    const int64_t sx = (int64_t)nx + 1, sy = (int64_t)ny + 1;
    int64_t t = 0;
    for (int32_t k = 0; k < nz; ++k)
        for (int32_t j = 0; j < ny; ++j)
            for (int32_t i = 0; i < nx; ++i) {
                float dc[8];
                int64_t id[8];
                const int32_t c[3] = {i, j, k};
                for (int q = 0; q < 8; ++q) {
                    id[q] = ((int64_t)(k + (q >> 2)) * sy + (j + ((q >> 1) & 1))) * sx + (i + (q & 1));
                    dc[q] = d[id[q]];
                }
                int64_t kk[TS_MESH_CELL_MAX_TRIS][3];
                int32_t a[TS_MESH_CELL_MAX_TRIS][3], z[TS_MESH_CELL_MAX_TRIS][3];
                const int n = ts_mesh_cell(dc, level, id, kk, a, z);
                for (int m = 0; m < n; ++m, ++t) {
                    if (t >= room) continue;
                    for (int v = 0; v < 3; ++v) {
                        float pa[3], pz[3];
                        for (int x = 0; x < 3; ++x) {
                            pa[x] = ts_mesh_corner_pos(lo[x], h, c[x] + ((a[m][v] >> x) & 1));
                            pz[x] = ts_mesh_corner_pos(lo[x], h, c[x] + ((z[m][v] >> x) & 1));
                        }
                        keys[t * 3 + v] = kk[m][v];
                        ts_mesh_interp(level, dc[a[m][v]], dc[z[m][v]], pa, pz, positions + (t * 3 + v) * 3);
                    }
                    cells[t] = ((int64_t)k * ny + j) * nx + i;
                }
            }
    return t;
}

}  // extern "C"
