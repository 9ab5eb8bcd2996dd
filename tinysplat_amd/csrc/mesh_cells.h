// mesh_cells.h - the per-cell routine of the iso-surface mesher (mesh.hip), for host and device.
//
// Marching tetrahedra on the Freudenthal split: a cell (local corners 0..7, bit 0 = +x, bit 1 = +y, bit 2 = +z) is cut
// into the six tetrahedra {0, a, a|b, 7} over the orders (a, b, c) of the axes 1, 2, 4 - the monotone paths from
// corner 0 to corner 7.  Every cell is cut the same way, so two cells agree on the diagonal of the face they share and
// the surface is closed by construction.  A tetrahedron edge joins corners lo, hi with lo's bits a subset of hi's: 12
// axis edges, 6 face diagonals, 1 body diagonal per cell; lo is also the corner of the lower id.  A vertex sits on an
// edge whose ends differ in `d > level`; its key is id(lo) * 8 + (lo ^ hi) (the direction, 1..7) and its position is
// interpolated from lo to hi in that fixed order: every cell sharing the edge computes the same bits.
//
// The 16 sign cases of a POSITIVELY oriented tetrahedron (v0, v1, v2, v3), det(v1 - v0, v2 - v0, v3 - v0) > 0, bit i of
// the case = vertex i above.  Edge uv = the vertex on the edge between vertices u < v.  Derivation: with one vertex a
// above and the others b, c, d such that (a, b, c, d) is positively oriented, the triangle (ab, ac, ad) has its normal
// pointing away from a, towards falling density.  With a, b above and c, d below, (a, b, c, d) positively oriented,
// the quad ac, ad, bd, bc is cut into (ac, ad, bd), (ac, bd, bc), normal towards c, d.  Three above is one above
// reversed.  A listing of (above ascending, below ascending) that is an odd permutation of (0, 1, 2, 3) reverses the
// triangles.  Three of the six tetrahedra are negatively oriented (kMeshTetFlip): their triangles are reversed again.
// tests/test_mesh_cpu.py runs all 256 corner patterns against a mesher that derives its triangles from positions.
#ifndef TINYSPLAT_MESH_CELLS_H
#define TINYSPLAT_MESH_CELLS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_MESH_HD __host__ __device__ inline
#else
#define TS_MESH_HD inline
#endif

#define TS_MESH_BRICK 8                 /* cells along a brick's edge */
#define TS_MESH_BRICK_CELLS 512
#ifndef TS_MESH_BRICK_CORNERS
#define TS_MESH_BRICK_CORNERS 729       /* 9^3 */
#endif
#define TS_MESH_CELL_MAX_TRIS 12        /* six tetrahedra, two triangles each */

// Corner i of an axis: the one expression every stage (and the tests' oracle, in float32) takes a position from.
// Compiled without contraction: the product and the sum are rounded separately.
TS_MESH_HD float ts_mesh_corner_pos(float lo, float h, int32_t i) { return lo + (float)i * h; }

// local cell corner of vertex v (0..3) of tetrahedron t (0..5)
TS_MESH_HD int ts_mesh_tet_corner(int t, int v) {
    // {0,1,3,7} {0,1,5,7} {0,2,3,7} {0,2,6,7} {0,4,5,7} {0,4,6,7}, 3 bits per vertex
    const uint16_t tets[6] = {0 | 1 << 3 | 3 << 6 | 7 << 9, 0 | 1 << 3 | 5 << 6 | 7 << 9, 0 | 2 << 3 | 3 << 6 | 7 << 9,
                              0 | 2 << 3 | 6 << 6 | 7 << 9, 0 | 4 << 3 | 5 << 6 | 7 << 9, 0 | 4 << 3 | 6 << 6 | 7 << 9};
    return (tets[t] >> (3 * v)) & 7;
}

// axis orders x y z, x z y, y x z, y z x, z x y, z y x: the odd ones are negatively oriented
TS_MESH_HD int ts_mesh_tet_flip(int t) { return (0x26 >> t) & 1; }      // t = 1, 2, 5

// the tetrahedron's sign case from the cell's 8-bit pattern
TS_MESH_HD unsigned ts_mesh_tet_case(int t, unsigned above8) {
    unsigned m = 0;
    for (int v = 0; v < 4; ++v) m |= ((above8 >> ts_mesh_tet_corner(t, v)) & 1u) << v;
    return m;
}

TS_MESH_HD int ts_mesh_case_count(unsigned m) {
    // 0 for cases 0 and 15, 2 for the six cases with two vertices above, 1 otherwise: 2 bits per case
    return (int)((0x16696994u >> (2 * m)) & 3u);
}

TS_MESH_HD int ts_mesh_cell_count(unsigned above8) {
    int n = 0;
    for (int t = 0; t < 6; ++t) n += ts_mesh_case_count(ts_mesh_tet_case(t, above8));
    return n;
}

// The triangles of tetrahedron t under the cell pattern above8 -> their number (0..2); ends[3 * j + k] = lo | hi << 3,
// the local cell corners of the edge that carries vertex k of triangle j.
TS_MESH_HD int ts_mesh_tet(int t, unsigned above8, uint8_t ends[6]) {
#define TS_E(u, v) ((u) | (v) << 2)
    const uint8_t cases[16][6] = {
        {0, 0, 0, 0, 0, 0},
        {TS_E(0, 1), TS_E(0, 2), TS_E(0, 3), 0, 0, 0},                                      // 0 above
        {TS_E(0, 1), TS_E(1, 3), TS_E(1, 2), 0, 0, 0},                                      // 1
        {TS_E(0, 2), TS_E(0, 3), TS_E(1, 3), TS_E(0, 2), TS_E(1, 3), TS_E(1, 2)},           // 0 1
        {TS_E(0, 2), TS_E(1, 2), TS_E(2, 3), 0, 0, 0},                                      // 2
        {TS_E(0, 1), TS_E(2, 3), TS_E(0, 3), TS_E(0, 1), TS_E(1, 2), TS_E(2, 3)},           // 0 2
        {TS_E(0, 1), TS_E(1, 3), TS_E(2, 3), TS_E(0, 1), TS_E(2, 3), TS_E(0, 2)},           // 1 2
        {TS_E(0, 3), TS_E(1, 3), TS_E(2, 3), 0, 0, 0},                                      // 0 1 2
        {TS_E(0, 3), TS_E(2, 3), TS_E(1, 3), 0, 0, 0},                                      // 3
        {TS_E(0, 1), TS_E(0, 2), TS_E(2, 3), TS_E(0, 1), TS_E(2, 3), TS_E(1, 3)},           // 0 3
        {TS_E(0, 1), TS_E(2, 3), TS_E(1, 2), TS_E(0, 1), TS_E(0, 3), TS_E(2, 3)},           // 1 3
        {TS_E(0, 2), TS_E(2, 3), TS_E(1, 2), 0, 0, 0},                                      // 0 1 3
        {TS_E(0, 2), TS_E(1, 2), TS_E(1, 3), TS_E(0, 2), TS_E(1, 3), TS_E(0, 3)},           // 2 3
        {TS_E(0, 1), TS_E(1, 2), TS_E(1, 3), 0, 0, 0},                                      // 0 2 3
        {TS_E(0, 1), TS_E(0, 3), TS_E(0, 2), 0, 0, 0},                                      // 1 2 3
        {0, 0, 0, 0, 0, 0}};
#undef TS_E
    const unsigned m = ts_mesh_tet_case(t, above8);
    const int n = ts_mesh_case_count(m);
    const int flip = ts_mesh_tet_flip(t);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < 3; ++k) {
            const int src = (flip && k) ? 3 - k : k;                // reversed: vertices 1 and 2 change places
            const unsigned e = cases[m][3 * j + src];
            ends[3 * j + k] = (uint8_t)(ts_mesh_tet_corner(t, e & 3) | ts_mesh_tet_corner(t, (e >> 2) & 3) << 3);
        }
    return n;
}

// The vertex on the edge from corner lo to corner hi (that order): p_lo + t (p_hi - p_lo), t = (level - d_lo) /
// (d_hi - d_lo).  The ends differ in `d > level`, so d_hi != d_lo and t lies in [0, 1].
TS_MESH_HD void ts_mesh_interp(float level, float d_lo, float d_hi, const float p_lo[3], const float p_hi[3],
                               float out[3]) {
    const float t = (level - d_lo) / (d_hi - d_lo);
    for (int c = 0; c < 3; ++c) out[c] = p_lo[c] + t * (p_hi[c] - p_lo[c]);
}

// One cell: d[c] and id[c] of its 8 corners -> the number of triangles (<= 12), in (tetrahedron, triangle) order;
// per triangle vertex k the edge key id[lo] * 8 + (lo ^ hi) and the local corners lo, hi to interpolate between.
TS_MESH_HD int ts_mesh_cell(const float d[8], float level, const int64_t id[8], int64_t keys[][3], int32_t lo[][3],
                            int32_t hi[][3]) {
    unsigned above8 = 0;
    for (int c = 0; c < 8; ++c) above8 |= (d[c] > level ? 1u : 0u) << c;
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        uint8_t ends[6];
        const int m = ts_mesh_tet(t, above8, ends);
        for (int j = 0; j < m; ++j, ++n)
            for (int k = 0; k < 3; ++k) {
                const int a = ends[3 * j + k] & 7, b = ends[3 * j + k] >> 3;
                lo[n][k] = a;
                hi[n][k] = b;
                keys[n][k] = id[a] * 8 + (a ^ b);
            }
    }
    return n;
}

#endif
