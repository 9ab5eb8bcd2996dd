// clean_math.h - the arithmetic of the mesh clean-up (clean.hip), for host and device.
//
//   edge key  the undirected edge {a, b} of a mesh of V vertices: min(a, b) V + max(a, b), int64 (below 2^62 for any
//             int32 V).  Entry 3 face + k of a mesh's edge list is the edge from corner k to corner (k + 1) % 3.
//   weight    of face (a, b, c), float32 positions: A2 = (n_x n_x + n_y n_y) + n_z n_z with n = (b - a) x (c - a), four
//             times the squared area, all in double.  The differences are taken first; each cross component is one
//             product minus another, in the order u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x; nothing is
//             contracted (compiled with -ffp-contract=off).  numpy forms the same IEEE operations, so the ranking by A2
//             is exact.
#ifndef TINYSPLAT_CLEAN_MATH_H
#define TINYSPLAT_CLEAN_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_CLEAN_HD __host__ __device__ inline
#else
#define TS_CLEAN_HD inline
#endif

TS_CLEAN_HD int64_t ts_clean_edge_key(int32_t a, int32_t b, int32_t v) {
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * (int64_t)v + hi;
}

TS_CLEAN_HD double ts_clean_face_weight(const float a[3], const float b[3], const float c[3]) {
    const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
    const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    return (nx * nx + ny * ny) + nz * nz;
}

#endif
