// simplify_math.h - the arithmetic of the mesh simplifier (simplify.hip), for host and device:
// vertex clustering on a uniform grid with quadric-optimal representatives (Lindstrom 2000).
//
//   grid      lo = the componentwise minimum of the vertices, cubes of edge c, n_a = max(1, ceil((hi_a - lo_a) / c))
//             cells on axis a.  A coordinate's cell is min(floor((p - lo) / c), n - 1): the float32 subtraction and
//             division are rounded separately (compiled without contraction), so that every stage, and the tests' oracle
//             in float32, files a vertex in the same cell.  The key of a cell is (i_z n_y + i_y) n_x + i_x.
//   quadric   per face (a, b, c) and corner, relative to the centre g of the corner's cell, all in double: the
//             area-weighted plane n = (b - a) x (c - a), d = -n . (a - g), and the ten numbers n n^T (xx xy xz yy yz zz),
//             n d, d^2.  Summed per cluster they give the error sum (n . x + d)^2 = x^T A x + 2 b^T x + d^2.
//   solve     the minimiser of that error closest to the mean m of the cluster's vertices: A's eigen-decomposition by
//             cyclic Jacobi (TS_SIMPLIFY_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2), written out: no array is indexed
//             by a runtime value), x = m + sum over lambda_i > tau lambda_max of v_i (v_i . (-b - A m)) / lambda_i, and m
//             itself where A has no positive finite eigenvalue, x is not finite or x leaves the cell.
#ifndef TINYSPLAT_SIMPLIFY_MATH_H
#define TINYSPLAT_SIMPLIFY_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_SIMPLIFY_HD __host__ __device__ inline
#else
#define TS_SIMPLIFY_HD inline
#endif

#define TS_SIMPLIFY_QUADRIC 10          /* A xx xy xz yy yz zz | b x y z | d^2 */
#define TS_SIMPLIFY_VSUM 4              /* sum (p - g) x y z | the number of vertices */
#define TS_SIMPLIFY_SWEEPS 6            /* cyclic Jacobi sweeps; tests/test_simplify_cpu.py shows 4 converge */

// cells on an axis of extent [lo, hi] (>= 1; saturates below 2^31 - 1, which no grid accepts)
TS_SIMPLIFY_HD int32_t ts_simplify_cells(float lo, float hi, float c) {
    const float q = ceilf((hi - lo) / c);
    if (!(q >= 1.f)) return 1;
    return q >= 2147483520.f ? 2147483520 : (int32_t)q;
}

// the cell of coordinate p on an axis of n cells: min(floor((p - lo) / c), n - 1); below lo (or not a number): cell 0
TS_SIMPLIFY_HD int32_t ts_simplify_cell(float p, float lo, float c, int32_t n) {
    const float q = floorf((p - lo) / c);
    if (!(q > 0.f)) return 0;
    return q >= (float)(n - 1) ? n - 1 : (int32_t)q;
}

TS_SIMPLIFY_HD int64_t ts_simplify_key(const float p[3], const float lo[3], float c, const int32_t n[3]) {
    const int64_t ix = ts_simplify_cell(p[0], lo[0], c, n[0]);
    const int64_t iy = ts_simplify_cell(p[1], lo[1], c, n[1]);
    const int64_t iz = ts_simplify_cell(p[2], lo[2], c, n[2]);
    return (iz * n[1] + iy) * n[0] + ix;
}

// the centre of cell i on an axis, in double
TS_SIMPLIFY_HD double ts_simplify_centre(float lo, float c, int32_t i) { return (double)lo + ((double)i + 0.5) * (double)c; }

// the ten numbers of face (a, b, c) for a corner whose cell is centred at g
TS_SIMPLIFY_HD void ts_simplify_face_term(const float a[3], const float b[3], const float c[3], const double g[3],
                                          double q[TS_SIMPLIFY_QUADRIC]) {
    const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
    const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double d = -((nx * ((double)a[0] - g[0]) + ny * ((double)a[1] - g[1])) + nz * ((double)a[2] - g[2]));
    q[0] = nx * nx;
    q[1] = nx * ny;
    q[2] = nx * nz;
    q[3] = ny * ny;
    q[4] = ny * nz;
    q[5] = nz * nz;
    q[6] = nx * d;
    q[7] = ny * d;
    q[8] = nz * d;
    q[9] = d * d;
}

// One Jacobi rotation in the plane (p, q) of a symmetric 3x3 matrix; r is the third index.  app, aqq, apq, apr, aqr are
// the entries it touches, (v0p, v0q), (v1p, v1q), (v2p, v2q) the rows of the eigenvector columns p and q.
TS_SIMPLIFY_HD void ts_simplify_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p,
                                       double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = cs * apr - sn * aqr, rq = sn * apr + cs * aqr;
    apr = rp;
    aqr = rq;
    const double a0 = cs * v0p - sn * v0q, b0 = sn * v0p + cs * v0q;
    const double a1 = cs * v1p - sn * v1q, b1 = sn * v1p + cs * v1q;
    const double a2 = cs * v2p - sn * v2q, b2 = sn * v2p + cs * v2q;
    v0p = a0; v0q = b0;
    v1p = a1; v1q = b1;
    v2p = a2; v2q = b2;
}

struct ts_simplify_eig {
    double l0, l1, l2;                                  // eigenvalues, in no particular order
    double v00, v01, v02, v10, v11, v12, v20, v21, v22; // vrc: component r of eigenvector c
};

// A = {xx, xy, xz, yy, yz, zz} -> its eigen-decomposition after `sweeps` cyclic sweeps
TS_SIMPLIFY_HD ts_simplify_eig ts_simplify_jacobi(const double A[6], int sweeps) {
    double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
    ts_simplify_eig e;
    e.v00 = 1.0; e.v01 = 0.0; e.v02 = 0.0;
    e.v10 = 0.0; e.v11 = 1.0; e.v12 = 0.0;
    e.v20 = 0.0; e.v21 = 0.0; e.v22 = 1.0;
    for (int s = 0; s < sweeps; ++s) {
        ts_simplify_rotate(a00, a11, a01, a02, a12, e.v00, e.v01, e.v10, e.v11, e.v20, e.v21);     // (0, 1), r = 2
        ts_simplify_rotate(a00, a22, a02, a01, a12, e.v00, e.v02, e.v10, e.v12, e.v20, e.v22);     // (0, 2), r = 1
        ts_simplify_rotate(a11, a22, a12, a01, a02, e.v01, e.v02, e.v11, e.v12, e.v21, e.v22);     // (1, 2), r = 0
    }
    e.l0 = a00;
    e.l1 = a11;
    e.l2 = a22;
    return e;
}

// One eigen-direction's share of the solution: v (v . r) / lambda where lambda > tau lambda_max
TS_SIMPLIFY_HD void ts_simplify_add_direction(double lambda, double bar, double vx, double vy, double vz, double rx,
                                              double ry, double rz, double x[3]) {
    if (!(lambda > bar)) return;
    const double w = ((vx * rx + vy * ry) + vz * rz) / lambda;
    x[0] += vx * w;
    x[1] += vy * w;
    x[2] += vz * w;
}

// The representative of a cluster relative to its cell centre: q = the summed quadric, s = {sum (p - g), count},
// c = the cell edge, tau = the singular threshold -> x, |x_a| <= c / 2
TS_SIMPLIFY_HD void ts_simplify_representative(const double q[TS_SIMPLIFY_QUADRIC], const double s[TS_SIMPLIFY_VSUM],
                                               double c, double tau, double x[3]) {
    const double mx = s[0] / s[3], my = s[1] / s[3], mz = s[2] / s[3];
    x[0] = mx;
    x[1] = my;
    x[2] = mz;
    const ts_simplify_eig e = ts_simplify_jacobi(q, TS_SIMPLIFY_SWEEPS);
    const double lmax = fmax(e.l0, fmax(e.l1, e.l2));
    if (!(lmax > 0.0) || !(lmax <= 1.7976931348623157e308)) return;
    const double rx = -q[6] - ((q[0] * mx + q[1] * my) + q[2] * mz);
    const double ry = -q[7] - ((q[1] * mx + q[3] * my) + q[4] * mz);
    const double rz = -q[8] - ((q[2] * mx + q[4] * my) + q[5] * mz);
    const double bar = tau * lmax;
    double y[3] = {mx, my, mz};
    ts_simplify_add_direction(e.l0, bar, e.v00, e.v10, e.v20, rx, ry, rz, y);
    ts_simplify_add_direction(e.l1, bar, e.v01, e.v11, e.v21, rx, ry, rz, y);
    ts_simplify_add_direction(e.l2, bar, e.v02, e.v12, e.v22, rx, ry, rz, y);
    const double half = 0.5 * c;
    // a value that is not a number fails every comparison: the mean stays
    if (fabs(y[0]) <= half && fabs(y[1]) <= half && fabs(y[2]) <= half) {
        x[0] = y[0];
        x[1] = y[1];
        x[2] = y[2];
    }
}

#endif
