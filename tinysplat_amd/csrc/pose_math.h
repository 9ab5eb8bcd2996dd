// pose_math.h - one Gaussian's share of the gradient of a loss with respect to a camera's pose (pose.hip, DESIGN.md
// section 6u), for host and device.
//
//   The view matrix V = [R | t] (R orthonormal) is perturbed on the left, V(delta) = Exp(delta) V with delta = (v, omega).
//   The loss reaches V only through the camera-space means R m + t and the camera-space orientations R R(q) (the colour
//   stage gives no gradient to the view directions), so with g = dL/dm and h = dL/dq (q raw, w x y z) at delta = 0
//
//     p    = R m + t                                   p_i  = ((R_i0 m_0 + R_i1 m_1) + R_i2 m_2) + t_i
//     gc   = R g                                       gc_i = (R_i0 g_0 + R_i1 g_1) + R_i2 g_2
//     tau  = 1/2 (h . (e_x (x) q), h . (e_y (x) q), h . (e_z (x) q))        world-frame torque, Hamilton products:
//            tau_x = 1/2 (((h_1 w - h_0 x) - h_2 z) + h_3 y)
//            tau_y = 1/2 (((h_2 w - h_0 y) + h_1 z) - h_3 x)
//            tau_z = 1/2 (((h_3 w - h_0 z) - h_1 y) + h_2 x)
//     dL/dv     += gc
//     dL/domega += p x gc + R tau                      (p x gc)_x = p_y gc_z - p_z gc_y, ...; R tau summed as gc is
//
// Every input is a float32 widened to double (exact); every product and sum is a double operation rounded on its own, in
// the order written (compiled with -ffp-contract=off).  The six terms of a row are defined as the bits of this header's
// host build (tests/hostmath/pose.cpp).
//
// The sum over rows is fixed by n alone: wave w owns rows [TS_POSE_WAVE_ROWS w, TS_POSE_WAVE_ROWS (w + 1)), lane l of it
// adds the rows l, l + 64, l + 128, ... of that range in this order to six sums that start at +0.0, the 64 lanes are
// added by the tree s_l <- s_l + s_(l + d), d = 32, 16, .., 1 (what the butterfly s_l <- s_l + s_(l ^ d) leaves in lane
// 0), the TS_POSE_BLOCK_WAVES wave sums of a workgroup are added left to right into the workgroup's record (a wave past
// the last row holds +0.0), slot i of the second pass adds the records i, i + TS_POSE_REDUCE_THREADS, ... in this order,
// and the slots are added by the same tree, d = TS_POSE_REDUCE_THREADS / 2, .., 1.
#ifndef TINYSPLAT_POSE_MATH_H
#define TINYSPLAT_POSE_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_POSE_HD __host__ __device__ inline
#else
#define TS_POSE_HD inline
#endif

#define TS_POSE_TERMS 6               // dL/dv (3), dL/domega (3)
#define TS_POSE_LANES 64
#define TS_POSE_LANE_ROWS 4           // rows a lane adds
#define TS_POSE_WAVE_ROWS (TS_POSE_LANES * TS_POSE_LANE_ROWS)
#define TS_POSE_BLOCK_WAVES 4         // waves whose sums make one record
#define TS_POSE_BLOCK_ROWS (TS_POSE_WAVE_ROWS * TS_POSE_BLOCK_WAVES)
#define TS_POSE_REDUCE_THREADS 1024   // slot i of the second pass adds the records i, i + 1024, ... in this order

// the 3x4 view matrix, row-major [R | t] as camera.view_matrix[:3, :] stores it; travels to the kernel by value
struct ts_pose_view {
    float m[12];
};

// records (workgroups of the first pass) of n rows
TS_POSE_HD int64_t ts_pose_records(int64_t n) { return (n + TS_POSE_BLOCK_ROWS - 1) / TS_POSE_BLOCK_ROWS; }

// acc[6] += the six terms of one row; m [3], q [4] (w x y z, raw), g [3] = dL/dm, h [4] = dL/dq
TS_POSE_HD void ts_pose_row_add(const ts_pose_view& view, const float* m, const float* q, const float* g, const float* h,
                                double* acc) {
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (double)view.m[4 * i + k];
        t[i] = (double)view.m[4 * i + 3];
    }
    const double m0 = m[0], m1 = m[1], m2 = m[2], g0 = g[0], g1 = g[1], g2 = g[2];
    const double w = q[0], x = q[1], y = q[2], z = q[3], h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
    double p[3], gc[3], rt[3];
    const double tx = 0.5 * (((h1 * w - h0 * x) - h2 * z) + h3 * y);
    const double ty = 0.5 * (((h2 * w - h0 * y) + h1 * z) - h3 * x);
    const double tz = 0.5 * (((h3 * w - h0 * z) - h1 * y) + h2 * x);
    for (int i = 0; i < 3; ++i) {
        p[i] = ((R[3 * i] * m0 + R[3 * i + 1] * m1) + R[3 * i + 2] * m2) + t[i];
        gc[i] = (R[3 * i] * g0 + R[3 * i + 1] * g1) + R[3 * i + 2] * g2;
        rt[i] = (R[3 * i] * tx + R[3 * i + 1] * ty) + R[3 * i + 2] * tz;
    }
    acc[0] += gc[0];
    acc[1] += gc[1];
    acc[2] += gc[2];
    acc[3] += (p[1] * gc[2] - p[2] * gc[1]) + rt[0];
    acc[4] += (p[2] * gc[0] - p[0] * gc[2]) + rt[1];
    acc[5] += (p[0] * gc[1] - p[1] * gc[0]) + rt[2];
}

#endif  // TINYSPLAT_POSE_MATH_H
