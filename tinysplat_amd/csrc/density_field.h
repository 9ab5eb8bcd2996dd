// density_field.h - the device side of the packed-record SuGaR density (DESIGN.md sections 6f and 6g): the record
// layout, the rotation the records are packed from, one neighbour's term and the 16-neighbour density of a point.
// extract.hip (pack, march), mesh.hip (boxes, density) and field_color.hip (the term as a colour's weight) include it: the level set the march samples is the one the mesh cuts, and a Gaussian's
// box is a statement about the R its record was packed from, because each is written once, here.
// density.hip is not a user: the regulariser works on raw parameters in float32 and has an oracle of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"

namespace {

constexpr int kK = TS_EXTRACT_K;
constexpr int kRec = TS_EXTRACT_RECORD;             // mean xyz | U00 U01 U02 U11 U12 U22 | sigmoid(o)

// quat_to_rot_tensor (utils.py:42-64) of q / max(|q|, 1e-12), from the float32 parameters, in double
__device__ __forceinline__ void quat_rotation(float qw, float qx, float qy, float qz, double R[3][3]) {
    const float qf[4] = {qw, qx, qy, qz};
    double q[4];
    for (int c = 0; c < 4; ++c) q[c] = (double)qf[c];
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double den = fmax(nrm, 1e-12);
    const double w = q[0] / den, x = q[1] / den, y = q[2] / den, z = q[3] / den;
    R[0][0] = 1. - 2. * (y * y + z * z); R[0][1] = 2. * (x * y - w * z); R[0][2] = 2. * (x * z + w * y);
    R[1][0] = 2. * (x * y + w * z); R[1][1] = 1. - 2. * (x * x + z * z); R[1][2] = 2. * (y * z - w * x);
    R[2][0] = 2. * (x * z - w * y); R[2][1] = 2. * (y * z + w * x); R[2][2] = 1. - 2. * (x * x + y * y);
}

// one neighbour's term of the density at p, from its 40-byte record: sigmoid(o) exp(-clamp(q, 0, 1e8) / 2),
// q = |U (p - mu)|^2.  density_at sums it; field_color.hip weighs the neighbour's colour by it.
__device__ __forceinline__ float neighbour_weight(const float* p, const float* __restrict__ records, int j) {
    const float2* r2 = reinterpret_cast<const float2*>(records + (int64_t)j * kRec);           // 40-byte records
    const float2 a = r2[0], b = r2[1], c = r2[2], d = r2[3], e = r2[4];
    const float dx = p[0] - a.x, dy = p[1] - a.y, dz = p[2] - b.x;
    const float y0 = (b.y * dx + c.x * dy) + c.y * dz;
    const float y1 = d.x * dy + d.y * dz;
    const float y2 = e.x * dz;
    const float qq = (y0 * y0 + y1 * y1) + y2 * y2;
    // a q that is not a number (an infinite entry of U times a zero offset) counts as the clamp's upper end:
    // the neighbour contributes nothing; fminf / fmaxf alone would turn it into 0 and a full sigmoid(o)
    const float q = qq == qq ? fminf(fmaxf(qq, 0.f), 1e8f) : 1e8f;
    return e.y * expf(-0.5f * q);
}

// the density of one point over K neighbour records: the sum of neighbour_weight, values above 1 set to 1
__device__ __forceinline__ float density_at(int n, const float* p, const int32_t* __restrict__ nbr,
                                            const float* __restrict__ records) {
    float dsum = 0.f;
    const int4* nb4 = reinterpret_cast<const int4*>(nbr);        // rows of 16 int32: 64-byte aligned
#pragma unroll
    for (int g = 0; g < kK / 4; ++g) {
        const int4 v = nb4[g];
        const int js[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = js[t];
            if (j < 0 || j >= n) continue;
            dsum += neighbour_weight(p, records, j);
        }
    }
    return dsum > 1.f ? 1.f : dsum;                 // d[d > 1] = 1 + 1e-12, which is 1.0 in float32
}

}  // namespace
