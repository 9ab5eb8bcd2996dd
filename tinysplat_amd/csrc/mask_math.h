// mask_math.h - what the masked loss (train.hip), the masked metrics (metrics.hip) and a host build (tests/mask_cases.py)
// share: the weight of a mask byte and the substituted image the masked loss reads.
//
//   weight    m = (float)b / 255.0f, the correctly rounded float32 quotient; the kernels take it from a 256-entry table
//             filled with this expression, one division per value.  255 -> 1.0f (the pixel counts), 0 -> 0.0f (ignored)
//   blend     x' = x where b == 255, fmaf(m, x - y, y) otherwise: the rendered value x pulled towards the target y by
//             the pixel's weight.  b == 0 gives y exactly (fmaf(0, d, y) == y for every finite d).  The plain expression
//             y + m (x - y) does not return x at m == 1 (x - y is rounded, and so is the sum), hence the select: with it
//             an all-255 mask is the identity, bit for bit.  The fused multiply-add rounds once: a float64 evaluation of
//             y + m (x - y) rounded to float32 is within one float32 ulp of it.
#ifndef TINYSPLAT_MASK_MATH_H
#define TINYSPLAT_MASK_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_MASK_HD __host__ __device__ inline
#else
#define TS_MASK_HD inline
#endif

TS_MASK_HD float ts_mask_weight(uint8_t b) { return (float)b / 255.0f; }

// m: ts_mask_weight(b), handed in because the kernels read it from their table
TS_MASK_HD float ts_mask_blend_value(float x, float y, uint8_t b, float m) {
    return b == 255 ? x : fmaf(m, x - y, y);
}

#endif  // TINYSPLAT_MASK_MATH_H
