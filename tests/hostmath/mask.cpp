// Host build of csrc/mask_math.h for tests/test_masks_cpu.py and tests/test_gpu_masks.py: a mask byte's weight and the
// substituted image of the masked loss behind a C interface (compiled with -ffp-contract=off; the one fused
// multiply-add is written out in the header).
#include "../../tinysplat_amd/csrc/mask_math.h"

extern "C" {

float kh_weight(int b) { return ts_mask_weight((uint8_t)b); }

// out[pixels, 3] <- blend(x, y, m) as ts_mask_blend computes it, every pointer on the host
void kh_blend(long long pixels, const float* x, const float* y, const uint8_t* mask, float* out) {
    float table[256];
    for (int i = 0; i < 256; ++i) table[i] = ts_mask_weight((uint8_t)i);
    for (long long p = 0; p < pixels; ++p)
        for (int k = 0; k < 3; ++k) out[3 * p + k] = ts_mask_blend_value(x[3 * p + k], y[3 * p + k], mask[p], table[mask[p]]);
}

}  // extern "C"
