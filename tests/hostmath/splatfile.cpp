// Host build of csrc/splat_record.h for tests/test_splat_cpu.py: the functions the kernels of csrc/splatfile.hip call,
// behind a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/splat_record.h"

extern "C" {

// scales [n,3], opacities [n] -> keys [n]
void sr_keys(int64_t n, const float* scales, const float* opacities, float* keys) {
    for (int64_t i = 0; i < n; ++i) keys[i] = ts_splat_key(scales + 3 * i, opacities[i]);
}

// the five tensors' rows -> records [n,32]
void sr_encode(int64_t n, const float* means, const float* scales, const float* dc, const float* opacities,
               const float* quats, uint8_t* records) {
    for (int64_t i = 0; i < n; ++i) {
        const ts_splat_words r = ts_splat_encode(means + 3 * i, scales + 3 * i, dc + 3 * i, opacities[i], quats + 4 * i);
        memcpy(records + 32 * i, r.lo, 16);
        memcpy(records + 32 * i + 16, r.hi, 16);
    }
}

// records [n,32] -> the five tensors' rows
void sr_decode(int64_t n, const uint8_t* records, float* means, float* scales, float* dc, float* opacities,
               float* quats) {
    for (int64_t i = 0; i < n; ++i) {
        ts_splat_words r;
        memcpy(r.lo, records + 32 * i, 16);
        memcpy(r.hi, records + 32 * i + 16, 16);
        ts_splat_decode(r, means + 3 * i, scales + 3 * i, dc + 3 * i, opacities + i, quats + 4 * i);
    }
}

}  // extern "C"
