// Host build of csrc/clean_math.h for tests/test_clean_cpu.py: the functions the kernels of csrc/clean.hip call, behind
// a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/clean_math.h"

extern "C" {

// faces [f,3] of a mesh of v vertices -> keys [3 f], entry 3 face + k the edge from corner k to corner (k + 1) % 3
void cm_edge_keys(int64_t f, int32_t v, const int32_t* faces, int64_t* keys) {
    for (int64_t i = 0; i < f; ++i)
        for (int k = 0; k < 3; ++k) keys[3 * i + k] = ts_clean_edge_key(faces[3 * i + k], faces[3 * i + (k + 1) % 3], v);
}

// vertices [v,3], faces [f,3] -> weights [f]
void cm_face_weights(int64_t f, const float* vertices, const int32_t* faces, double* weights) {
    for (int64_t i = 0; i < f; ++i)
        weights[i] = ts_clean_face_weight(vertices + 3 * (int64_t)faces[3 * i], vertices + 3 * (int64_t)faces[3 * i + 1],
                                          vertices + 3 * (int64_t)faces[3 * i + 2]);
}

}  // extern "C"
