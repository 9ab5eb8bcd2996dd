// Host build of csrc/simplify_math.h for tests/test_simplify_cpu.py: the functions the kernels of csrc/simplify.hip call,
// behind a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/simplify_math.h"

extern "C" {

int32_t sm_cells(float lo, float hi, float c) { return ts_simplify_cells(lo, hi, c); }

int32_t sm_cell(float p, float lo, float c, int32_t n) { return ts_simplify_cell(p, lo, c, n); }

void sm_keys(int64_t v, const float* vertices, const float* lo, float c, const int32_t* n, int64_t* keys) {
    for (int64_t i = 0; i < v; ++i) keys[i] = ts_simplify_key(vertices + 3 * i, lo, c, n);
}

double sm_centre(float lo, float c, int32_t i) { return ts_simplify_centre(lo, c, i); }

void sm_face_term(const float* a, const float* b, const float* c, const double* g, double* q) {
    ts_simplify_face_term(a, b, c, g, q);
}

// A [count,6] -> lam [count,3], vec [count,3,3] (vec[r][c]: component r of eigenvector c)
void sm_jacobi(int64_t count, const double* A, int32_t sweeps, double* lam, double* vec) {
    for (int64_t i = 0; i < count; ++i) {
        const ts_simplify_eig e = ts_simplify_jacobi(A + 6 * i, sweeps);
        const double l[3] = {e.l0, e.l1, e.l2};
        const double v[9] = {e.v00, e.v01, e.v02, e.v10, e.v11, e.v12, e.v20, e.v21, e.v22};
        for (int k = 0; k < 3; ++k) lam[3 * i + k] = l[k];
        for (int k = 0; k < 9; ++k) vec[9 * i + k] = v[k];
    }
}

// quadrics [count,10], vertex sums [count,4] -> x [count,3]
void sm_representative(int64_t count, const double* q, const double* s, double c, double tau, double* x) {
    for (int64_t i = 0; i < count; ++i) ts_simplify_representative(q + 10 * i, s + 4 * i, c, tau, x + 3 * i);
}

int32_t sm_sweeps() { return TS_SIMPLIFY_SWEEPS; }

}  // extern "C"
