// Host build of csrc/mcmc_math.h for tests/test_mcmc_cpu.py and tests/test_gpu_mcmc.py: the functions the kernels of
// csrc/mcmc.hip call, behind a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/mcmc_math.h"

extern "C" {

int32_t mc_n_max() { return TS_MCMC_N_MAX; }

uint64_t mc_binom(int32_t n, int32_t k) { return kTsMcmcBinom.c[n][k]; }

float mc_sigmoid(float x) { return ts_mcmc_sigmoid(x); }

int32_t mc_pick(int32_t n, const double* P, const double* w, double target) { return ts_mcmc_pick(n, P, w, target); }

// draws over an exact prefix: P_i = w_0 + ... + w_i as a running sum (the tests use weights whose sums are exact)
void mc_sample(int32_t n, int32_t m, const double* P, const double* w, const float* u, int32_t* picks) {
    for (int32_t j = 0; j < m; ++j) picks[j] = ts_mcmc_pick(n, P, w, (double)u[j] * P[n - 1]);
}

double mc_split_opacity(double o, int32_t M) { return ts_mcmc_split_opacity(o, M); }

double mc_series(double op, int32_t M) { return ts_mcmc_series(op, M); }

void mc_relocate_values(float o, int32_t M, float* new_opacity, float* coeff) {
    ts_mcmc_relocate_values(o, M, new_opacity, coeff);
}

void mc_relocate(float o, int32_t count, float min_opacity, float* new_logit, float* log_coeff) {
    ts_mcmc_relocate(o, count, min_opacity, new_logit, log_coeff);
}

void mc_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { ts_philox4x32_10(ctr, key, out); }

float mc_uniform(uint32_t x) { return ts_mcmc_uniform(x); }

// rows first .. first + count - 1 -> out [count, 3]
void mc_normals(uint64_t seed, uint32_t step, uint32_t first, int32_t count, float* out) {
    for (int32_t i = 0; i < count; ++i)
        ts_mcmc_normals3((uint32_t)seed, (uint32_t)(seed >> 32), first + (uint32_t)i, step, out + 3 * i);
}

float mc_gate(float o) { return ts_mcmc_gate(o); }

void mc_sigma_z(const float* q, const float* s, const float* z, float* d) { ts_mcmc_sigma_z(q, s, z, d); }

}  // extern "C"
