// Host build of csrc/pose_math.h for tests/test_pose_cpu.py and tests/test_gpu_pose.py: the row terms the kernel of
// csrc/pose.hip adds, in the order that header fixes, behind a C interface (compiled with -ffp-contract=off, as the
// kernel is).
#include "../../tinysplat_amd/csrc/pose_math.h"

#include <vector>

extern "C" {

// the arguments of ts_pose_grad with every pointer on the host; view34: 12 floats
void ph_pose_grad(int64_t n, const float* view34, const float* means, const float* quats, const float* v_means,
                  const float* v_quats, double* out6) {
    ts_pose_view view;
    for (int i = 0; i < 12; ++i) view.m[i] = view34[i];
    const int64_t blocks = ts_pose_records(n), waves = blocks * TS_POSE_BLOCK_WAVES;
    std::vector<double> records(TS_POSE_TERMS * (blocks > 0 ? blocks : 1), 0.0);
    for (int64_t w = 0; w < waves; ++w) {
        double lanes[TS_POSE_LANES][TS_POSE_TERMS] = {};
        for (int l = 0; l < TS_POSE_LANES; ++l)
            for (int j = 0; j < TS_POSE_LANE_ROWS; ++j) {
                const int64_t r = w * TS_POSE_WAVE_ROWS + l + (int64_t)j * TS_POSE_LANES;
                if (r < n) ts_pose_row_add(view, means + 3 * r, quats + 4 * r, v_means + 3 * r, v_quats + 4 * r, lanes[l]);
            }
        for (int d = TS_POSE_LANES / 2; d >= 1; d >>= 1)
            for (int l = 0; l < d; ++l)
                for (int k = 0; k < TS_POSE_TERMS; ++k) lanes[l][k] += lanes[l + d][k];
        // the workgroup's record: its waves' sums left to right (the first one copied, not added to a zero)
        double* const rec = &records[TS_POSE_TERMS * (w / TS_POSE_BLOCK_WAVES)];
        for (int k = 0; k < TS_POSE_TERMS; ++k) rec[k] = w % TS_POSE_BLOCK_WAVES == 0 ? lanes[0][k] : rec[k] + lanes[0][k];
    }
    std::vector<double> part(TS_POSE_TERMS * TS_POSE_REDUCE_THREADS, 0.0);
    for (int i = 0; i < TS_POSE_REDUCE_THREADS; ++i)
        for (int64_t r = i; r < blocks; r += TS_POSE_REDUCE_THREADS)
            for (int k = 0; k < TS_POSE_TERMS; ++k) part[TS_POSE_TERMS * i + k] += records[TS_POSE_TERMS * r + k];
    for (int step = TS_POSE_REDUCE_THREADS / 2; step >= 1; step >>= 1)
        for (int i = 0; i < step; ++i)
            for (int k = 0; k < TS_POSE_TERMS; ++k) part[TS_POSE_TERMS * i + k] += part[TS_POSE_TERMS * (i + step) + k];
    for (int k = 0; k < TS_POSE_TERMS; ++k) out6[k] = part[k];
}

// one row's six terms (added to zeros)
void ph_pose_row(const float* view34, const float* m, const float* q, const float* g, const float* h, double* out6) {
    ts_pose_view view;
    for (int i = 0; i < 12; ++i) view.m[i] = view34[i];
    for (int k = 0; k < TS_POSE_TERMS; ++k) out6[k] = 0.0;
    ts_pose_row_add(view, m, q, g, h, out6);
}

}  // extern "C"
