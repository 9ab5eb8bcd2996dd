// Host build of csrc/vote_math.h for tests/test_semantic_cpu.py: the quantisation of a compositing weight and the rule
// that turns rows of votes into labels, the functions the kernels of csrc/votes.hip call, behind a C interface.
#include "../../tinysplat_amd/csrc/vote_math.h"

extern "C" {

uint32_t vh_quantise(float vis) { return ts_vote_quantise(vis); }

// votes: int64 [n, num_classes] -> labels uint8 [n], confidence float32 [n], top and total int64 [n]
int vh_votes_labels(int n, int num_classes, const int64_t* votes, double min_share, uint8_t* labels, float* confidence,
                    int64_t* top, int64_t* total) {
    if (n < 0 || num_classes < 1 || num_classes > TS_VOTE_MAX_CLASSES) return -1;
    for (int g = 0; g < n; ++g) {
        const int best = ts_vote_argmax(votes + (size_t)g * num_classes, num_classes, &top[g], &total[g]);
        labels[g] = ts_vote_label(best, top[g], total[g], min_share, &confidence[g]);
    }
    return 0;
}

}  // extern "C"
