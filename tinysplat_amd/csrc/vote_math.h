// vote_math.h - what the label-vote kernels (votes.hip) and a host build (tests/hostmath/votes.cpp)
// share: the quantisation of a compositing weight and the rule that turns a Gaussian's row of votes into a label.
//
//   weight    vis in [0, 1) is the float32 weight with which the forward compositing kernel blends a Gaussian into a
//             pixel.  2^24 vis is exact in float32 (a power-of-two scale), rint rounds it half-to-even to an integer
//             <= 2^24 - 1; 256 pixels of a tile sum below 2^32, a wave's sum fits 32 bits and everything behind it is
//             integer addition: associative, so a row of votes does not depend on tile, wave, view or batch order
//   row       votes int64 [C].  top = the largest entry, ties to the SMALLER column (first maximum); total = the row sum
//   label     argmax where total > 0 and double(top) >= min_share * double(total), else TS_VOTE_NONE;
//             confidence = float32(double(top) / double(total)), 0 where total == 0.  The product and the quotient are
//             single double operations: nothing here can contract
#ifndef TINYSPLAT_VOTE_MATH_H
#define TINYSPLAT_VOTE_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_VOTE_HD __host__ __device__ inline
#else
#define TS_VOTE_HD inline
#endif

#define TS_VOTE_SCALE 16777216.0f            // 2^24
#define TS_VOTE_NONE 255                     // the label of a Gaussian without one, and the column of a pixel that does not vote
#define TS_VOTE_MAX_CLASSES 255

TS_VOTE_HD uint32_t ts_vote_quantise(float vis) { return (uint32_t)rintf(vis * TS_VOTE_SCALE); }

// -> the first column holding the row's maximum; *top = that entry, *total = the row's sum
TS_VOTE_HD int ts_vote_argmax(const int64_t* row, int num_classes, int64_t* top, int64_t* total) {
    int best = 0;
    int64_t t = row[0], sum = row[0];
    for (int c = 1; c < num_classes; ++c) {
        const int64_t v = row[c];
        sum += v;
        if (v > t) { t = v; best = c; }
    }
    *top = t;
    *total = sum;
    return best;
}

TS_VOTE_HD uint8_t ts_vote_label(int argmax, int64_t top, int64_t total, double min_share, float* confidence) {
    *confidence = total > 0 ? (float)((double)top / (double)total) : 0.0f;
    return (total > 0 && (double)top >= min_share * (double)total) ? (uint8_t)argmax : (uint8_t)TS_VOTE_NONE;
}

#endif  // TINYSPLAT_VOTE_MATH_H
