// votes.hip - per-Gaussian label votes: votes[g, c] = the sum, over the pixels of column c, of the
// quantised weight with which the forward compositing kernel blends Gaussian g into the pixel, and the labels that follow
// from a row of votes (vote_math.h).
//
// label_votes_kernel walks the sorted 16x16 tile lists exactly as raster_fwd_kernel (raster.hip) does with one wave per
// tile: the lane's four pixels (one per 8x8 block), 64-entry chunks, every lane stages one record and culls it against
// the rectangles of the blocks' unfinished pixels, the survivors are compacted into LDS and read back wave-uniformly, and
// a chunk runs the GENERAL per-pixel body iff one of its survivors carries the general flag - the forward's choice, made
// from the forward's staging (stage_fields, stage_splat and update_rects below restate raster.hip's: change both; the
// GPU tests hold this kernel to the forward's weights bit for bit).  The per-pixel arithmetic is the C++ form of
// fwd_alpha / fwd_update under `fp contract(off)`: the same operations on the same operands in the same order.
// What differs is what a pixel keeps: no colour, only T; and a pixel that does not vote (outside the image, or of an
// ignored label) starts finished, so a tile without voters ends before its first chunk - a cull of bodies whose weight
// would not be counted.
//
// Per list entry with a non-zero weight the wave sums its lanes' quantised weights per distinct column of the tile (the
// set is built once per tile with a ballot / first-lane loop; one column is the common case and has a path of its own),
// reduces the 32-bit sums with DPP inside the rows of 16 and four lane reads across them, and one lane adds the total to
// votes[g, c] with an integer atomic.  Integer addition is associative: the result is the same bits whatever the order.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "splat_math.h"
#include "vote_math.h"

namespace {

constexpr int kWaves = 4;                 // tiles (= waves) per workgroup; the waves never synchronise
constexpr int kThreads = 64 * kWaves;
constexpr int NBC = 2, NB = NBC * NBC;    // a tile as 2 x 2 blocks of 8 x 8 pixels, lane l at (l & 7, l >> 3) of each
constexpr int kLabelThreads = 256;
using ts::kLog2e;
using ts::kLog2_255;

#define TS_VOTE_WAVE_SYNC()                                       \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

// ---- raster.hip's staging, restated -------------------------------------------------------------------------------
__device__ __forceinline__ float sigma_l2(float hA, float B, float hC, float neg_lo, float dx, float dy) {
    float s = __builtin_fmaf(hC * dy, dy, neg_lo);
    s = __builtin_fmaf(hA * dx, dx, s);
    return __builtin_fmaf(B * dx, dy, s);
}

__device__ __forceinline__ int xcd_tile_group(int num_groups) {
    const int per_xcd = (num_groups + 7) >> 3;
    return (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
}

struct Staged {
    int mask;                      // bit k: the alpha >= 1/255 level set may reach block k; bit NB: the general body
    float gx, gy, hA, B, hC, lo;
};

__device__ __forceinline__ bool mask_rect(unsigned long long m, int& xmin, int& xmax, int& ymin, int& ymax) {
    if (m == 0ull) return false;
    ymin = __builtin_ctzll(m) >> 3;
    ymax = (63 - __builtin_clzll(m)) >> 3;
    unsigned int c = (unsigned int)(m | (m >> 32));
    c |= c >> 16;
    c |= c >> 8;
    c &= 0xffu;
    xmin = __builtin_ctz(c);
    xmax = 31 - __builtin_clz(c);
    return true;
}

__device__ __forceinline__ Staged stage_splat(bool have, const float4 q0, const float2 q1, const float4* __restrict__ rects,
                                              int blocks) {
    Staged s;
    s.gx = q0.x; s.gy = q0.y;
    const float A = q0.w, Bc = q1.x, Cc = q1.y, op = q0.z;
    s.hA = 0.5f * kLog2e * A;
    s.B = kLog2e * Bc;
    s.hC = 0.5f * kLog2e * Cc;
    s.lo = __log2f(op);
    s.mask = 0;
    const bool general = !(s.hA > 0.0f && s.hC > 0.0f && 4.0f * s.hA * s.hC > s.B * s.B && op <= 0.99f);
    if (have && op > 0.0f) {
        const float tau = s.lo + kLog2_255;
        if (tau >= -0.02f) {
            if (s.hA > 0.0f && s.hC > 0.0f) {
                const float inv2A = 0.5f / s.hA, inv2C = 0.5f / s.hC;
#pragma unroll 1
                for (int k = 0; k < NB; ++k) {
                    if (!(blocks & (1 << k))) continue;
                    const float4 r = rects[k];
                    if (ts::rect_may_contribute(s.hA, s.B, s.hC, inv2A, inv2C, tau, s.gx, s.gy, r.x, r.y, r.z, r.w))
                        s.mask |= (1 << k);
                }
            } else {
                s.mask = blocks;
            }
            if (s.mask != 0 && general) s.mask |= (1 << NB);
        }
    }
    return s;
}

__device__ __forceinline__ int update_rects(const bool (&sel)[NB], float X0, float Y0, float4* rects, int lane) {
    int blocks = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const unsigned long long m = __ballot(sel[k]);
        int xmin, xmax, ymin, ymax;
        if (mask_rect(m, xmin, xmax, ymin, ymax)) {
            blocks |= (1 << k);
            const float bx = X0 + (float)(8 * (k % NBC)), by = Y0 + (float)(8 * (k / NBC));
            if (lane == 0)
                rects[k] = make_float4(bx + (float)xmin, bx + (float)xmax, by + (float)ymin, by + (float)ymax);
        }
    }
    return blocks;
}

// ---- the vote walk ------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ unsigned int dpp_add(unsigned int v) {
    return v + (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// the wave's sum of a 32-bit value, as a scalar: two quad levels, row_half_mirror and row_mirror leave every lane of a
// row of 16 with the row's sum; the four rows are read out and added on the scalar unit
__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) {
    v = dpp_add<0xB1>(v);          // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);          // quad_perm:[2,3,0,1]
    v = dpp_add<0x141>(v);         // row_half_mirror
    v = dpp_add<0x140>(v);         // row_mirror
    return (unsigned int)__builtin_amdgcn_readlane((int)v, 0) + (unsigned int)__builtin_amdgcn_readlane((int)v, 16) +
           (unsigned int)__builtin_amdgcn_readlane((int)v, 32) + (unsigned int)__builtin_amdgcn_readlane((int)v, 48);
}

// The `cnt` staged entries of one chunk: T as in fwd_chunk (T > 0: unfinished; T < 0: finished, outside or not voting),
// the weight of every flagged block's pixel, and the entry's votes.
//   col[k]: the column of the lane's pixel in block k (TS_VOTE_NONE: none) | cols[0 .. ncols): the tile's distinct columns
template <bool GENERAL>
__device__ __forceinline__ void vote_chunk(const float4* __restrict__ lds, int cnt, const float (&fpx)[NBC],
                                           const float (&fpy)[2], float (&T)[NB], const int (&col)[NB],
                                           const int* __restrict__ cols, int ncols, int num_classes,
                                           unsigned long long* __restrict__ votes, int lane) {
#pragma clang fp contract(off)
    const int c0 = __builtin_amdgcn_readfirstlane(cols[0]);
    for (int j = 0; j < cnt; ++j) {
        const float4 r0 = lds[2 * j], r1 = lds[2 * j + 1];
        const int bm = __builtin_amdgcn_readfirstlane(__float_as_int(r1.w));
        const int g = __builtin_amdgcn_readfirstlane(__float_as_int(r1.z));
        const float neg_lo = -r1.y;
        unsigned int q[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            q[k] = 0u;
            if (!(bm & (1 << k))) continue;                           // wave-uniform
            const float sgl = sigma_l2(r0.z, r0.w, r1.x, neg_lo, r0.x - fpx[k % NBC], r0.y - fpy[k / NBC]);
            const float a = __builtin_amdgcn_exp2f(-sgl);
            float ae = a >= ts::kAlphaMin ? a : 0.0f;                 // alpha >= 1/255 ? alpha : 0
            if (GENERAL) {
                ae = fminf(ts::kAlphaMax, ae);
                ae = sgl >= neg_lo ? ae : 0.0f;                       // sigma >= 0
            }
            const float nT = __builtin_fmaf(-ae, T[k], T[k]);
            const float d = T[k] - nT;
            const bool goes_on = !(nT <= ts::kTEps);                  // the stopping Gaussian is not composited
            const float vis = goes_on ? d : 0.0f;
            T[k] = goes_on ? nT : -__builtin_fabsf(T[k]);
            q[k] = ts_vote_quantise(vis);
        }
        if (__ballot((q[0] | q[1] | q[2] | q[3]) != 0u) == 0ull) continue;
        unsigned long long* row = votes + (size_t)g * (size_t)num_classes;
        if (ncols == 1) {
            // every voting pixel of the tile has column c0 (the others have weight 0: they started finished)
            const unsigned int total = wave_sum_u32(q[0] + q[1] + q[2] + q[3]);
            if (lane == 0) atomicAdd(row + c0, (unsigned long long)total);
        } else {
#pragma unroll 1
            for (int i = 0; i < ncols; ++i) {
                const int c = __builtin_amdgcn_readfirstlane(cols[i]);
                unsigned int v = 0u;
#pragma unroll
                for (int k = 0; k < NB; ++k) v += col[k] == c ? q[k] : 0u;
                if (__ballot(v != 0u) == 0ull) continue;              // the entry has no weight in this column
                const unsigned int total = wave_sum_u32(v);
                if (lane == 0) atomicAdd(row + c, (unsigned long long)total);
            }
        }
    }
}

template <bool MAP>
__global__ __launch_bounds__(kThreads) void label_votes_kernel(
    const ts_camera cam, const int num_tiles, const int* __restrict__ tile_bins, const int* __restrict__ ids,
    const float4* __restrict__ splats, const uint8_t* __restrict__ labels, const uint8_t* __restrict__ class_map,
    const int num_classes, unsigned long long* __restrict__ votes) {
    __shared__ float4 lds_all[kWaves][64 * 2];
    __shared__ float4 rect_all[kWaves][NB];
    __shared__ int cols_all[kWaves][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = xcd_tile_group((num_tiles + kWaves - 1) / kWaves) * kWaves + wave;
    if (tile >= num_tiles) return;
    float4* lds = lds_all[wave];
    float4* rects = rect_all[wave];
    int* cols = cols_all[wave];
    const int tbx = cam.tile_bounds_x;
    const int tx = tile % tbx, ty = tile / tbx + cam.tile_row0;
    const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
    float fpx[NBC];
#pragma unroll
    for (int c = 0; c < NBC; ++c) fpx[c] = (float)(px0 + 8 * c) + ts::kPixOff;
    const float fpy[2] = {(float)py0 + ts::kPixOff, (float)(py0 + 8) + ts::kPixOff};
    const float X0 = (float)(tx * 16) + ts::kPixOff, Y0 = (float)(ty * 16) + ts::kPixOff;
    const int W = cam.img_width, H = cam.img_height;

    const int2 range = reinterpret_cast<const int2*>(tile_bins)[tile];
    if (range.x >= range.y) return;

    // the lane's columns; a pixel outside the image, of an ignored label or of a column the table does not have starts
    // finished and never votes
    float T[NB];
    int col[NB];
    int pending = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int px = px0 + 8 * (k % NBC), py = py0 + 8 * (k / NBC);
        int c = TS_VOTE_NONE;
        if (px < W && py < H) c = MAP ? (int)class_map[labels[(size_t)py * (size_t)W + (size_t)px]] : 0;
        if (c >= num_classes) c = TS_VOTE_NONE;
        col[k] = c;
        T[k] = c != TS_VOTE_NONE ? 1.0f : -1.0f;
        if (c != TS_VOTE_NONE) pending |= 1 << k;
    }
    // the wave-uniform set of distinct columns: the first lane with a pixel not yet covered names its column, every pixel
    // of that column is covered (at least one per round: at most 255 rounds, usually one to three)
    int ncols = 0;
    for (;;) {
        const unsigned long long m = __ballot(pending != 0);
        if (m == 0ull) break;
        const int k0 = __builtin_ctz(pending | 16);
        const int mine = k0 == 0 ? col[0] : (k0 == 1 ? col[1] : (k0 == 2 ? col[2] : col[3]));
        const int c = __builtin_amdgcn_readlane(mine, __builtin_ctzll(m));
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (col[k] == c) pending &= ~(1 << k);
        if (lane == 0) cols[ncols] = c;
        ++ncols;
    }
    if (ncols == 0) return;
    TS_VOTE_WAVE_SYNC();

    // software pipeline over 64-entry chunks: the id of chunk c + 2 and the record of chunk c + 1 are in flight while
    // chunk c is walked.  A record's first 24 bytes are all the walk reads: {x, y, opacity, conic.xx | conic.xy, conic.yy}
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float2 zero2 = make_float2(0.f, 0.f);
    int g_cur = 0, g_next = 0;
    float4 q0 = zero4;
    float2 q1 = zero2;
    if (range.x + lane < range.y) {
        g_cur = ids[range.x + lane];
        q0 = splats[3 * (size_t)g_cur];
        q1 = *reinterpret_cast<const float2*>(splats + 3 * (size_t)g_cur + 1);
    }
    if (range.x + 64 + lane < range.y) g_next = ids[range.x + 64 + lane];

    int live = (1 << NB) - 1;
    for (int base = range.x; base < range.y && live != 0; base += 64) {
        const int i = base + lane;
        const bool have = i < range.y;
        const int g_this = g_cur;
        const float4 p0 = q0;
        const float2 p1 = q1;
        if (i + 64 < range.y) {
            g_cur = g_next;
            q0 = splats[3 * (size_t)g_cur];
            q1 = *reinterpret_cast<const float2*>(splats + 3 * (size_t)g_cur + 1);
        }
        if (i + 128 < range.y) g_next = ids[i + 128];
        {
            bool sel[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) sel[k] = T[k] > 0.0f;
            live = update_rects(sel, X0, Y0, rects, lane);
            TS_VOTE_WAVE_SYNC();
            if (live == 0) break;
        }
        const Staged s = stage_splat(have, p0, p1, rects, live);
        const bool keep = (s.mask & ((1 << NB) - 1)) != 0;
        const unsigned long long mask = __ballot(keep);
        const int cnt = __popcll(mask);
        if (keep) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            lds[2 * pos] = make_float4(s.gx, s.gy, s.hA, s.B);
            lds[2 * pos + 1] = make_float4(s.hC, s.lo, __int_as_float(g_this), __int_as_float(s.mask));
        }
        TS_VOTE_WAVE_SYNC();
        const bool general = __ballot(keep && (s.mask & (1 << NB))) != 0ull;
        if (general)
            vote_chunk<true>(lds, cnt, fpx, fpy, T, col, cols, ncols, num_classes, votes, lane);
        else
            vote_chunk<false>(lds, cnt, fpx, fpy, T, col, cols, ncols, num_classes, votes, lane);
        TS_VOTE_WAVE_SYNC();
    }
}

__global__ __launch_bounds__(kLabelThreads) void votes_labels_kernel(const int n, const int num_classes,
                                                                    const int64_t* __restrict__ votes,
                                                                    const double min_share,
                                                                    uint8_t* __restrict__ labels_out,
                                                                    float* __restrict__ confidence_out) {
    const int g = (int)(blockIdx.x * (unsigned)kLabelThreads + threadIdx.x);
    if (g >= n) return;
    int64_t top, total;
    const int best = ts_vote_argmax(votes + (size_t)g * (size_t)num_classes, num_classes, &top, &total);
    float confidence;
    labels_out[g] = ts_vote_label(best, top, total, min_share, &confidence);
    if (confidence_out) confidence_out[g] = confidence;
}

}  // namespace

extern "C" {

int ts_label_votes(int32_t flags, const ts_camera* cam, const int32_t* tile_bins, const int32_t* gaussian_ids_sorted,
                   const float* splats, const uint8_t* labels, const uint8_t* class_map, int32_t num_classes,
                   int64_t* votes, void* stream) {
    if (flags != 0 || !cam || cam->wide_tiles != 0 || num_classes < 1 || num_classes > TS_VOTE_MAX_CLASSES)
        return TS_E_BADARG;
    if ((labels == nullptr) != (class_map == nullptr)) return TS_E_BADARG;
    if (cam->img_width < 1 || cam->img_height < 1 || cam->tile_row0 < 0 || cam->tile_rows < 0 ||
        cam->tile_bounds_x != (cam->img_width + 15) / 16 || cam->tile_row0 + cam->tile_rows > (cam->img_height + 15) / 16)
        return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (nt <= 0) return 0;
    if (!tile_bins || !gaussian_ids_sorted || !splats || !votes) return TS_E_BADARG;
    const int grid = 8 * (((nt + kWaves - 1) / kWaves + 7) / 8);      // see xcd_tile_group
    hipStream_t s = (hipStream_t)stream;
    const float4* sp = reinterpret_cast<const float4*>(splats);
    unsigned long long* v = reinterpret_cast<unsigned long long*>(votes);
    if (labels)
        hipLaunchKernelGGL(label_votes_kernel<true>, dim3(grid), dim3(kThreads), 0, s, *cam, nt, tile_bins,
                           gaussian_ids_sorted, sp, labels, class_map, num_classes, v);
    else
        hipLaunchKernelGGL(label_votes_kernel<false>, dim3(grid), dim3(kThreads), 0, s, *cam, nt, tile_bins,
                           gaussian_ids_sorted, sp, labels, class_map, num_classes, v);
    return launch_status();
}

int ts_votes_labels(int32_t n, int32_t num_classes, const int64_t* votes, double min_share, uint8_t* labels_out,
                    float* confidence_out, void* stream) {
    if (n < 0 || num_classes < 1 || num_classes > TS_VOTE_MAX_CLASSES || !(min_share == min_share)) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!votes || !labels_out) return TS_E_BADARG;
    hipLaunchKernelGGL(votes_labels_kernel, dim3((unsigned)nblocks(n, kLabelThreads)), dim3(kLabelThreads), 0,
                       (hipStream_t)stream, n, num_classes, votes, min_share, labels_out, confidence_out);
    return launch_status();
}

}  // extern "C"
