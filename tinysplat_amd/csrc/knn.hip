// knn.hip - exact k-nearest neighbours on a hashed uniform grid, and the parameter initialisation of
// GaussianModel.from_pcd (tinysplat/splatting/model_gaussian.py:66-90) built on it.
//
// Reference: from_pcd sets every point's three log-scales to the log of the mean distance to its 3
// nearest other points, found by sklearn NearestNeighbors(n_neighbors=4) on the CPU (:76-81).  The
// same search with a general k <= 16 and general queries is what pytorch3d's knn_points does for the
// (still out of scope) SuGaR regulariser and mesh extraction.
//
// ts_knn, all on one stream, no host round trip:
//   init      hash keys := empty, cell counts := 0, bounding box := empty, counters := 0
//   bbox      min / max of points and queries (ordered-int atomicMin / atomicMax: order-free)
//   sample    S <= 64 evenly strided points: the exact distance to their 8th nearest other point
//             (the brute-force routine of the fallback below, each point's scan cut into 8 workgroups
//             whose partial lists params merges)
//   params    cell edge h = median of those distances: the density of OCCUPIED space (SfM clouds are
//             surfaces with far outliers; the box volume says nothing about them), at least
//             extent / (2^21 - 2) so that a cell coordinate fits 21 bits
//   insert    per point: cell -> open-addressing hash (capacity: power of two >= max(2n, 1024), linear probing,
//             atomicCAS on the 63-bit cell key) -> slot; rank within the cell = atomicAdd on its count
//   scan      exclusive scan of the per-slot counts (block sums, one-block scan of them, apply)
//   scatter   points counting-sorted by slot: float4 {x, y, z, original index}
//   query     one lane per query (the self-search walks the sorted points, so a wave's lanes share
//             cells; results go back to the caller's row): rings of cells around the query's cell,
//             a k-element list sorted by (distance, index) in registers; a cell whose box lies
//             beyond the current k-th distance is skipped, the search stops once the lower bound of
//             the next ring exceeds the k-th distance (or the rings cover the grid).  Queries still
//             open after kRings rings (far outliers) are appended to a compacted list
//   fallback  one workgroup per listed query scans all n points (grid-stride over the list)
//
// Exactness: distances are sqrt(dx*dx + dy*dy + dz*dz) in double (built with -ffp-contract=off) from
// the float32 coordinates, rounded to float32 only when written; the order is the total order on
// (double distance, index), so the output is one fixed function of the input whatever order the
// atomics ran in.  Every pruning bound is a lower bound on the distance minus a slack (1e-6 h plus
// 1e-13 of the largest coordinate) that covers the rounding of the cell assignment, and it prunes
// only when STRICTLY greater than the k-th distance (an equal distance with a smaller index still
// enters the list).  Rounding can cost one more ring, never a neighbour.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;                          // slots per thread in the scan passes
constexpr int kScanBlock = kThreads * kScanItems;      // 1024 slots per block
constexpr int kSamples = 64;                           // points whose 8th-neighbour distance sets h
constexpr int kSampleRank = 9;                         // the point itself + 8 others
constexpr int kSampleParts = 8;                        // workgroups per sampled point's scan
constexpr int kSampleEntries = kSamples * kSampleParts * kSampleRank;
constexpr int kRings = 5;                              // rings 0..4 (9^3 cells) before the fallback
constexpr int kCellBits = 21;
constexpr int kMaxDim = (1 << kCellBits) - 1;          // cells per axis
constexpr int kFallbackBlocks = 2048;
constexpr int kMaxPoints = 1 << 28;
constexpr unsigned long long kEmpty = ~0ull;           // never a key: keys use 63 bits
constexpr double kInf = __builtin_huge_val();

struct KnnHeader {
    int bbox[6];                  // ordered-int min x y z, max x y z
    int fallback_count;           // stats[0]
    int max_rings;                // stats[1]
    double lo[3];
    double h, inv_h, slack;
    int dim[3];
    int pad;
};

struct Workspace {
    KnnHeader* hdr;
    double* sample_d;             // partial lists of the sampled points: S x parts x kSampleRank
    int* sample_i;
    unsigned long long* keys;
    int* cnt;
    int* start;                   // cap + 1
    int* bsum;
    int2* slot_rank;
    float4* sorted;
    int* fallback;
    unsigned cap;
    int nb;
};

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

inline unsigned capacity(int n) {
    unsigned c = kScanBlock;
    while (c < 2u * (unsigned)n) c <<= 1;
    return c;
}

// the workspace carved in a fixed order; `total` is its size (ts_knn_ws_bytes)
struct Layout {
    size_t hdr, sample_d, sample_i, keys, cnt, start, bsum, slot_rank, sorted, fallback, total;
    unsigned cap;
    int nb;
    Layout(int n, int m) {
        cap = capacity(n);
        nb = (int)(cap / kScanBlock);
        size_t at = 0;
        hdr = at; at += align256(sizeof(KnnHeader));
        sample_d = at; at += align256(kSampleEntries * sizeof(double));
        sample_i = at; at += align256(kSampleEntries * sizeof(int));
        keys = at; at += align256((size_t)cap * sizeof(unsigned long long));
        cnt = at; at += align256((size_t)cap * sizeof(int));
        start = at; at += align256(((size_t)cap + 1) * sizeof(int));
        bsum = at; at += align256((size_t)nb * sizeof(int));
        slot_rank = at; at += align256((size_t)n * sizeof(int2));
        sorted = at; at += align256((size_t)n * sizeof(float4));
        fallback = at; at += align256((size_t)m * sizeof(int));
        total = at;
    }
    Workspace carve(void* base) const {
        char* b = (char*)base;
        Workspace w;
        w.hdr = (KnnHeader*)(b + hdr);
        w.sample_d = (double*)(b + sample_d);
        w.sample_i = (int*)(b + sample_i);
        w.keys = (unsigned long long*)(b + keys);
        w.cnt = (int*)(b + cnt);
        w.start = (int*)(b + start);
        w.bsum = (int*)(b + bsum);
        w.slot_rank = (int2*)(b + slot_rank);
        w.sorted = (float4*)(b + sorted);
        w.fallback = (int*)(b + fallback);
        w.cap = cap;
        w.nb = nb;
        return w;
    }
};

// ---------------------------------------------------------------------------------- k-element list
// Sorted ascending by (distance, index).  K slots (K >= k) are kept; only the first k are exact, the
// threshold of admission is slot k-1.
template <int K>
struct KList {
    double d[K];
    int i[K];
    double kth, kth2;             // slot k-1; kth^2 widened by 1e-12 for the squared-distance pre-test
    int kthi;

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < K; ++j) { d[j] = kInf; i[j] = INT_MAX; }
        kth = kInf; kth2 = kInf; kthi = INT_MAX;
    }
    __device__ __forceinline__ bool admits(double dd, int ii) const {
        return dd < kth || (dd == kth && ii < kthi);
    }
    __device__ __forceinline__ void push(double dd, int ii, int k) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool lt = dd < d[j] || (dd == d[j] && ii < i[j]);
            const double od = d[j];
            const int oi = i[j];
            d[j] = lt ? dd : od;
            i[j] = lt ? ii : oi;
            dd = lt ? od : dd;
            ii = lt ? oi : ii;
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j == k - 1) { kth = d[j]; kthi = i[j]; }
        kth2 = kth * kth * (1.0 + 1e-12);
    }
    // candidate point p (float32 coordinates) with index pi, query q in double
    __device__ __forceinline__ void consider(double qx, double qy, double qz, float px, float py, float pz,
                                             int pi, int k) {
        const double dx = qx - (double)px, dy = qy - (double)py, dz = qz - (double)pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 <= kth2)) return;                       // sqrt(d2) > kth for sure
        const double dd = sqrt(d2);
        if (admits(dd, pi)) push(dd, pi, k);
    }
    __device__ __forceinline__ void write(long long row, int k, float* __restrict__ dist,
                                          int* __restrict__ idx) const {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) {
                dist[row * k + j] = (float)d[j];
                idx[row * k + j] = i[j];
            }
    }
    __device__ __forceinline__ double at(int j) const {
        double r = kInf;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s == j) r = d[s];
        return r;
    }
};

// Brute force over the points [begin, end) by one 256-thread workgroup: every thread keeps a list of its
// strided share, then the lists are merged pairwise through LDS.  The result is in thread 0's list.
template <int K>
struct BruteLds {
    double d[K][kThreads / 2];
    int i[K][kThreads / 2];
};

template <int K>
__device__ void brute_block(int begin, int end, const float* __restrict__ pts, double qx, double qy, double qz,
                            int k, KList<K>& L, BruteLds<K>& s) {
    const int t = threadIdx.x;
    L.init();
#pragma unroll 1
    for (int p = begin + t; p < end; p += kThreads)
        L.consider(qx, qy, qz, pts[3ll * p], pts[3ll * p + 1], pts[3ll * p + 2], p, k);
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (t >= half && t < 2 * half) {
#pragma unroll
            for (int j = 0; j < K; ++j) { s.d[j][t - half] = L.d[j]; s.i[j][t - half] = L.i[j]; }
        }
        __syncthreads();
        if (t < half) {
#pragma unroll 1
            for (int j = 0; j < K; ++j) {
                const double dd = s.d[j][t];
                const int ii = s.i[j][t];
                if (L.admits(dd, ii)) L.push(dd, ii, k);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------ grid helpers
__device__ __forceinline__ int ordered(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float unordered(int b) { return __int_as_float(b >= 0 ? b : b ^ 0x7FFFFFFF); }

__device__ __forceinline__ int cell_of(double x, const KnnHeader& p, int a) {
    double t = (x - p.lo[a]) * p.inv_h;
    t = fmin(fmax(t, 0.0), (double)(p.dim[a] - 1));     // NaN -> 0; never outside the grid
    return (int)t;
}
__device__ __forceinline__ unsigned long long cell_key(int cx, int cy, int cz) {
    return (unsigned long long)cx | ((unsigned long long)cy << kCellBits) |
           ((unsigned long long)cz << (2 * kCellBits));
}
__device__ __forceinline__ unsigned hash_key(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}
// slot of key, or -1 when the cell holds no point
__device__ __forceinline__ int lookup(const unsigned long long* __restrict__ keys, unsigned cap,
                                      unsigned long long key) {
    unsigned s = hash_key(key) & (cap - 1);
    for (unsigned t = 0; t < cap; ++t) {
        const unsigned long long k = keys[s];
        if (k == key) return (int)s;
        if (k == kEmpty) return -1;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    __shared__ int wave_sum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) base += wave_sum[w];
        all += wave_sum[w];
    }
    *total = all;
    __syncthreads();
    return base + inc - v;
}

// ----------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kThreads) void init_kernel(Workspace w) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s < w.cap; s += stride) {
        w.keys[s] = kEmpty;
        w.cnt[s] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) w.hdr->bbox[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
    if (blockIdx.x == 0 && threadIdx.x == 6) { w.hdr->fallback_count = 0; w.hdr->max_rings = 0; }
}

__global__ __launch_bounds__(kThreads) void bbox_kernel(int n, const float* __restrict__ pts, int m,
                                                        const float* __restrict__ qs, KnnHeader* hdr) {
    __shared__ int red[6][kThreads / 64];
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
    const long long total = (long long)n + (qs ? m : 0);
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
        const float* p = e < n ? pts + 3 * e : qs + 3 * (e - n);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int o = ordered(p[a]);
            mn[a] = min(mn[a], o);
            mx[a] = max(mx[a], o);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo = mn[a], hi = mx[a];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d));
            hi = max(hi, __shfl_xor(hi, d));
        }
        if (lane == 0) { red[a][wave] = lo; red[3 + a][wave] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        int v = red[a][0];
        for (int w = 1; w < kThreads / 64; ++w) v = a < 3 ? min(v, red[a][w]) : max(v, red[a][w]);
        if (a < 3) atomicMin(&hdr->bbox[a], v);
        else atomicMax(&hdr->bbox[a], v);
    }
}

// S evenly strided points x kSampleParts slices of the points: the k = min(9, n) nearest of each slice
// (unused entries +inf); params_kernel merges a point's slices
__global__ __launch_bounds__(kThreads) void sample_kernel(int n, const float* __restrict__ pts, int S,
                                                          double* __restrict__ sample_d, int* __restrict__ sample_i) {
    __shared__ BruteLds<16> lds;
    const int s = blockIdx.x / kSampleParts, part = blockIdx.x % kSampleParts;
    const long long p = (long long)s * n / S;
    const int begin = (int)((long long)part * n / kSampleParts), end = (int)((long long)(part + 1) * n / kSampleParts);
    const int k = min(kSampleRank, n);
    KList<16> L;
    brute_block<16>(begin, end, pts, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], k, L, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kSampleRank; ++j) {
            sample_d[blockIdx.x * kSampleRank + j] = L.d[j];
            sample_i[blockIdx.x * kSampleRank + j] = L.i[j];
        }
    }
}

__global__ __launch_bounds__(64) void params_kernel(int n, int S, const double* __restrict__ sample_d,
                                                    const int* __restrict__ sample_i, KnnHeader* hdr) {
    __shared__ double med;
    __shared__ double sample[kSamples];
    const int t = threadIdx.x;
    if (t == 0) med = 0.0;
    if (t < S) {                                   // merge the sampled point's slices: its k-th distance
        const int k = min(kSampleRank, n);
        KList<16> L;
        L.init();
        for (int e = t * kSampleParts * kSampleRank; e < (t + 1) * kSampleParts * kSampleRank; ++e)
            if (L.admits(sample_d[e], sample_i[e])) L.push(sample_d[e], sample_i[e], k);
        sample[t] = L.at(k - 1);
    }
    __syncthreads();
    if (t < S) {
        const double v = sample[t];
        int rank = 0;
        for (int j = 0; j < S; ++j) {
            const double u = sample[j];
            rank += (u < v || (u == v && j < t)) ? 1 : 0;
        }
        if (rank == S / 2) med = v;
    }
    __syncthreads();
    if (t != 0) return;
    double lo[3], hi[3], ext = 0.0, big = 0.0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)unordered(hdr->bbox[a]);
        hi[a] = (double)unordered(hdr->bbox[3 + a]);
        ext = fmax(ext, hi[a] - lo[a]);
        big = fmax(big, fmax(fabs(lo[a]), fabs(hi[a])));
    }
    double h = med;
    if (!(h > 0.0) || !(h < kInf)) h = ext / cbrt((double)n);         // mostly duplicates: box density
    if (!(h > 0.0) || !(h < kInf)) h = 1.0;                           // a single location
    h = fmax(h, ext / (double)(kMaxDim - 1));
    const double inv_h = 1.0 / h;
    for (int a = 0; a < 3; ++a) {
        hdr->lo[a] = lo[a];
        const double c = floor((hi[a] - lo[a]) * inv_h) + 1.0;
        hdr->dim[a] = (int)fmin(fmax(c, 1.0), (double)kMaxDim);
    }
    hdr->h = h;
    hdr->inv_h = inv_h;
    hdr->slack = 1e-6 * h + 1e-13 * big;
}

__global__ __launch_bounds__(kThreads) void insert_kernel(int n, const float* __restrict__ pts, Workspace w) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const KnnHeader p = *w.hdr;
    const unsigned long long key = cell_key(cell_of(pts[3ll * i], p, 0), cell_of(pts[3ll * i + 1], p, 1),
                                            cell_of(pts[3ll * i + 2], p, 2));
    unsigned s = hash_key(key) & (w.cap - 1);
    for (unsigned t = 0; t < w.cap; ++t) {                // cap >= 2n > cells: always finds a slot
        const unsigned long long prev = atomicCAS(&w.keys[s], kEmpty, key);
        if (prev == kEmpty || prev == key) break;
        s = (s + 1) & (w.cap - 1);
    }
    const int rank = atomicAdd(&w.cnt[s], 1);
    w.slot_rank[i] = make_int2((int)s, rank);
}

__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(Workspace w) {
    const long long first = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) v += w.cnt[first + j];
    int total;
    block_exclusive_scan(v, &total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// one block: block sums -> exclusive bases in place
__global__ __launch_bounds__(kThreads) void scan_top_kernel(Workspace w) {
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < w.nb; b0 += kThreads) {
        const int b = b0 + threadIdx.x;
        const int v = b < w.nb ? w.bsum[b] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        const int base = carry;
        if (b < w.nb) w.bsum[b] = base + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry = base + total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(int n, Workspace w) {
    const long long first = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int c[kScanItems], v = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) { c[j] = w.cnt[first + j]; v += c[j]; }
    int total;
    int at = w.bsum[blockIdx.x] + block_exclusive_scan(v, &total);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) { w.start[first + j] = at; at += c[j]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) w.start[w.cap] = n;
}

__global__ __launch_bounds__(kThreads) void scatter_kernel(int n, const float* __restrict__ pts, Workspace w) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int2 sr = w.slot_rank[i];
    w.sorted[w.start[sr.x] + sr.y] = make_float4(pts[3ll * i], pts[3ll * i + 1], pts[3ll * i + 2], __int_as_float(i));
}

// qs == nullptr: the self-search, query j is the j-th point in cell order
template <int K>
__global__ __launch_bounds__(kThreads) void query_kernel(int m, const float* __restrict__ qs, int k, Workspace w,
                                                         float* __restrict__ dist, int* __restrict__ idx) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    int rings = 0;
    if (j < m) {
        const KnnHeader p = *w.hdr;
        double q[3];
        int row;
        if (qs) {
            q[0] = qs[3ll * j]; q[1] = qs[3ll * j + 1]; q[2] = qs[3ll * j + 2];
            row = j;
        } else {
            const float4 s = w.sorted[j];
            q[0] = s.x; q[1] = s.y; q[2] = s.z;
            row = __float_as_int(s.w);
        }
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = cell_of(q[a], p, a);
        KList<K> L;
        L.init();
        bool done = false;
        for (int r = 0; r < kRings && !done; ++r) {
            for (int dz = -r; dz <= r; ++dz) {
                const int cz = c[2] + dz;
                if (cz < 0 || cz >= p.dim[2]) continue;
                for (int dy = -r; dy <= r; ++dy) {
                    const int cy = c[1] + dy;
                    if (cy < 0 || cy >= p.dim[1]) continue;
                    const int step = (dz == -r || dz == r || dy == -r || dy == r) ? 1 : 2 * r;
                    for (int dx = -r; dx <= r; dx += step) {
                        const int cx = c[0] + dx;
                        if (cx < 0 || cx >= p.dim[0]) continue;
                        // the cell's box (widened by the slack) lies beyond the k-th distance: skip
                        const int cc[3] = {cx, cy, cz};
                        double g2 = 0.0;
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const double blo = p.lo[a] + (double)cc[a] * p.h - p.slack;
                            const double bhi = p.lo[a] + (double)(cc[a] + 1) * p.h + p.slack;
                            const double g = fmax(fmax(blo - q[a], q[a] - bhi), 0.0);
                            g2 += g * g;
                        }
                        if (g2 > L.kth2) continue;
                        const int s = lookup(w.keys, w.cap, cell_key(cx, cy, cz));
                        if (s < 0) continue;
                        const int e = w.start[s + 1];
                        for (int t = w.start[s]; t < e; ++t) {
                            const float4 pt = w.sorted[t];
                            L.consider(q[0], q[1], q[2], pt.x, pt.y, pt.z, __float_as_int(pt.w), k);
                        }
                    }
                }
            }
            rings = r + 1;
            // lower bound on the distance to any point outside rings 0..r: the nearest face of the
            // ring-r cube that has cells beyond it (none left: every cell has been seen)
            double bound = kInf;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (c[a] - r > 0) bound = fmin(bound, q[a] - (p.lo[a] + (double)(c[a] - r) * p.h));
                if (c[a] + r + 1 < p.dim[a]) bound = fmin(bound, (p.lo[a] + (double)(c[a] + r + 1) * p.h) - q[a]);
            }
            done = bound == kInf || L.kth < bound - p.slack;
        }
        if (done) {
            L.write(row, k, dist, idx);
        } else {
            const int at = atomicAdd(&w.hdr->fallback_count, 1);       // < m: each query at most once
            w.fallback[at] = row;
        }
    }
    rings = wave_max(rings);
    if ((threadIdx.x & 63) == 0 && rings > 0) atomicMax(&w.hdr->max_rings, rings);
}

template <int K>
__global__ __launch_bounds__(kThreads) void fallback_kernel(int n, const float* __restrict__ pts, int m,
                                                            const float* __restrict__ qs, int k, Workspace w,
                                                            float* __restrict__ dist, int* __restrict__ idx) {
    __shared__ BruteLds<K> lds;
    const int count = min(w.hdr->fallback_count, m);
    const float* src = qs ? qs : pts;
    for (int e = blockIdx.x; e < count; e += gridDim.x) {
        const int row = w.fallback[e];
        KList<K> L;
        brute_block<K>(0, n, pts, src[3ll * row], src[3ll * row + 1], src[3ll * row + 2], k, L, lds);
        if (threadIdx.x == 0) L.write(row, k, dist, idx);
    }
}

template <int K>
int run_queries(int32_t n, const float* points, int32_t m, const float* qs, int32_t k, const Workspace& w,
                float* dist, int32_t* idx, hipStream_t s) {
    query_kernel<K><<<(m + kThreads - 1) / kThreads, kThreads, 0, s>>>(m, qs, k, w, dist, idx);
    fallback_kernel<K><<<min(m, kFallbackBlocks), kThreads, 0, s>>>(n, points, m, qs, k, w, dist, idx);
    return launch_status();
}

// ------------------------------------------------------------------------------- from_pcd init
__global__ __launch_bounds__(kThreads) void init_points_kernel(int n, int k_rest, const float* __restrict__ xyz,
                                                               const float* __restrict__ colors,
                                                               const float* __restrict__ u,
                                                               const float* __restrict__ v,
                                                               const float* __restrict__ w,
                                                               const int* __restrict__ knn_idx,
                                                               float* __restrict__ means, float* __restrict__ dc,
                                                               float* __restrict__ rest, float* __restrict__ scales,
                                                               float* __restrict__ quats, float* __restrict__ opac,
                                                               float* __restrict__ mean_dist) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float C0 = 0.28209479177387814f;
    const double qx = xyz[3ll * i], qy = xyz[3ll * i + 1], qz = xyz[3ll * i + 2];
    for (int a = 0; a < 3; ++a) {
        means[3ll * i + a] = xyz[3ll * i + a];
        dc[3ll * i + a] = (colors[3ll * i + a] / 255.0f - 0.5f) / C0;           // RGB2SH(colors / 255)
    }
    for (int e = 0; e < 3 * k_rest; ++e) rest[3ll * k_rest * i + e] = 0.0f;
    // np.mean(distances[:, 1:], axis=1) in double, then float32 (model_gaussian.py:80)
    double sum = 0.0;
    for (int j = 1; j < 4; ++j) {
        const int pj = min(max(knn_idx[4ll * i + j], 0), n - 1);
        const double dx = qx - (double)xyz[3ll * pj], dy = qy - (double)xyz[3ll * pj + 1],
                     dz = qz - (double)xyz[3ll * pj + 2];
        sum += sqrt(dx * dx + dy * dy + dz * dz);
    }
    const float md = (float)(sum / 3.0);
    // log in double, rounded once: within 1 ulp of numpy's float32 log; log(0) = -inf, as np.log
    const float ls = (float)log((double)md);
    for (int a = 0; a < 3; ++a) scales[3ll * i + a] = ls;
    if (mean_dist) mean_dist[i] = md;
    // random_quat_tensor (utils.py:15-27): 2 * math.pi * v is a float32 product with 2 pi rounded to float32
    const float two_pi = 6.283185307179586f;
    const float su = sqrtf(1.0f - u[i]), sv = sqrtf(u[i]);
    const float tv = two_pi * v[i], tw = two_pi * w[i];
    quats[4ll * i] = su * sinf(tv);
    quats[4ll * i + 1] = su * cosf(tv);
    quats[4ll * i + 2] = sv * sinf(tw);
    quats[4ll * i + 3] = sv * cosf(tw);
    const float o = 0.1f;
    opac[i] = logf(o / (1.0f - o));                                             // torch.logit(0.1)
}

}  // namespace

extern "C" {

int64_t ts_knn_ws_bytes(int32_t n, int32_t m, int32_t k) {
    if (n < 1 || n > kMaxPoints || m < 0 || k < 1 || k > TS_KNN_MAX_K || k > n) return TS_E_BADARG;
    return (int64_t)Layout(n, m).total;
}

int ts_knn(int32_t n, const float* points, int32_t m, const float* queries, int32_t k, float* dist, int32_t* idx,
           void* ws, int32_t* stats, void* stream) {
    if (n < 1 || n > kMaxPoints || m < 0 || k < 1 || k > TS_KNN_MAX_K || k > n) return TS_E_BADARG;
    if (!points || !ws || (m > 0 && (!queries || !dist || !idx))) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const Layout lay(n, m);
    const Workspace w = lay.carve(ws);
    const bool self = queries == points && m == n;
    const float* qs = self ? nullptr : queries;
    const int S = min(n, kSamples);
    init_kernel<<<(int)(w.cap / kThreads < 2048u ? w.cap / kThreads : 2048u), kThreads, 0, s>>>(w);
    const long long extent = (long long)n + (qs ? m : 0);
    bbox_kernel<<<(int)((extent + kThreads - 1) / kThreads < 1024 ? (extent + kThreads - 1) / kThreads : 1024), kThreads, 0, s>>>(n, points, m, qs,
                                                                                                  w.hdr);
    sample_kernel<<<S * kSampleParts, kThreads, 0, s>>>(n, points, S, w.sample_d, w.sample_i);
    params_kernel<<<1, 64, 0, s>>>(n, S, w.sample_d, w.sample_i, w.hdr);
    insert_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(n, points, w);
    scan_reduce_kernel<<<w.nb, kThreads, 0, s>>>(w);
    scan_top_kernel<<<1, kThreads, 0, s>>>(w);
    scan_apply_kernel<<<w.nb, kThreads, 0, s>>>(n, w);
    scatter_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(n, points, w);
    int code = launch_status();
    if (code) return code;
    if (m > 0) {
        code = k <= 4 ? run_queries<4>(n, points, m, qs, k, w, dist, idx, s)
             : k <= 8 ? run_queries<8>(n, points, m, qs, k, w, dist, idx, s)
                      : run_queries<16>(n, points, m, qs, k, w, dist, idx, s);
        if (code) return code;
    }
    if (stats) {
        const hipError_t e = hipMemcpyAsync(stats, &w.hdr->fallback_count, 2 * sizeof(int32_t),
                                            hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

int ts_init_from_points(int32_t n, int32_t k_rest, const float* xyz, const float* colors, const float* u,
                        const float* v, const float* w, const int32_t* knn_idx, float* means, float* colors_dc,
                        float* colors_rest, float* scales, float* quats, float* opacities, float* mean_dist,
                        void* stream) {
    if (n < 4 || k_rest < 0) return TS_E_BADARG;
    if (!xyz || !colors || !u || !v || !w || !knn_idx || !means || !colors_dc || !scales || !quats || !opacities ||
        (k_rest > 0 && !colors_rest))
        return TS_E_BADARG;
    init_points_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, (hipStream_t)stream>>>(
        n, k_rest, xyz, colors, u, v, w, knn_idx, means, colors_dc, colors_rest, scales, quats, opacities, mean_dist);
    return launch_status();
}

}  // extern "C"
