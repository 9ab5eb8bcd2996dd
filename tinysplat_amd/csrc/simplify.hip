// simplify.hip - triangle-budget simplification of a mesh by vertex clustering with quadric-optimal representatives
// (the arithmetic lives in simplify_math.h, shared with the host tests).
//
//   count       one thread per face: the keys of its three corners at the probed grid; a face survives when they are
//               pairwise distinct.  Ballot + popcount per wave, the four wave totals through LDS, one plain int32 store
//               per workgroup; torch sums the workgroup counts.  One launch per probe of the budget search.
//   keys        one thread per vertex: its int64 cell key.
//   accumulate  the face corners (or the vertices) stably sorted by cluster.  One thread sums a chunk of 128 consecutive
//               sorted entries serially in double, recomputing each entry's numbers from the face (36 bytes of gathers)
//               instead of reading materialised rows.  A run of one cluster that lies inside a chunk is stored at once; a
//               run that crosses chunk ends is finished by the chunk it starts in, which adds the later chunks' leading
//               partial sums in chunk order (the scheme of ts_segment_sum).  The order of additions is a function of
//               the sorted list alone: a call may cover any range of chunks (its workspace holds two partial rows and a
//               flag per chunk of the range), and where a run leaves the range the finishing thread recomputes the later
//               chunks' leading sums itself, in the same order.  Plain stores, no atomics.
//   solve       one thread per cluster: ts_simplify_representative, 12 bytes out.
//   faces       one thread per face: the corners' clusters, rotated so that the smallest comes first, and a keep flag
//               (no two corners in one cluster).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "simplify_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = TS_SIMPLIFY_CHUNK;
constexpr int kOwn = 1;      // the chunk's last run continues into the next chunk and is finished from here
constexpr int kThrough = 2;  // the chunk is one run that came from the previous chunk and continues

struct Grid {
    float lo[3];
    float c;
    int32_t n[3];
};

__device__ __forceinline__ void load3(const float* __restrict__ vertices, int64_t i, float p[3]) {
    p[0] = vertices[i * 3];
    p[1] = vertices[i * 3 + 1];
    p[2] = vertices[i * 3 + 2];
}

__global__ __launch_bounds__(kThreads) void count_kernel(int32_t f, Grid g, const float* __restrict__ vertices,
                                                         const int32_t* __restrict__ faces,
                                                         int32_t* __restrict__ block_counts) {
    __shared__ int wave_total[kThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool keep = false;
    if (i < f) {
        float p[3];
        load3(vertices, faces[i * 3], p);
        const int64_t k0 = ts_simplify_key(p, g.lo, g.c, g.n);
        load3(vertices, faces[i * 3 + 1], p);
        const int64_t k1 = ts_simplify_key(p, g.lo, g.c, g.n);
        load3(vertices, faces[i * 3 + 2], p);
        const int64_t k2 = ts_simplify_key(p, g.lo, g.c, g.n);
        keep = k0 != k1 && k1 != k2 && k0 != k2;
    }
    const int total = __popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) sum += wave_total[w];
        block_counts[blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(kThreads) void keys_kernel(int32_t v, Grid g, const float* __restrict__ vertices,
                                                        int64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= v) return;
    float p[3];
    load3(vertices, i, p);
    keys[i] = ts_simplify_key(p, g.lo, g.c, g.n);
}

__device__ __forceinline__ void cell_centre(const Grid& g, const float p[3], double c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = ts_simplify_centre(g.lo[a], g.c, ts_simplify_cell(p[a], g.lo[a], g.c, g.n[a]));
}

// entry e = face * 3 + corner: the face's plane against the centre of the corner's cell
struct FaceTerm {
    static constexpr int D = TS_SIMPLIFY_QUADRIC;
    const float* __restrict__ vertices;
    const int32_t* __restrict__ faces;
    Grid g;
    __device__ __forceinline__ void operator()(int64_t e, double q[D]) const {
        const int64_t face = e / 3;
        const int corner = (int)(e - face * 3);
        const int32_t ia = faces[face * 3], ib = faces[face * 3 + 1], ic = faces[face * 3 + 2];
        float a[3], b[3], c[3];
        load3(vertices, ia, a);
        load3(vertices, ib, b);
        load3(vertices, ic, c);
        double centre[3];
        cell_centre(g, corner == 0 ? a : corner == 1 ? b : c, centre);
        ts_simplify_face_term(a, b, c, centre, q);
    }
};

// entry e = a vertex: its offset from the centre of its cell, and one for the count
struct VertexTerm {
    static constexpr int D = TS_SIMPLIFY_VSUM;
    const float* __restrict__ vertices;
    Grid g;
    __device__ __forceinline__ void operator()(int64_t e, double q[D]) const {
        float p[3];
        load3(vertices, e, p);
        double centre[3];
        cell_centre(g, p, centre);
        for (int a = 0; a < 3; ++a) q[a] = (double)p[a] - centre[a];
        q[3] = 1.0;
    }
};

// chunks [chunk0, chunk0 + chunks) of the T sorted entries; head, tail and flags are indexed by chunk - chunk0
template <class Term>
__global__ __launch_bounds__(kThreads) void accumulate_local_kernel(int64_t T, int64_t chunk0, int64_t chunks,
                                                                    int32_t clusters, Term term,
                                                                    const int32_t* __restrict__ keys,
                                                                    const int64_t* __restrict__ order,
                                                                    double* __restrict__ out, double* __restrict__ head,
                                                                    double* __restrict__ tail,
                                                                    int32_t* __restrict__ flags) {
    constexpr int D = Term::D;
    const int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (w >= chunks) return;
    const int64_t c = chunk0 + w;
    const int64_t i0 = c * kChunk, i1 = (i0 + kChunk < T) ? i0 + kChunk : T;
    const int32_t key_before = c > 0 ? keys[i0 - 1] : -1;
    const int32_t key_after = i1 < T ? keys[i1] : -1;
    int fl = 0;
    double acc[D], q[D];
    int32_t cur = keys[i0];
    bool first = true;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.0;
    for (int64_t i = i0; i <= i1; ++i) {
        const bool end = i == i1;
        const int32_t key = end ? -2 : keys[i];
        if (end || key != cur) {
            // the run of `cur` inside this chunk is complete
            const bool cin = first && cur == key_before;
            const bool cout = end && cur == key_after;
            if (cur >= 0 && cur < clusters) {
                if (!cin && !cout) {
#pragma unroll
                    for (int d = 0; d < D; ++d) out[(int64_t)cur * D + d] = acc[d];
                } else if (cin) {
#pragma unroll
                    for (int d = 0; d < D; ++d) head[w * D + d] = acc[d];
                    if (cout) fl |= kThrough;
                } else {
#pragma unroll
                    for (int d = 0; d < D; ++d) tail[w * D + d] = acc[d];
                    fl |= kOwn;
                }
            }
            if (end) break;
            cur = key;
            first = false;
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] = 0.0;
        }
        term(order[i], q);
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] += q[d];
    }
    flags[w] = fl;
}

template <class Term>
__global__ __launch_bounds__(kThreads) void accumulate_join_kernel(int64_t T, int64_t chunk0, int64_t chunks, Term term,
                                                                   const int32_t* __restrict__ keys,
                                                                   const int64_t* __restrict__ order,
                                                                   double* __restrict__ out,
                                                                   const double* __restrict__ head,
                                                                   const double* __restrict__ tail,
                                                                   const int32_t* __restrict__ flags) {
    constexpr int D = Term::D;
    const int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (w >= chunks || !(flags[w] & kOwn)) return;
    const int64_t nchunks = (T + kChunk - 1) / kChunk;
    const int64_t c = chunk0 + w;
    const int32_t key = keys[(c + 1) * kChunk - 1];         // (c + 1) * kChunk < T: the run continues into chunk c + 1
    double acc[D], q[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = tail[w * D + d];
    for (int64_t c2 = c + 1; c2 < nchunks; ++c2) {
        if (c2 < chunk0 + chunks) {
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += head[(c2 - chunk0) * D + d];
            if (!(flags[c2 - chunk0] & kThrough)) break;
        } else {
            // beyond this call's range: the leading sum of chunk c2 as its own thread forms it, from zero, in order
            const int64_t i0 = c2 * kChunk, i1 = (i0 + kChunk < T) ? i0 + kChunk : T;
            double h[D];
#pragma unroll
            for (int d = 0; d < D; ++d) h[d] = 0.0;
            int64_t i = i0;
            for (; i < i1 && keys[i] == key; ++i) {
                term(order[i], q);
#pragma unroll
                for (int d = 0; d < D; ++d) h[d] += q[d];
            }
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += h[d];
            if (i < i1 || i1 >= T || keys[i1] != key) break;
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) out[(int64_t)key * D + d] = acc[d];
}

__global__ __launch_bounds__(kThreads) void solve_kernel(int32_t clusters, Grid g, double tau,
                                                         const int64_t* __restrict__ cluster_keys,
                                                         const double* __restrict__ quadrics,
                                                         const double* __restrict__ vsums,
                                                         float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= clusters) return;
    double q[TS_SIMPLIFY_QUADRIC], s[TS_SIMPLIFY_VSUM], x[3];
#pragma unroll
    for (int d = 0; d < TS_SIMPLIFY_QUADRIC; ++d) q[d] = quadrics[i * TS_SIMPLIFY_QUADRIC + d];
#pragma unroll
    for (int d = 0; d < TS_SIMPLIFY_VSUM; ++d) s[d] = vsums[i * TS_SIMPLIFY_VSUM + d];
    ts_simplify_representative(q, s, (double)g.c, tau, x);
    const int64_t key = cluster_keys[i];
    const int32_t ix = (int32_t)(key % g.n[0]), iy = (int32_t)((key / g.n[0]) % g.n[1]);
    const int32_t iz = (int32_t)(key / ((int64_t)g.n[0] * g.n[1]));
    out[i * 3] = (float)(ts_simplify_centre(g.lo[0], g.c, ix) + x[0]);
    out[i * 3 + 1] = (float)(ts_simplify_centre(g.lo[1], g.c, iy) + x[1]);
    out[i * 3 + 2] = (float)(ts_simplify_centre(g.lo[2], g.c, iz) + x[2]);
}

__global__ __launch_bounds__(kThreads) void faces_kernel(int32_t f, const int32_t* __restrict__ faces,
                                                         const int32_t* __restrict__ vertex_cluster,
                                                         int32_t* __restrict__ out, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    const int32_t a = vertex_cluster[faces[i * 3]], b = vertex_cluster[faces[i * 3 + 1]];
    const int32_t c = vertex_cluster[faces[i * 3 + 2]];
    int32_t r0 = a, r1 = b, r2 = c;                     // the rotation that starts at the smallest
    if (b < a && b <= c) {
        r0 = b; r1 = c; r2 = a;
    } else if (c < a && c < b) {
        r0 = c; r1 = a; r2 = b;
    }
    out[i * 3] = r0;
    out[i * 3 + 1] = r1;
    out[i * 3 + 2] = r2;
    keep[i] = (a != b && b != c && a != c) ? 1 : 0;
}

// host float[4] {lo, c} and int32[3] cells per axis -> Grid; false for anything a kernel must not see
bool read_grid(const float* grid_host, const int32_t* cells_host, Grid* g) {
    if (!grid_host || !cells_host) return false;
    for (int k = 0; k < 4; ++k)
        if (!isfinite(grid_host[k])) return false;
    if (!(grid_host[3] > 0.f)) return false;
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        if (cells_host[a] < 1) return false;
        cells *= (double)cells_host[a];
    }
    if (cells >= 4.6e18) return false;                  // the key must fit int64
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = grid_host[a];
        g->n[a] = cells_host[a];
    }
    g->c = grid_host[3];
    return true;
}

template <class Term>
void accumulate(int64_t T, int64_t chunk0, int64_t chunks, int32_t clusters, const Term& term, const int32_t* keys,
                const int64_t* order, double* sums, void* ws, hipStream_t s) {
    double* head = (double*)ws;
    double* tail = (double*)((char*)ws + align256(chunks * Term::D * 8));
    int32_t* flags = (int32_t*)((char*)ws + 2 * align256(chunks * Term::D * 8));
    const dim3 grid((unsigned)nblocks(chunks, kThreads));
    hipLaunchKernelGGL(accumulate_local_kernel<Term>, grid, dim3(kThreads), 0, s, T, chunk0, chunks, clusters, term, keys,
                       order, sums, head, tail, flags);
    hipLaunchKernelGGL(accumulate_join_kernel<Term>, grid, dim3(kThreads), 0, s, T, chunk0, chunks, term, keys, order,
                       sums, (const double*)head, (const double*)tail, (const int32_t*)flags);
}

}  // namespace

extern "C" {

int ts_simplify_count(int32_t v, int32_t f, const float* vertices, const int32_t* faces, const float* grid_host,
                      const int32_t* cells_host, int32_t* block_counts, void* stream) {
    Grid g;
    if (v < 0 || f < 0 || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (f == 0) return 0;
    if (v < 1 || !vertices || !faces || !block_counts) return TS_E_BADARG;
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)nblocks(f, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, f, g,
                       vertices, faces, block_counts);
    return launch_status();
}

int ts_simplify_keys(int32_t v, const float* vertices, const float* grid_host, const int32_t* cells_host, int64_t* keys,
                     void* stream) {
    Grid g;
    if (v < 0 || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (v == 0) return 0;
    if (!vertices || !keys) return TS_E_BADARG;
    hipLaunchKernelGGL(keys_kernel, dim3((unsigned)nblocks(v, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, v, g,
                       vertices, keys);
    return launch_status();
}

int64_t ts_simplify_ws_bytes(int64_t chunks) {
    if (chunks < 1 || chunks > ((int64_t)1 << 40)) return TS_E_BADARG;
    return 2 * align256(chunks * TS_SIMPLIFY_QUADRIC * 8) + align256(chunks * 4);
}

int ts_simplify_accumulate(int32_t v, int32_t f, int32_t clusters, const float* vertices, const int32_t* faces,
                           const float* grid_host, const int32_t* cells_host, int32_t what, int64_t entries,
                           const int32_t* clusters_sorted, const int64_t* order, int64_t chunk0, int64_t chunks,
                           double* sums, void* ws, void* stream) {
    Grid g;
    if (v < 0 || f < 0 || clusters < 0 || entries < 0 || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (what != TS_SIMPLIFY_FACE_CORNERS && what != TS_SIMPLIFY_VERTICES) return TS_E_BADARG;
    if (entries != (what == TS_SIMPLIFY_FACE_CORNERS ? (int64_t)f * 3 : (int64_t)v)) return TS_E_BADARG;
    const int64_t nchunks = (entries + kChunk - 1) / kChunk;
    if (chunk0 < 0 || chunks < 0 || chunk0 > nchunks || chunks > nchunks - chunk0) return TS_E_BADARG;
    if (entries == 0 || chunks == 0) return 0;
    if (v < 1 || clusters < 1 || !vertices || !clusters_sorted || !order || !sums || !ws) return TS_E_BADARG;
    if (what == TS_SIMPLIFY_FACE_CORNERS) {
        if (!faces) return TS_E_BADARG;
        accumulate(entries, chunk0, chunks, clusters, FaceTerm{vertices, faces, g}, clusters_sorted, order, sums, ws,
                   (hipStream_t)stream);
    } else {
        accumulate(entries, chunk0, chunks, clusters, VertexTerm{vertices, g}, clusters_sorted, order, sums, ws,
                   (hipStream_t)stream);
    }
    return launch_status();
}

int ts_simplify_solve(int32_t clusters, const int64_t* cluster_keys, const float* grid_host, const int32_t* cells_host,
                      const double* quadrics, const double* vertex_sums, double singular_threshold,
                      float* representatives, void* stream) {
    Grid g;
    if (clusters < 0 || !read_grid(grid_host, cells_host, &g)) return TS_E_BADARG;
    if (!(singular_threshold > 0.0 && singular_threshold < 1.0)) return TS_E_BADARG;
    if (clusters == 0) return 0;
    if (!cluster_keys || !quadrics || !vertex_sums || !representatives) return TS_E_BADARG;
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned)nblocks(clusters, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       clusters, g, singular_threshold, cluster_keys, quadrics, vertex_sums, representatives);
    return launch_status();
}

int ts_simplify_faces(int32_t v, int32_t f, const int32_t* faces, const int32_t* vertex_cluster, int32_t* out_faces,
                      uint8_t* keep, void* stream) {
    if (v < 0 || f < 0) return TS_E_BADARG;
    if (f == 0) return 0;
    if (v < 1 || !faces || !vertex_cluster || !out_faces || !keep) return TS_E_BADARG;
    hipLaunchKernelGGL(faces_kernel, dim3((unsigned)nblocks(f, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, f,
                       faces, vertex_cluster, out_faces, keep);
    return launch_status();
}

}  // extern "C"
