// clean.hip - mesh clean-up: the faces at edges of valence above two, and the connected components (DESIGN.md section
// 6j; the arithmetic lives in clean_math.h, shared with the host tests).  Integer work throughout: the results are a
// fixed function of the mesh, bit-identical from run to run.
//
//   degenerate  one thread per face: 1 where two of its indices are equal.
//   edge_keys   one thread per face: the int64 keys of its three undirected edges, entry 3 face + k.
//   weights     one thread per face: A2, four times its squared area in double.
//   mark        one thread per entry of the edge list sorted by (key, A2 descending, face): entry i shares its key with
//               entry i - 2 exactly when at least two faces of its edge rank before it; its face is marked with a plain
//               byte store of 1 (several threads may store the same 1).
//   components  union-find over the vertices in the style of ECL-CC (Jaiganesh and Burtscher, HPDC 2018).  parent starts
//               as the identity; one thread per face joins the roots of (a, b) and of (b, c); a last launch writes every
//               vertex's root (a plain walk without shortcuts: its cost follows the depth the joins left).  The kernel
//               rests on two invariants:
//                 1. parent[x] <= x at all times, and x and parent[x] lie in one component of the mesh.  Every store
//                    keeps it: a link stores the smaller of two roots onto the larger, a shortcut stores an ancestor's
//                    ancestor.
//                    A walk x -> parent[x] therefore strictly descends and ends within V steps whatever it reads,
//                    including a value that another XCD's L2 has since replaced: any value parent[x] ever held is below
//                    x and in x's component, and trees only ever merge.
//                 2. A join loops only on a failed compare-and-swap, and every retry strictly lowers the larger of its
//                    two roots (the swap returns what the word held, which is below the root it was tried on).  Both are
//                    non-negative integers, so a join ends; no thread ever waits for another.
//               A link succeeds only on a true root (the compare-and-swap is done at memory, agent scope), so no link is
//               lost, and when all joins have returned every face's vertices share a root.  A root is the smallest index
//               of its tree (invariant 1), so the labels are the components' minima whatever the interleaving was.
//               parent is read with relaxed agent-scope atomic loads and written with relaxed agent-scope atomic stores
//               (they bypass the CU's L1, which no other CU's store refreshes); integer vector atomics only, no fences,
//               no spin-waits.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "clean_math.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void degenerate_kernel(int32_t f, const int32_t* __restrict__ faces,
                                                              uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    const int32_t a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    flags[i] = (a == b || b == c || a == c) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void edge_keys_kernel(int32_t v, int32_t f, const int32_t* __restrict__ faces,
                                                             int64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    const int32_t a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    keys[i * 3] = ts_clean_edge_key(a, b, v);
    keys[i * 3 + 1] = ts_clean_edge_key(b, c, v);
    keys[i * 3 + 2] = ts_clean_edge_key(c, a, v);
}

__global__ __launch_bounds__(kThreads) void weights_kernel(int32_t v, int32_t f, const float* __restrict__ vertices,
                                                           const int32_t* __restrict__ faces,
                                                           double* __restrict__ weights) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    float p[3][3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t at = faces[i * 3 + k];
        inside = inside && at >= 0 && at < v;
        const int64_t row = (at >= 0 && at < v) ? at : 0;       // an index outside the vertices reads vertex 0
#pragma unroll
        for (int d = 0; d < 3; ++d) p[k][d] = vertices[row * 3 + d];
    }
    weights[i] = inside ? ts_clean_face_weight(p[0], p[1], p[2]) : 0.0;
}

__global__ __launch_bounds__(kThreads) void mark_kernel(int32_t f, int64_t entries, const int64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ order,
                                                        uint8_t* __restrict__ marks) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x + 2;
    if (i >= entries || keys[i] != keys[i - 2]) return;
    const int64_t e = order[i];
    if (e < 0 || e >= (int64_t)f * 3) return;
    marks[e / 3] = 1;
}

__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x.  Every vertex on the way is pointed at its parent's parent, as ECL-CC's intermediate pointer jumping
// does.  The loop goes on only while the value read is below the vertex it was read at: it strictly descends.
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t prev = x, curr = load_parent(parent, x);
    if (curr >= x) return x;
    for (;;) {
        const int32_t next = load_parent(parent, curr);
        if (next >= curr) return curr;
        __hip_atomic_store(parent + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        prev = curr;
        curr = next;
    }
}

__device__ __forceinline__ void join(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (seen >= hi) return;                 // cannot happen while invariant 1 holds; never loop on it
        ra = find_root(parent, seen);           // <= seen < hi
        rb = lo;
    }
}

__global__ __launch_bounds__(kThreads) void identity_kernel(int32_t v, int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < v) parent[i] = (int32_t)i;
}

__global__ __launch_bounds__(kThreads) void join_kernel(int32_t v, int32_t f, const int32_t* __restrict__ faces,
                                                        int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    const int32_t a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    if (a < 0 || a >= v || b < 0 || b >= v || c < 0 || c >= v) return;     // never index outside parent
    join(parent, a, b);
    join(parent, b, c);
}

__global__ __launch_bounds__(kThreads) void labels_kernel(int32_t v, const int32_t* parent,
                                                          int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= v) return;
    int32_t x = (int32_t)i;
    for (;;) {
        const int32_t p = load_parent(parent, x);
        if (p >= x) break;
        x = p;
    }
    labels[i] = x;
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)nblocks(n, kThreads)); }

}  // namespace

extern "C" {

int ts_clean_degenerate(int32_t f, const int32_t* faces, uint8_t* flags, void* stream) {
    if (f < 0) return TS_E_BADARG;
    if (f == 0) return 0;
    if (!faces || !flags) return TS_E_BADARG;
    hipLaunchKernelGGL(degenerate_kernel, blocks_of(f), dim3(kThreads), 0, (hipStream_t)stream, f, faces, flags);
    return launch_status();
}

int ts_clean_edge_keys(int32_t v, int32_t f, const int32_t* faces, int64_t* keys, void* stream) {
    if (v < 0 || f < 0) return TS_E_BADARG;
    if (f == 0) return 0;
    if (v < 1 || !faces || !keys) return TS_E_BADARG;
    hipLaunchKernelGGL(edge_keys_kernel, blocks_of(f), dim3(kThreads), 0, (hipStream_t)stream, v, f, faces, keys);
    return launch_status();
}

int ts_clean_face_weights(int32_t v, int32_t f, const float* vertices, const int32_t* faces, double* weights,
                          void* stream) {
    if (v < 0 || f < 0) return TS_E_BADARG;
    if (f == 0) return 0;
    if (v < 1 || !vertices || !faces || !weights) return TS_E_BADARG;
    hipLaunchKernelGGL(weights_kernel, blocks_of(f), dim3(kThreads), 0, (hipStream_t)stream, v, f, vertices, faces,
                       weights);
    return launch_status();
}

int ts_clean_mark(int32_t f, int64_t entries, const int64_t* sorted_keys, const int64_t* order, uint8_t* marks,
                  void* stream) {
    if (f < 0 || entries != (int64_t)f * 3) return TS_E_BADARG;
    if (f == 0) return 0;
    if (!sorted_keys || !order || !marks) return TS_E_BADARG;
    hipLaunchKernelGGL(mark_kernel, blocks_of(entries - 2), dim3(kThreads), 0, (hipStream_t)stream, f, entries,
                       sorted_keys, order, marks);
    return launch_status();
}

int ts_clean_components(int32_t v, int32_t f, const int32_t* faces, int32_t* parent, int32_t* labels, void* stream) {
    if (v < 0 || f < 0 || (f > 0 && v < 1)) return TS_E_BADARG;
    if (v == 0) return 0;
    if (!parent || !labels || (f > 0 && !faces)) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(identity_kernel, blocks_of(v), dim3(kThreads), 0, s, v, parent);
    if (f > 0) hipLaunchKernelGGL(join_kernel, blocks_of(f), dim3(kThreads), 0, s, v, f, faces, parent);
    hipLaunchKernelGGL(labels_kernel, blocks_of(v), dim3(kThreads), 0, s, v, (const int32_t*)parent, labels);
    return launch_status();
}

}  // extern "C"
