// appearance.hip - per-view appearance: a bilateral grid of 3x4 affine colour matrices applied
// between the render and the loss, its backward pass, the grid's total variation and the sums of a least-squares affine
// colour fit.  The arithmetic is appearance_math.h's, which tests/hostmath/appearance.cpp compiles for the host.
//
//   ts_appearance_fwd   one streaming pass; a thread owns four consecutive pixels of the flat image (48 bytes: three 16-byte
//                       loads and stores, a wave covers 3072 contiguous bytes); the vertices a workgroup's 1024 pixels can
//                       reach are staged in LDS where they fit, else a vertex is three 16-byte loads from cache
//   ts_appearance_bwd   a workgroup takes a 64 x 8 pixel tile, one wave per row segment: every thread writes its pixels'
//                       v_I and leaves (V, in, tz, l0) in LDS.  The tile's slab - one double per (vertex the tile's pixels
//                       can reach, entry c) - is then summed from that table in a fixed order, without atomics: thread
//                       (row, di, c) walks its row's 64 pixels in column order and adds each to the two luminance levels
//                       the pixel touches, in an LDS table of doubles that only this thread writes (the data-dependent
//                       level is an address, not a lane); thread e = (dj, di, l, c) then adds the eight rows in row order
//                       with their y weights.  A tile that reaches more vertex columns than the table holds (cells of a
//                       few pixels) lets thread e walk all the tile's pixels instead.  A second launch sums, per vertex,
//                       the slabs of the tiles that reach it in ascending tile order and rounds once.
//   ts_grid_tv          one workgroup: thread t takes elements t, t + 1024, ...; a binary tree over the threads
//   ts_affine_fit_sums  a wave takes 2048 consecutive pixels, lane i the pixels i, i + 64, ...; 22 doubles per wave, then
//                       the same one-workgroup sum
// Every result is a function of the inputs alone: the same bits on every run.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "appearance_math.h"

namespace {

constexpr int kE = TS_APP_ENTRIES, kTW = TS_APP_TILE_W, kTH = TS_APP_TILE_H, kThreads = 256;
constexpr int kSumThreads = 128, kReduce = TS_APP_REDUCE_THREADS;
constexpr int kRowTable = 4096;                        // doubles of the per-row level table (32 KB): 8 rows x ni x L x 12
static_assert(kTW == 64 && kThreads == 4 * kTW && kTH % 4 == 0, "one wave per row segment, four rows per pass");

// The vertices a workgroup's pixels can reach: rows [jlo, jlo + nj) x columns [ilo, ilo + ni) of every level.  Where they fit
// they are copied to LDS once (48 bytes each, vertex (l, jlo + dj, ilo + di) at ((l * nj + dj) * ni + di) * 3 float4) and
// every pixel's eight vertices are LDS reads; a workgroup that reaches more (grid cells of a few pixels) reads them from
// cache, three 16-byte loads each.
struct Reach { int jlo, nj, ilo, ni; };
constexpr int kStageVertices = kRowTable * 8 / 48;     // 682 vertices in the 32 KB the backward pass's table takes later

__device__ __forceinline__ bool stage_vertices(const float* __restrict__ G, int L, int Gh, int Gw, const Reach& r,
                                               float4* stage) {
    const int64_t count = (int64_t)L * r.nj * r.ni;
    if (count > kStageVertices) return false;            // (the same for every thread of the workgroup)
    for (int v = threadIdx.x; v < (int)count * 3; v += kThreads) {
        const int part = v % 3, vert = v / 3;
        const int di = vert % r.ni, dj = (vert / r.ni) % r.nj, l = vert / (r.ni * r.nj);
        stage[v] = reinterpret_cast<const float4*>(G + ts_app_vertex(Gh, Gw, l, r.jlo + dj, r.ilo + di))[part];
    }
    return true;
}

__device__ __forceinline__ void unpack_vertex(const float4* p, float* dst) {
    const float4 a = p[0], b = p[1], c = p[2];
    dst[0] = a.x; dst[1] = a.y; dst[2] = a.z; dst[3] = a.w;
    dst[4] = b.x; dst[5] = b.y; dst[6] = b.z; dst[7] = b.w;
    dst[8] = c.x; dst[9] = c.y; dst[10] = c.z; dst[11] = c.w;
}

template <bool kStaged>
__device__ __forceinline__ void load_vertex(const float* __restrict__ G, const float4* stage, const Reach& r, int Gh, int Gw,
                                            int l, int j, int i, float* dst) {
    if (kStaged) unpack_vertex(stage + ((l * r.nj + (j - r.jlo)) * r.ni + (i - r.ilo)) * 3, dst);
    else unpack_vertex(reinterpret_cast<const float4*>(G + ts_app_vertex(Gh, Gw, l, j, i)), dst);   // (a 16-byte aligned grid)
}

template <bool kStaged>
__device__ __forceinline__ void level_matrix(const float* __restrict__ G, const float4* stage, const Reach& r, int Gh, int Gw,
                                             int l, const TsAppAxis& ax, const TsAppAxis& ay, float* A) {
    float v00[kE], v01[kE], v10[kE], v11[kE];
    load_vertex<kStaged>(G, stage, r, Gh, Gw, l, ay.i0, ax.i0, v00);
    load_vertex<kStaged>(G, stage, r, Gh, Gw, l, ay.i0, ax.i1, v01);
    load_vertex<kStaged>(G, stage, r, Gh, Gw, l, ay.i1, ax.i0, v10);
    load_vertex<kStaged>(G, stage, r, Gh, Gw, l, ay.i1, ax.i1, v11);
    ts_app_bilerp(v00, v01, v10, v11, ax.t, ay.t, A);
}

// the two level matrices of a pixel
template <bool kStaged>
__device__ __forceinline__ void pixel_levels(const float* __restrict__ G, const float4* stage, const Reach& r, int Gh, int Gw,
                                             const TsAppLevel& z, const TsAppAxis& ax, const TsAppAxis& ay, float* A0,
                                             float* A1) {
    level_matrix<kStaged>(G, stage, r, Gh, Gw, z.l0, ax, ay, A0);
    if (z.l1 != z.l0) level_matrix<kStaged>(G, stage, r, Gh, Gw, z.l1, ax, ay, A1);
    else for (int c = 0; c < kE; ++c) A1[c] = A0[c];
}

__device__ __forceinline__ void pixel_fwd(int W, int H, int L, int Gh, int Gw, const float* __restrict__ G,
                                          const float4* stage, const Reach& r, bool staged, int x, int y, const float* in,
                                          float* out) {
    const TsAppAxis ax = ts_app_axis(x, W, Gw), ay = ts_app_axis(y, H, Gh);
    const TsAppLevel z = ts_app_level(ts_app_gray(in[0], in[1], in[2]), L);
    float A0[kE], A1[kE];
    if (staged) pixel_levels<true>(G, stage, r, Gh, Gw, z, ax, ay, A0, A1);
    else pixel_levels<false>(G, stage, r, Gh, Gw, z, ax, ay, A0, A1);
    ts_app_pixel_fwd(A0, A1, z.t, in[0], in[1], in[2], out);
}

// kVec: image and output are 16-byte aligned (three float4 per thread); otherwise the same pixels with scalar accesses
template <bool kVec>
__global__ __launch_bounds__(kThreads) void appearance_fwd_kernel(int H, int W, int L, int Gh, int Gw, int64_t N,
                                                                  const float* __restrict__ I,
                                                                  const float* __restrict__ G, float* __restrict__ O) {
    __shared__ float4 stage[kStageVertices * 3];
    // the workgroup's 1024 consecutive pixels: one stretch of a row, or whole rows
    const int64_t first = (int64_t)blockIdx.x * (4 * kThreads), last = (first + 4 * kThreads < N ? first + 4 * kThreads : N) - 1;
    const int ya = (int)((unsigned)first / (unsigned)W), yb = (int)((unsigned)last / (unsigned)W);       // (N < 2^29)
    const int xa = ya == yb ? (int)(first - (int64_t)ya * W) : 0, xb = ya == yb ? (int)(last - (int64_t)ya * W) : W - 1;
    Reach r;
    r.jlo = ts_app_axis(ya, H, Gh).i0; r.nj = ts_app_axis(yb, H, Gh).i1 - r.jlo + 1;
    r.ilo = ts_app_axis(xa, W, Gw).i0; r.ni = ts_app_axis(xb, W, Gw).i1 - r.ilo + 1;
    const bool staged = stage_vertices(G, L, Gh, Gw, r, stage);
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x, p0 = 4 * q;
    if (p0 >= N) return;
    const int count = (int)(N - p0 < 4 ? N - p0 : 4);
    float in[12], out[12];
    if (kVec && count == 4) {
        const float4* src = reinterpret_cast<const float4*>(I) + 3 * q;
        const float4 a = src[0], b = src[1], c = src[2];
        in[0] = a.x; in[1] = a.y; in[2] = a.z; in[3] = a.w; in[4] = b.x; in[5] = b.y; in[6] = b.z; in[7] = b.w;
        in[8] = c.x; in[9] = c.y; in[10] = c.z; in[11] = c.w;
    } else {
        for (int m = 0; m < 3 * count; ++m) in[m] = I[3 * p0 + m];
    }
    int y = (int)((unsigned)p0 / (unsigned)W), x = (int)((unsigned)p0 - (unsigned)y * (unsigned)W);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m < count) pixel_fwd(W, H, L, Gh, Gw, G, stage, r, staged, x, y, in + 3 * m, out + 3 * m);
        if (++x == W) { x = 0; ++y; }
    }
    if (kVec && count == 4) {
        float4* dst = reinterpret_cast<float4*>(O) + 3 * q;
        dst[0] = make_float4(out[0], out[1], out[2], out[3]);
        dst[1] = make_float4(out[4], out[5], out[6], out[7]);
        dst[2] = make_float4(out[8], out[9], out[10], out[11]);
    } else {
        for (int m = 0; m < 3 * count; ++m) O[3 * p0 + m] = out[m];
    }
}

// slabs: one per tile (tile = by * gridDim.x + bx), `slab_doubles` apart; entry ((dj * ni + di) * L + l) * 12 + c of a
// slab belongs to vertex (l, jlo + dj, ilo + di) with (jlo, nj), (ilo, ni) the tile's reach (ts_app_tile_reach)
__global__ __launch_bounds__(kThreads) void appearance_bwd_kernel(int H, int W, int L, int Gh, int Gw,
                                                                  const float* __restrict__ I,
                                                                  const float* __restrict__ G,
                                                                  const float* __restrict__ V, float* __restrict__ vI,
                                                                  double* __restrict__ slabs, int64_t slab_doubles) {
    __shared__ float px[kTH * kTW][8];                  // V[3], in[3], tz, l0 (bits) of every pixel of the tile
    // [row][di][l][c]: a row's pixels summed along x and z; before that, the staged vertices of the tile's reach
    __shared__ __attribute__((aligned(16))) double table[kRowTable];
    __shared__ int col_i0[kTW], col_i1[kTW], row_j0[kTH], row_j1[kTH];      // relative to the reach; -8: outside the image
    __shared__ float col_t[kTW], row_t[kTH];
    const int tid = threadIdx.x, col = tid & (kTW - 1);
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    int ilo, ni, jlo, nj;
    ts_app_tile_reach(blockIdx.x, kTW, W, Gw, &ilo, &ni);
    ts_app_tile_reach(blockIdx.y, kTH, H, Gh, &jlo, &nj);
    if (tid < kTW) {
        const bool in = x0 + tid < W;
        const TsAppAxis a = ts_app_axis(in ? x0 + tid : 0, W, Gw);
        col_i0[tid] = in ? a.i0 - ilo : -8; col_i1[tid] = in ? a.i1 - ilo : -8; col_t[tid] = a.t;
    } else if (tid < kTW + kTH) {
        const int r = tid - kTW;
        const bool in = y0 + r < H;
        const TsAppAxis a = ts_app_axis(in ? y0 + r : 0, H, Gh);
        row_j0[r] = in ? a.i0 - jlo : -8; row_j1[r] = in ? a.i1 - jlo : -8; row_t[r] = a.t;
    }
    Reach reach;
    reach.jlo = jlo; reach.nj = nj; reach.ilo = ilo; reach.ni = ni;
    const float4* stage = reinterpret_cast<const float4*>(table);
    const bool staged = stage_vertices(G, L, Gh, Gw, reach, reinterpret_cast<float4*>(table));
    __syncthreads();
    const int x = x0 + col;
#pragma unroll
    for (int m = 0; m < kTH / 4; ++m) {
        const int row = (tid >> 6) + 4 * m, y = y0 + row;
        if (x >= W || y >= H) continue;                  // (its column or row is marked outside: px is never read)
        const size_t at = ((size_t)y * W + x) * 3;
        const float r = I[at], g = I[at + 1], b = I[at + 2];
        const float v[3] = {V[at], V[at + 1], V[at + 2]};
        const TsAppAxis ax = ts_app_axis(x, W, Gw), ay = ts_app_axis(y, H, Gh);
        const TsAppLevel z = ts_app_level(ts_app_gray(r, g, b), L);
        float A0[kE], A1[kE], vA[kE], v_in[3];
        if (staged) pixel_levels<true>(G, stage, reach, Gh, Gw, z, ax, ay, A0, A1);
        else pixel_levels<false>(G, stage, reach, Gh, Gw, z, ax, ay, A0, A1);
        ts_app_pixel_bwd(A0, A1, z, L, r, g, b, v, vA, v_in);
        vI[at] = v_in[0]; vI[at + 1] = v_in[1]; vI[at + 2] = v_in[2];
        float* s = px[row * kTW + col];
        s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; s[3] = r; s[4] = g; s[5] = b; s[6] = z.t; s[7] = __int_as_float(z.l0);
    }
    __syncthreads();
    int64_t entries = (int64_t)nj * ni * L * kE;
    if (entries > slab_doubles) entries = 0;             // (cannot happen: the host sized the slab with the same function)
    double* slab = slabs + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * slab_doubles;
    const int per_row = ni * L * kE;
    if ((int64_t)kTH * per_row <= kRowTable) {
        // x and z: thread (row, di, c) owns table[row][di][0..L)[c] and adds its row's pixels in column order
        for (int u = tid; u < kTH * per_row; u += kThreads) table[u] = 0.0;
        __syncthreads();
        for (int u = tid; u < kTH * ni * kE; u += kThreads) {
            const int c = u % kE, di = (u / kE) % ni, row = u / (kE * ni);
            if (row_j0[row] < 0) continue;               // a row below the image
            const int q = c >> 2, k = c & 3;
            double* mine = table + ((size_t)row * ni + di) * L * kE + c;
            for (int cc = 0; cc < kTW; ++cc) {
                const float fx = ts_app_hat(di, col_i0[cc], col_i1[cc], col_t[cc]);
                if (fx == 0.0f) continue;
                const float* s = px[row * kTW + cc];
                const int l0 = __float_as_int(s[7]);
                const float tz = s[6], vA = s[q] * (k < 3 ? s[3 + k] : 1.0f);
                const double term = (double)fx * (double)vA;
                if (L == 1) {
                    mine[0] += (double)((1.0f - tz) + tz) * term;
                } else {
                    mine[l0 * kE] += (double)(1.0f - tz) * term;
                    mine[(l0 + 1) * kE] += (double)tz * term;
                }
            }
        }
        __syncthreads();
        // y: entry (dj, di, l, c) of the slab from the eight rows, in row order
        for (int64_t e = tid; e < entries; e += kThreads) {
            const int within = (int)(e % per_row), dj = (int)(e / per_row);
            double acc = 0.0;
            for (int row = 0; row < kTH; ++row) {
                const float fy = ts_app_hat(dj, row_j0[row], row_j1[row], row_t[row]);
                if (fy != 0.0f) acc += (double)fy * table[row * per_row + within];
            }
            slab[e] = acc;
        }
        return;
    }
    for (int64_t e = tid; e < entries; e += kThreads) {
        const int c = (int)(e % kE), l = (int)((e / kE) % L);
        const int di = (int)((e / ((int64_t)kE * L)) % ni), dj = (int)(e / ((int64_t)kE * L * ni));
        const int q = c >> 2, k = c & 3;
        double acc = 0.0;
        for (int row = 0; row < kTH; ++row) {
            const float fy = ts_app_hat(dj, row_j0[row], row_j1[row], row_t[row]);
            if (fy == 0.0f) continue;
            for (int cc = 0; cc < kTW; ++cc) {
                const float fx = ts_app_hat(di, col_i0[cc], col_i1[cc], col_t[cc]);
                if (fx == 0.0f) continue;
                const float* s = px[row * kTW + cc];
                const int l0 = __float_as_int(s[7]);
                const float fz = ts_app_hat(l, l0, L == 1 ? l0 : l0 + 1, s[6]);
                if (fz == 0.0f) continue;
                const float vA = s[q] * (k < 3 ? s[3 + k] : 1.0f);
                acc += ((double)fz * (double)fy * (double)fx) * (double)vA;
            }
        }
        slab[e] = acc;
    }
}

// one workgroup per vertex column (j, i): the tiles that reach it, in ascending tile order, for each of its L * 12 entries
__global__ __launch_bounds__(kSumThreads) void appearance_sum_kernel(int H, int W, int L, int Gh, int Gw, int tiles_x,
                                                                     int tiles_y, const double* __restrict__ slabs,
                                                                     int64_t slab_doubles, float* __restrict__ vG) {
    __shared__ int range[4];                             // bx lo, bx hi, by lo, by hi
    const int tid = threadIdx.x, i = blockIdx.x % Gw, j = blockIdx.x / Gw;
    if (tid == 0) { range[0] = tiles_x; range[1] = -1; range[2] = tiles_y; range[3] = -1; }
    __syncthreads();
    for (int t = tid; t < tiles_x; t += kSumThreads) {
        int lo, n;
        ts_app_tile_reach(t, kTW, W, Gw, &lo, &n);
        if (i >= lo && i < lo + n) { atomicMin(&range[0], t); atomicMax(&range[1], t); }
    }
    for (int t = tid; t < tiles_y; t += kSumThreads) {
        int lo, n;
        ts_app_tile_reach(t, kTH, H, Gh, &lo, &n);
        if (j >= lo && j < lo + n) { atomicMin(&range[2], t); atomicMax(&range[3], t); }
    }
    __syncthreads();
    const int bx0 = range[0], by0 = range[2];
    const int nbx = range[1] - bx0 + 1, nby = range[3] - by0 + 1;          // (not positive: no tile reaches the vertex)
    const int count = nbx > 0 && nby > 0 ? nbx * nby : 0;
    // the offset of entry e in the slab of the t-th of those tiles, in ascending tile order; -1: the tile has no such entry
    auto slab_entry = [&](int t, int e) -> int64_t {
        const int by = by0 + t / nbx, bx = bx0 + t % nbx;
        int jlo, nj, ilo, ni;
        ts_app_tile_reach(by, kTH, H, Gh, &jlo, &nj);
        ts_app_tile_reach(bx, kTW, W, Gw, &ilo, &ni);
        if (j < jlo || j >= jlo + nj || i < ilo || i >= ilo + ni) return -1;
        const int64_t at = ((int64_t)(j - jlo) * ni + (i - ilo)) * L * kE + e;
        return at < slab_doubles ? ((int64_t)by * tiles_x + bx) * slab_doubles + at : -1;
    };
    constexpr int kAhead = 8;                            // loads in flight per thread; the additions stay in tile order
    for (int e = tid; e < L * kE; e += kSumThreads) {
        double acc = 0.0;
        for (int t = 0; t < count; t += kAhead) {
            double v[kAhead];
            bool has[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int64_t at = t + u < count ? slab_entry(t + u, e) : -1;
                has[u] = at >= 0;
                v[u] = has[u] ? slabs[at] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
                if (has[u]) acc += v[u];
        }
        const int l = e / kE, c = e % kE;
        vG[ts_app_vertex(Gh, Gw, l, j, i) + c] = (float)acc;
    }
}

// a binary tree over the kReduce threads' values, the same additions on every run; the total ends in part[0]
__device__ __forceinline__ void tree_sum(double* part) {
    __syncthreads();
    for (int step = kReduce / 2; step >= 1; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
}

// (v_out may be v_in: an element is read and written by one thread)
__global__ __launch_bounds__(kReduce) void grid_tv_kernel(int L, int Gh, int Gw, const float* __restrict__ G, float weight,
                                                          const float* v_in, double* __restrict__ value, float* v_out) {
    __shared__ double part[3][kReduce];
    double n[3], acc[3] = {0.0, 0.0, 0.0};
    ts_app_tv_counts(L, Gh, Gw, n);
    const int total = L * Gh * Gw * kE;
#pragma unroll 4
    for (int e = threadIdx.x; e < total; e += kReduce) {
        const float g = (float)ts_app_tv_element(G, L, Gh, Gw, e, n, acc);
        v_out[e] = (v_in ? v_in[e] : 0.0f) + weight * g;
    }
    for (int a = 0; a < 3; ++a) part[a][threadIdx.x] = acc[a];
    for (int a = 0; a < 3; ++a) tree_sum(part[a]);
    if (threadIdx.x == 0) {
        const double sums[3] = {part[0][0], part[1][0], part[2][0]};
        value[0] = ts_app_tv_value(sums, n);
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void fit_waves_kernel(int64_t N, const float* __restrict__ X, const T* __restrict__ Y,
                                                             double* __restrict__ partials) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int64_t first = wave * 64 * TS_APP_FIT_LANE_PIXELS;
    if (first >= N) return;                              // (wave-uniform)
    double acc[TS_APP_FIT_SUMS];
    for (int s = 0; s < TS_APP_FIT_SUMS; ++s) acc[s] = 0.0;
    for (int m = 0; m < TS_APP_FIT_LANE_PIXELS; ++m) {
        const int64_t p = first + lane + 64 * (int64_t)m;
        if (p >= N) break;
        float t[3];
        for (int c = 0; c < 3; ++c) {
            if constexpr (sizeof(T) == 1) t[c] = ts_app_byte_to_float(Y[3 * p + c]); else t[c] = Y[3 * p + c];
        }
        ts_app_fit_pixel(X[3 * p], X[3 * p + 1], X[3 * p + 2], t[0], t[1], t[2], acc);
    }
    for (int s = 0; s < TS_APP_FIT_SUMS; ++s) {
        const double total = wave_sum(acc[s]);
        if (lane == 0) partials[wave * TS_APP_FIT_SUMS + s] = total;
    }
}

__global__ __launch_bounds__(kReduce) void fit_reduce_kernel(int64_t waves, const double* __restrict__ partials,
                                                             double* __restrict__ out) {
    __shared__ double part[kReduce];
    for (int s = 0; s < TS_APP_FIT_SUMS; ++s) {
        double acc = 0.0;
        for (int64_t i = threadIdx.x; i < waves; i += kReduce) acc += partials[i * TS_APP_FIT_SUMS + s];
        part[threadIdx.x] = acc;
        tree_sum(part);
        if (threadIdx.x == 0) out[s] = part[0];
        __syncthreads();
    }
}

bool sizes_ok(int32_t h, int32_t w, int32_t L, int32_t Gh, int32_t Gw) {
    if (h <= 0 || w <= 0 || L <= 0 || Gh <= 0 || Gw <= 0) return false;
    if ((int64_t)h * w > INT32_MAX / 4) return false;                        // float offsets of the image stay in 32 bits
    return (int64_t)L * Gh * Gw * kE <= INT32_MAX;
}

}  // namespace

extern "C" {

int64_t ts_appearance_ws_bytes(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w) {
    if (!sizes_ok(height, width, levels, grid_h, grid_w)) return 0;
    return ts_app_tiles(height, width) * ts_app_slab_doubles(height, width, levels, grid_h, grid_w) * (int64_t)sizeof(double);
}

int ts_appearance_fwd(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w, const float* image,
                      const float* grid, float* out, void* stream) {
    if (!sizes_ok(height, width, levels, grid_h, grid_w) || !image || !grid || !out) return TS_E_BADARG;
    if ((uintptr_t)grid % 16 || (uintptr_t)image % sizeof(float) || (uintptr_t)out % sizeof(float)) return TS_E_BADARG;
    const int64_t n = (int64_t)height * width;
    const dim3 blocks((unsigned)nblocks((n + 3) / 4, kThreads));
    hipStream_t s = (hipStream_t)stream;
    if ((uintptr_t)image % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(appearance_fwd_kernel<true>, blocks, dim3(kThreads), 0, s, (int)height, (int)width, (int)levels,
                           (int)grid_h, (int)grid_w, n, image, grid, out);
    else
        hipLaunchKernelGGL(appearance_fwd_kernel<false>, blocks, dim3(kThreads), 0, s, (int)height, (int)width, (int)levels,
                           (int)grid_h, (int)grid_w, n, image, grid, out);
    return launch_status();
}

int ts_appearance_bwd(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w, const float* image,
                      const float* grid, const float* v_out, float* v_image, void* ws, float* v_grid, void* stream) {
    if (!sizes_ok(height, width, levels, grid_h, grid_w)) return TS_E_BADARG;
    if (!image || !grid || !v_out || !v_image || !ws || !v_grid) return TS_E_BADARG;
    if ((uintptr_t)grid % 16 || (uintptr_t)ws % sizeof(double)) return TS_E_BADARG;
    if ((uintptr_t)image % sizeof(float) || (uintptr_t)v_out % sizeof(float) || (uintptr_t)v_image % sizeof(float) ||
        (uintptr_t)v_grid % sizeof(float)) return TS_E_BADARG;
    const int tiles_x = (width + kTW - 1) / kTW, tiles_y = (height + kTH - 1) / kTH;
    if (tiles_y > 65535) return TS_E_BADARG;                                  // (more than half a million rows)
    const int64_t slab = ts_app_slab_doubles(height, width, levels, grid_h, grid_w);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(appearance_bwd_kernel, dim3(tiles_x, tiles_y), dim3(kThreads), 0, s, (int)height, (int)width,
                       (int)levels, (int)grid_h, (int)grid_w, image, grid, v_out, v_image, (double*)ws, slab);
    hipLaunchKernelGGL(appearance_sum_kernel, dim3((unsigned)(grid_h * grid_w)), dim3(kSumThreads), 0, s, (int)height,
                       (int)width, (int)levels, (int)grid_h, (int)grid_w, tiles_x, tiles_y, (const double*)ws, slab, v_grid);
    return launch_status();
}

int ts_grid_tv(int32_t levels, int32_t grid_h, int32_t grid_w, const float* grid, float weight, const float* v_in,
               double* value, float* v_out, void* stream) {
    if (!sizes_ok(1, 1, levels, grid_h, grid_w) || !grid || !value || !v_out) return TS_E_BADARG;
    if ((uintptr_t)value % sizeof(double) || (uintptr_t)grid % sizeof(float) || (uintptr_t)v_out % sizeof(float) ||
        (uintptr_t)v_in % sizeof(float)) return TS_E_BADARG;
    hipLaunchKernelGGL(grid_tv_kernel, dim3(1), dim3(kReduce), 0, (hipStream_t)stream, (int)levels, (int)grid_h,
                       (int)grid_w, grid, weight, v_in, value, v_out);
    return launch_status();
}

int64_t ts_affine_fit_ws_bytes(int32_t height, int32_t width) {
    if (height <= 0 || width <= 0) return 0;
    return ts_app_fit_waves((int64_t)height * width) * TS_APP_FIT_SUMS * (int64_t)sizeof(double);
}

int ts_affine_fit_sums(int32_t height, int32_t width, const float* image, const void* target, int32_t target_is_u8,
                       void* ws, double* out22, void* stream) {
    if (height <= 0 || width <= 0 || !image || !target || !ws || !out22) return TS_E_BADARG;
    if ((int64_t)height * width > INT32_MAX / 4) return TS_E_BADARG;
    if ((uintptr_t)ws % sizeof(double) || (uintptr_t)out22 % sizeof(double) || (uintptr_t)image % sizeof(float)) return TS_E_BADARG;
    if (!target_is_u8 && (uintptr_t)target % sizeof(float)) return TS_E_BADARG;
    const int64_t n = (int64_t)height * width, waves = ts_app_fit_waves(n);
    const dim3 blocks((unsigned)nblocks(waves, kThreads / 64));
    hipStream_t s = (hipStream_t)stream;
    if (target_is_u8)
        hipLaunchKernelGGL(fit_waves_kernel<uint8_t>, blocks, dim3(kThreads), 0, s, n, image, (const uint8_t*)target, (double*)ws);
    else
        hipLaunchKernelGGL(fit_waves_kernel<float>, blocks, dim3(kThreads), 0, s, n, image, (const float*)target, (double*)ws);
    hipLaunchKernelGGL(fit_reduce_kernel, dim3(1), dim3(kReduce), 0, s, waves, (const double*)ws, out22);
    return launch_status();
}

}  // extern "C"
