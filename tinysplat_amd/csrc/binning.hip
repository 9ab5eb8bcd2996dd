// binning.hip - tile binning and per-tile depth sort for gfx950.
//
// What gsplat's rasterize_gaussians does before compositing (the part reached from
// /root/reference/tinysplat/splatting/rasterize.py:44,50): cumsum(num_tiles_hit), emit one
// (tile<<32 | depth bits, gaussian id) pair per covered tile, global 64-bit sort, bin edges.
// Here the same final order (tile-major, then depth bits, ties by ascending Gaussian id) is produced
// without a global sort:
//   scan_tiles      wave-scan (DPP-free __shfl_up ladder inside a wave, LDS across the 4 waves)
//   bin_count       per-chunk tile histograms in LDS (ds_add), B x T count matrix, no global atomics
//   tile_offsets    column scan of the matrix (per-chunk bases, one launch) + exclusive scan over tiles -> tile_bins
//   bin_scatter     replays each chunk with LDS cursors preloaded from its bases, 4-byte id stores
//                   (the sort gathers depth by id from the 4 N-byte, L2-resident depth array;
//                   sort key = depth_bits << 32 | gaussian_id, unique inside a tile)
//   sort_tiles      one workgroup per tile.  <= 1024 keys: bitonic network with the keys in registers
//                   (in-thread stages), 64-bit lane exchanges (in-wave stages) and LDS only for the
//                   few cross-wave stages.  Larger tiles: per-tile sample sort (splitters from a
//                   sorted sample, LDS histogram + cursors, then every wave sorts sub-buckets of
//                   <= 256 keys on its own) - O(n log n), no size limit
//   pack_splats     gathers the compositing operands of a Gaussian into one 48-byte record
// Frames that scatter in two hops (2^18 Gaussians and more) have a GROUP FORM of bin_count / tile_offsets / bin_scatter:
// counts per (chunk, group of 32 tiles), all offsets in one launch, the lists counted by the scatter's fine hop.
// ONE WALK form of the same frames (bin_scatter_emit / group_tile_offsets<false> / bin_scatter_fine_runs): the Gaussians are
// walked once - a chunk stages its pairs in LDS, orders them by group and writes them into its own bounding-box slots of
// the scratch buffer; the fine hop gathers its group's run from every chunk.
// Every form lists a Gaussian through ONE piece of code, walk_one (box, TightTest, row_range per tile row, emit_row); the
// fine hops share place_pass, the two emit kernels the EmitChunk pieces, the offsets launches arm_guard / empty_every_list.
// Traffic: 4 I written + 4 I read (+ gathers) + 4 I written (+ 8 B T for the count matrix; 8 B G + 4 I read once more in the
// group form) against the 36 I a 3-pass 64-bit LSD radix sort of key+payload would move at minimum.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "pack.h"
#include "row_spans.h"
#include "splat_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;                       // per thread
constexpr int kScanBlock = kThreads * kScanItems;   // 1024 elements per block

__device__ __forceinline__ int wave_inclusive_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// block-wide inclusive scan of one int per thread (WAVES waves; 256 threads = 4 by default); returns the
// inclusive value, *total = block sum.
template <int WAVES = 4>
__device__ __forceinline__ int block_inclusive_scan(int v, int* total) {
    __shared__ int wave_sums[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = wave_inclusive_scan(v);
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int add = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = wave_sums[w];
        if (w < wave) add += s;
        tot += s;
    }
    *total = tot;
    __syncthreads();
    return inc + add;
}

// total_out (may be null): device-visible address - pinned host memory - that receives out[n-1], the
// grand total, from the thread that produces it (system-scope store): the host reads it there without
// a copy operation behind the scan
__global__ __launch_bounds__(kThreads) void scan_local_kernel(int n, const int* __restrict__ in,
                                                              int* __restrict__ out,
                                                              int* __restrict__ block_sums,
                                                              int* __restrict__ total_out) {
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v[kScanItems];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        sum += v[k];
        v[k] = sum;
    }
    int total;
    const int inc = block_inclusive_scan(sum, &total);
    const int excl = inc - sum;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) {
            out[base + k] = v[k] + excl;
            if (total_out && gridDim.x == 1 && base + k == n - 1)
                __hip_atomic_store(total_out, v[k] + excl, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// adds to every element of block b the sum of the blocks before it, which the block reduces itself from
// the <= n / 1024 block sums (a separate single-workgroup scan of those sums would be one more launch on
// the critical path of the frame: ~5 us each on MI355X however small the kernel)
__global__ __launch_bounds__(kThreads) void scan_add_kernel(int n, int* __restrict__ out,
                                                            const int* __restrict__ block_sums,
                                                            int* __restrict__ total_out) {
    __shared__ int red[kThreads / 64];
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += kThreads) part += block_sums[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) add += red[w];
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) {
            const int v = out[base + k] + add;
            if (blockIdx.x != 0) out[base + k] = v;
            if (total_out && base + k == n - 1)
                __hip_atomic_store(total_out, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
}

// ---- tile bucketing without global atomics --------------------------------------------------
// Device-scope atomics on MI355X are executed memory-side (the per-XCD L2s are not coherent), and
// measured ~25 G atomics/s: 6 M intersections cost 0.25 ms per pass.  Instead the Gaussians are cut
// into B contiguous chunks; workgroup b builds the tile histogram of its chunk in LDS (ds_add, no
// memory traffic), the B x T count matrix is column-scanned into per-(chunk,tile) bases, and the
// scatter pass replays the chunk with LDS cursors preloaded from those bases.  The order inside a
// bucket is arbitrary (LDS atomic order); sort_tiles makes it canonical.
// Block (b, w) replays chunk b and touches the tiles of window w.  Measured on config 3 / config 5:
// one window per chunk (as long as the tile count fits the LDS) with 4096-Gaussian chunks is the
// fastest split - larger chunks with several tile windows make the runs written into a bucket
// longer but re-read every Gaussian once per window and lost 10-30 %.
#ifndef TS_BIN_THREADS
#define TS_BIN_THREADS 1024
#endif
constexpr int kBinThreads = TS_BIN_THREADS;
#ifndef TS_BIN_CHUNK
#define TS_BIN_CHUNK 4096
#endif
constexpr int kBinChunkMin = TS_BIN_CHUNK;  // Gaussians per chunk (at least)
constexpr int kBinMaxChunks = 512;
constexpr int kBinWindowMax = 36864;      // tiles per LDS window (144 KiB of the 160 KiB LDS)
constexpr int kBinTargetBlocks = 1;       // chunks x windows aimed at (1 = no extra windows)

// Chunk size: kBinChunkMin Gaussians for scenes of ~1 M and more (one workgroup per CU); smaller scenes get
// smaller chunks, down to 1024, so that a 100 k-Gaussian frame still spreads over ~100 workgroups
// (config 2: bin_count 30 -> 15 us, bin_scatter 33 -> 17 us).
__host__ __device__ inline int bin_num_chunks(int n) {
    int per = n / 192;
    per = per < 1024 ? 1024 : (per > kBinChunkMin ? kBinChunkMin : per);
    int b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > kBinMaxChunks) b = kBinMaxChunks;
    return b;
}

// tiles per window: enough windows to reach kBinTargetBlocks workgroups, never above the LDS budget
inline int bin_window_tiles(int n, int num_tiles) {
    const int chunks = bin_num_chunks(n);
    int nwin = (kBinTargetBlocks + chunks - 1) / chunks;
    const int max_win = (num_tiles + 255) / 256;           // keep windows >= 256 tiles
    if (nwin > max_win) nwin = max_win;
    if (nwin < 1) nwin = 1;
    int window = (num_tiles + nwin - 1) / nwin;
    window = (window + 63) & ~63;
    if (window > kBinWindowMax) window = kBinWindowMax;
    return window;
}

// Tight binning (splats != nullptr): a (Gaussian, tile) pair of the bounding box is dropped when the
// packed record proves that no pixel of the 16x16 tile can reach alpha >= 1/255.  Dropped pairs
// contribute exactly nothing to the image or to any gradient, so the frame is bit-identical; on the
// random scenes ~36 % of the bounding-box pairs go away before the scatter, the sort and the
// compositing kernels ever see them.  Count and scatter make the same decisions (same code, same
// inputs).  With splats == nullptr the lists are gsplat's bounding-box lists.
//
// The test itself is ts::TightTest in splat_math.h, beside ts::rect_may_contribute: the header compiles for the host
// too, and tests/test_hostmath_cull.py checks every rejection against a float64 per-pixel evaluation.
using ts::TightTest;

// THE PER-GAUSSIAN WALK, stated once for the walks of this file (walk_chunk, the span walk's fallback, and - its row
// mapping - the balanced walk): the list forms are held to each other bit for bit, and they are because they decide here.
// emit_row: 16x16 tiles lo..hi-1 of tile row ty -> emit(list, i) for the list columns: those tiles, or the wide tiles
// that contain them (ws: list column = 16x16 column >> ws; tbx: list columns per row)
template <typename Emit>
__device__ __forceinline__ void emit_row(int ty, int lo, int hi, int i, const ts_camera& cam, int ws, int tbx, Emit emit) {
    for (int tx = lo >> ws; tx <= (hi - 1) >> ws; ++tx) emit((ty - cam.tile_row0) * tbx + tx, i);
}
// walk_one: Gaussian i of radius r > 0 with its loaded operands (q0, q1: the two record words of the tight test, unused
// for bounding-box lists) -> emit(list, i) for every list it is entered in
template <typename Emit>
__device__ __forceinline__ void walk_one(bool tight_lists, int i, int r, float2 xy, float4 q0, float4 q1,
                                         const ts_camera& cam, int ws, int tbx, Emit emit) {
    const ts::TileBox b = ts::tile_bbox(xy.x, xy.y, (float)r, cam.tile_bounds_x, cam.tile_bounds_y, cam.tile_row0,
                                        cam.tile_rows);
    if (b.maxy <= b.miny || b.maxx <= b.minx) return;            // not in this stripe (its record was never written)
    const TightTest tight(tight_lists, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, (float)r);
    if (tight.cull_all) return;
    for (int ty = b.miny; ty < b.maxy; ++ty) {
        int lo, hi;
        tight.row_range(ty, b.minx, b.maxx, lo, hi);
        if (hi <= lo) continue;
        emit_row(ty, lo, hi, i, cam, ws, tbx, emit);
    }
}

// Walks the Gaussians of a chunk and calls emit(t) for every list (tile of the lists' shape, index t
// inside the launch) a Gaussian is entered in.  Count and scatter replay the same walk, so they agree.
// A thread handles kBinThreads-strided Gaussians; the operands of kBinPre of them (radius, centre, the
// two record words of the tight test) are loaded before the first one is processed, and a workgroup is
// 1024 threads: with one workgroup per CU the walk is a chain of dependent loads and square roots per
// Gaussian, and more waves / more loads in flight are what hide it.  Measured against 512 threads without
// prefetch: bin_count 32.5 -> 25.7 us on config 3, 125 -> 111 us on config 5; bin_scatter 0.63 -> 0.49 ms
// on config 5 (63 us either way on config 3, where the scattered 4-byte stores bind).
#ifndef TS_BIN_PRE
#define TS_BIN_PRE 2
#endif
constexpr int kBinPre = TS_BIN_PRE;
template <typename Emit>
__device__ __forceinline__ void walk_chunk(int g0, int g1, const float* __restrict__ xys,
                                           const int* __restrict__ radii,
                                           const float4* __restrict__ splats, const ts_camera& cam,
                                           Emit emit) {
    const int ws = cam.wide_tiles ? 1 : 0;                         // list column = 16x16 column >> ws
    const int tbx = (cam.tile_bounds_x + ws) >> ws;
    const bool tight_lists = splats != nullptr;
    for (int base = g0 + threadIdx.x; base < g1; base += kBinPre * kBinThreads) {
        int r[kBinPre];
        float2 xy[kBinPre];
        float4 q0[kBinPre], q1[kBinPre];
#pragma unroll
        for (int u = 0; u < kBinPre; ++u) {
            const int i = base + u * kBinThreads;
            r[u] = i < g1 ? radii[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kBinPre; ++u) {
            const int i = base + u * kBinThreads;
            xy[u] = make_float2(0.f, 0.f);
            q0[u] = q1[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r[u] > 0) {
                xy[u] = reinterpret_cast<const float2*>(xys)[i];
                if (tight_lists) { q0[u] = splats[3 * (size_t)i]; q1[u] = splats[3 * (size_t)i + 1]; }
            }
        }
#pragma unroll
        for (int u = 0; u < kBinPre; ++u) {
            if (r[u] <= 0) continue;
            walk_one(tight_lists, base + u * kBinThreads, r[u], xy[u], q0[u], q1[u], cam, ws, tbx, emit);
        }
    }
}

// LOAD-BALANCED WALK (round 4).  walk_chunk gives every lane one Gaussian and lets it loop over
// its tile rows and the tiles of a row: a Gaussian of the random scenes has 1-3 rows, the slowest lane of a wave ~5,
// and the 35-instruction row_range runs at ~40 % lane use (bin_count: 670 wave instructions per 64 Gaussians).  Here
// a batch of 1024 Gaussians (one per thread) is expanded into ITEMS = (Gaussian, tile row): phase 1 computes the box
// and the TightTest once per Gaussian and stashes what a row needs in LDS; a workgroup scan of the row counts gives
// every Gaussian its item range; the items are written out in windows of kItemCap and phase 2 hands consecutive
// items to consecutive lanes.  Same decisions as walk_one (phase 1 restates its first four lines around the stash - taken
// from a shared helper, by callback or by struct, they compile to other instructions in the two balanced kernels,
// profiles/r27_binning_shared.txt; phase 2 has the stashed TightTest members, the same row_range and emit_row), different
// ORDER of the emits - which no caller depends on (LDS histogram / cursors; the per-tile sort follows).
constexpr int kItemCap = 4096;                    // items per window
constexpr int kStashWords = 11;                   // per Gaussian: 10 TightTest floats + (minx | maxx << 16)
constexpr size_t kBalancedLds = (size_t)(kStashWords * kBinThreads + kItemCap + 32) * 4;      // static LDS it needs
template <typename Emit>
__device__ __forceinline__ void walk_chunk_balanced(int g0, int g1, const float* __restrict__ xys,
                                                    const int* __restrict__ radii,
                                                    const float4* __restrict__ splats, const ts_camera& cam,
                                                    Emit emit) {
    static_assert(kBinThreads == 1024, "one Gaussian per thread and batch, items packed as lt | row << 10");
    __shared__ float stash[kStashWords][kBinThreads];
    __shared__ int items[kItemCap];
    __shared__ int wave_sum[kBinThreads / 64 + 1];
    static_assert(sizeof(stash) + sizeof(items) + sizeof(wave_sum) <= kBalancedLds, "kBalancedLds states this walk's LDS");
    const int ws = cam.wide_tiles ? 1 : 0;
    const int tbx = (cam.tile_bounds_x + ws) >> ws;
    const bool tight_lists = splats != nullptr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int base = g0; base < g1; base += kBinThreads) {
        // ---- phase 1: one Gaussian per thread
        const int i = base + tid;
        int rows = 0;
        if (i < g1) {
            const int r = radii[i];
            if (r > 0) {
                const float2 xy = reinterpret_cast<const float2*>(xys)[i];
                float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
                if (tight_lists) { q0 = splats[3 * (size_t)i]; q1 = splats[3 * (size_t)i + 1]; }
                const ts::TileBox b = ts::tile_bbox(xy.x, xy.y, (float)r, cam.tile_bounds_x, cam.tile_bounds_y,
                                                    cam.tile_row0, cam.tile_rows);
                if (b.maxy > b.miny && b.maxx > b.minx) {
                    const TightTest t(tight_lists, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, (float)r);
                    if (!t.cull_all) {
                        rows = b.maxy - b.miny;
                        stash[0][tid] = t.geometric ? t.dymax : -1.0f;          // dymax >= 0 when geometric
                        stash[1][tid] = t.gx; stash[2][tid] = t.gy; stash[3][tid] = t.B; stash[4][tid] = t.D4;
                        stash[5][tid] = t.inv2A; stash[6][tid] = t.tau4A; stash[7][tid] = t.dxext;
                        stash[8][tid] = t.dy_left; stash[9][tid] = __int_as_float(b.miny);
                        stash[10][tid] = __int_as_float(b.minx | (b.maxx << 16));
                    }
                }
            }
        }
        // ---- exclusive scan of the row counts over the workgroup
        int incl = rows;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            int v = lane < kBinThreads / 64 ? wave_sum[lane] : 0;
#pragma unroll
            for (int d = 1; d < kBinThreads / 64; d <<= 1) {
                const int u = __shfl_up(v, d, 64);
                if (lane >= d) v += u;
            }
            if (lane < kBinThreads / 64) wave_sum[lane] = v;                     // inclusive over waves
        }
        __syncthreads();
        const int total = wave_sum[kBinThreads / 64 - 1];
        const int first = incl - rows + (wave > 0 ? wave_sum[wave - 1] : 0);   // this Gaussian's first item
        // ---- items in windows of kItemCap: written by their Gaussians, consumed by consecutive lanes
        for (int w0 = 0; w0 < total; w0 += kItemCap) {
            const int lo_k = max(0, w0 - first), hi_k = min(rows, w0 + kItemCap - first);
            for (int k = lo_k; k < hi_k; ++k) items[first + k - w0] = tid | (k << 10);
            __syncthreads();
            const int m = min(kItemCap, total - w0);
            for (int j = tid; j < m; j += kBinThreads) {
                const int it = items[j], lt = it & 1023, k = it >> 10;
                TightTest t(false, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
                const float d0 = stash[0][lt];
                t.geometric = d0 >= 0.0f;
                t.dymax = d0;
                t.gx = stash[1][lt]; t.gy = stash[2][lt]; t.B = stash[3][lt]; t.D4 = stash[4][lt];
                t.inv2A = stash[5][lt]; t.tau4A = stash[6][lt]; t.dxext = stash[7][lt]; t.dy_left = stash[8][lt];
                const int ty = __float_as_int(stash[9][lt]) + k;
                const int xx = __float_as_int(stash[10][lt]);
                int lo, hi;
                t.row_range(ty, xx & 0xffff, xx >> 16, lo, hi);
                if (hi <= lo) continue;
                emit_row(ty, lo, hi, base + lt, cam, ws, tbx, emit);
            }
            __syncthreads();
        }
        __syncthreads();          // wave_sum and the stash change hands (a batch without items has no barrier above)
    }
}

// grid = (chunks, windows); counts[b * T + t]
__global__ __launch_bounds__(kBinThreads) void bin_count_kernel(
    int n, int chunk, const float* __restrict__ xys, const int* __restrict__ radii,
    const float4* __restrict__ splats, const ts_camera cam, int num_tiles, int window,
    int* __restrict__ counts) {
    extern __shared__ int hist[];
    const int t0 = blockIdx.y * window;
    const int tw = min(num_tiles - t0, window);
    for (int j = threadIdx.x; j < tw; j += kBinThreads) hist[j] = 0;
    __syncthreads();
    const int g0 = blockIdx.x * chunk, g1 = min(n, g0 + chunk);
    auto emit = [&](int t, int) {
        t -= t0;
        if ((unsigned)t < (unsigned)tw) atomicAdd(&hist[t], 1);
    };
    // (the load-balanced walk does not pay for the count: 26 -> 28 us on config 3, 111 -> 149 us on config 5)
    walk_chunk(g0, g1, xys, radii, splats, cam, emit);
    __syncthreads();
    int* dst = counts + (size_t)blockIdx.x * num_tiles + t0;
    for (int j = threadIdx.x; j < tw; j += kBinThreads) dst[j] = hist[j];
}

constexpr int kScanGroups = 16;     // chunk groups of the column scan (waves of its workgroup)

// Column scan of the B x T count matrix in ONE launch: a workgroup owns 64 tile columns, its 16 waves own the
// 16 chunk groups; thread (tile, group) loads its <= kColPer counts (coalesced across the tiles of a wave, all
// loads issued before the first use), scans them in registers, the group sums of a tile are exchanged through LDS,
// and the thread writes the exclusive prefixes back.  tile_total[t] = column sum.  Replaces three launches
// (group sums, scan of the group sums, finish: ~6 us each on an in-order stream whatever their size).
constexpr int kColTiles = 64;
constexpr int kColPer = (kBinMaxChunks + kScanGroups - 1) / kScanGroups;      // 32 chunks per group at most
__global__ __launch_bounds__(kColTiles * kScanGroups) void column_scan_kernel(int num_tiles, int chunks,
                                                                              int per_group,
                                                                              int* __restrict__ counts,
                                                                              int* __restrict__ tile_total,
                                                                              bool write_bases) {
    __shared__ int gsum[kScanGroups][kColTiles];
    const int tl = threadIdx.x & (kColTiles - 1), g = threadIdx.x / kColTiles;
    const int t = blockIdx.x * kColTiles + tl;
    const int b0 = g * per_group, b1 = min(chunks, b0 + per_group);
    int c[kColPer];
    int sum = 0;
    if (t < num_tiles) {
#pragma unroll
        for (int j = 0; j < kColPer; ++j) c[j] = (b0 + j < b1) ? counts[(size_t)(b0 + j) * num_tiles + t] : 0;
#pragma unroll
        for (int j = 0; j < kColPer; ++j) {
            const int v = c[j];
            c[j] = sum;
            sum += v;
        }
    }
    gsum[g][tl] = sum;
    __syncthreads();
    if (t >= num_tiles) return;
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kScanGroups; ++q) {
        const int v = gsum[q][tl];
        if (q < g) base += v;
        tot += v;
    }
    if (write_bases) {                                     // (the ONE WALK form wants the totals only: its counts stay counts)
#pragma unroll
        for (int j = 0; j < kColPer; ++j)
            if (b0 + j < b1) counts[(size_t)(b0 + j) * num_tiles + t] = base + c[j];
    }
    if (g == 0) tile_total[t] = tot;
}

// single workgroup of 1024 threads, 8 tiles per lane and step (a 1080p frame's 8160 tiles in one step):
// exclusive scan over tiles -> tile_bins; tile_total[t] becomes start[t]
constexpr int kOffsetsThreads = 1024;
// CAPACITY GUARD: when the caller sized the per-intersection buffers from an estimate (capacity >= 0) instead of
// waiting for the count, a frame whose bounding-box total cum[n-1] exceeds it must not touch them: the guard word
// (spare[-1]) is set, every list is left empty (tile_bins = 0, tile_start = 0), ts_bin_scatter returns at once, and
// the compositing kernels find nothing to do; the host sees the same total when it reads the count and runs the
// frame again with exact sizes.
// One thread of an offsets launch (tile_offsets_kernel, group_tile_offsets_kernel) arms the guard: over (the workgroup's
// LDS word) = whether it tripped.  refuse_negative: a negative total trips it whatever the capacity
__device__ __forceinline__ void arm_guard(int& over, int* __restrict__ spare, const int* __restrict__ total_ptr,
                                          long long capacity, bool refuse_negative) {
    *spare = 0;                                           // the workspace's last word: ts_sort_tiles' tile counter
    over = (total_ptr && capacity >= 0 && ((long long)*total_ptr > capacity || *total_ptr < 0)) ? 1 : 0;
    if (refuse_negative && total_ptr && *total_ptr < 0) over = 1;
    spare[-1] = over;
}
// ... and where it tripped (or nothing is listed) the whole workgroup leaves every list empty
template <int THREADS>
__device__ __forceinline__ void empty_every_list(int num_tiles, int* __restrict__ tile_start, int* __restrict__ tile_bins) {
    for (int t = threadIdx.x; t <= num_tiles; t += THREADS) {
        tile_start[t] = 0;
        if (t < num_tiles) reinterpret_cast<int2*>(tile_bins)[t] = make_int2(0, 0);
    }
}
__global__ __launch_bounds__(kOffsetsThreads) void tile_offsets_kernel(int num_tiles,
                                                                       int* __restrict__ tile_total,
                                                                       int* __restrict__ tile_bins,
                                                                       int* __restrict__ spare,
                                                                       const int* __restrict__ total_ptr,
                                                                       long long capacity, int* __restrict__ longest_out) {
    constexpr int kPer = 8;
    __shared__ int carry, over, longest;
    int my_longest = 0;
    if (threadIdx.x == 0) {
        carry = 0;
        longest = 0;
        arm_guard(over, spare, total_ptr, capacity, /*refuse_negative=*/false);
    }
    __syncthreads();
    if (over) {
        empty_every_list<kOffsetsThreads>(num_tiles, tile_total, tile_bins);
        return;
    }
    for (int base = 0; base < num_tiles; base += kOffsetsThreads * kPer) {
        const int t0 = base + threadIdx.x * kPer;
        int v[kPer], sum = 0;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            v[e] = (t0 + e < num_tiles) ? tile_total[t0 + e] : 0;
            sum += v[e];
            my_longest = max(my_longest, v[e]);
        }
        int total;
        const int inc = block_inclusive_scan<kOffsetsThreads / 64>(sum, &total);
        int start = carry + inc - sum;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            if (t0 + e < num_tiles) {
                tile_total[t0 + e] = start;
                reinterpret_cast<int2*>(tile_bins)[t0 + e] =
                    v[e] > 0 ? make_int2(start, start + v[e]) : make_int2(0, 0);
            }
            start += v[e];
        }
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_total[num_tiles] = carry;     // tile_start[T]: end of the last bucket
    if (longest_out) {          // the longest list of the frame (a scene statistic for the caller's launch policy; may be mapped host memory)
        atomicMax(&longest, my_longest);                     // (LDS)
        __syncthreads();
        if (threadIdx.x == 0) *longest_out = longest;
    }
}

__global__ __launch_bounds__(kBinThreads) void bin_scatter_kernel(
    int n, int chunk, const float* __restrict__ xys,
    const int* __restrict__ radii, const float4* __restrict__ splats, const ts_camera cam,
    int num_tiles, int window, const int* __restrict__ bases, const int* __restrict__ tile_start,
    int* __restrict__ bucket_ids) {
    extern __shared__ int cursor[];
    if (tile_start[num_tiles + 1] != 0) return;              // capacity guard (tile_offsets_kernel)
    const int t0 = blockIdx.y * window;
    const int tw = min(num_tiles - t0, window);
    const int* src = bases + (size_t)blockIdx.x * num_tiles + t0;
    for (int j = threadIdx.x; j < tw; j += kBinThreads) cursor[j] = tile_start[t0 + j] + src[j];
    __syncthreads();
    const int g0 = blockIdx.x * chunk, g1 = min(n, g0 + chunk);
    walk_chunk(g0, g1, xys, radii, splats, cam, [&](int t, int i) {
        t -= t0;
        if ((unsigned)t < (unsigned)tw) bucket_ids[atomicAdd(&cursor[t], 1)] = i;
    });
}

// Two-level scatter.  The direct scatter above writes every 4-byte id to a different cache line (a chunk of
// 4096 Gaussians puts ~2 entries into each of 8160 buckets) from whichever XCD runs the chunk: the L2s hold
// partial lines of the same bucket and write them back separately - WRITE_SIZE measured 8x the id bytes
// (131 MB for 16 MB on config 3).  With a scratch buffer of I words the ids instead travel in two coalesced
// hops:
//   coarse  each chunk appends (id | tile-in-group << 27) to the region of the tile GROUP (kCoarseTiles = 32
//           consecutive lists) - a group's region is the concatenation of its tiles' buckets, so a chunk's
//           entries for it form one run of ~64 words;
//   fine    one workgroup per group streams its region and places the ids in the tiles' buckets with LDS
//           cursors: all of a bucket's lines are written by one workgroup, merge in one L2 and leave as full lines.
// Three forms of these launches exist, chosen per frame (frame.hip: list_form); the fine hop is one piece of code:
//   matrix    bin_count -> column_scan + tile_offsets -> scatter (direct, or coarse + fine): B x T counts
//   group     group_bin_count -> group_tile_offsets -> coarse<.., true> + fine_groups: B x G counts, two walks
//   one walk  emit -> group_tile_offsets<false> -> fine_runs: B x G counts and run starts, ONE walk; the coarse hop's
//             scattered 4-byte stores into ~G open runs become a linear copy of the chunk's region out of LDS
// Shared by the forms: the per-Gaussian walk (walk_one, through walk_chunk or the span walk's fallback; the balanced walk
// takes its row mapping), the guard and the emptying of every list in the offsets launches (arm_guard, empty_every_list),
// the fine hop (place_pass), and in the two emit kernels everything but what is staged and how it is placed (EmitChunk:
// emit_chunk_begin, stage_slot, emit_chunk_rows, emit_copy_out).
#ifndef TS_COARSE_SHIFT
#define TS_COARSE_SHIFT 5
#endif
constexpr int kCoarseShift = TS_COARSE_SHIFT;
constexpr int kCoarseTiles = 1 << kCoarseShift;
constexpr int kCoarseIdBits = 32 - kCoarseShift;            // ids below 2^27
#ifndef TS_TWO_HOP_FROM
#define TS_TWO_HOP_FROM (1 << 18)
#endif
constexpr int kTwoHopFrom = TS_TWO_HOP_FROM;
// THE predicate of the two-hop scatter, and therefore of the group form of count and offsets (below): a frame
// either runs all three launches in the group form or none
inline bool two_hop(int n) { return n >= kTwoHopFrom && n < (1 << kCoarseIdBits); }
// (a two-hop frame has at least four chunks: the group form keeps G + T + 1 words in front of the B x T words of
// the workspace that the matrix form fills)
static_assert(kTwoHopFrom >= 4096, "the group form's workspace layout needs bin_num_chunks(n) >= 4");

// GROUP COUNTS (ts_bin_count_groups -> ts_group_offsets -> ts_bin_scatter_groups).  The coarse hop of a two-hop frame
// consumes a base per (chunk, tile GROUP), and the fine hop streams the whole region of its group anyway - it can
// count its 32 lists itself.  So nobody needs the B x T matrix: the histogram has one counter per group of
// kCoarseTiles lists and the matrix is B x G (250 KB instead of 8 MB on a 1080p frame of 1 M Gaussians), written
// once, scanned by one workgroup, read once (the workspace: BinGeometry below).
// counts[b * groups + g]; same walk, same TightTest, same list index as bin_count_kernel.
__global__ __launch_bounds__(kBinThreads) void group_bin_count_kernel(
    int n, int chunk, const float* __restrict__ xys, const int* __restrict__ radii,
    const float4* __restrict__ splats, const ts_camera cam, int groups, int* __restrict__ counts) {
    extern __shared__ int hist[];
    for (int j = threadIdx.x; j < groups; j += kBinThreads) hist[j] = 0;
    __syncthreads();
    const int g0 = blockIdx.x * chunk, g1 = min(n, g0 + chunk);
    walk_chunk(g0, g1, xys, radii, splats, cam, [&](int t, int) { atomicAdd(&hist[t >> kCoarseShift], 1); });
    __syncthreads();
    int* dst = counts + (size_t)blockIdx.x * groups;
    for (int j = threadIdx.x; j < groups; j += kBinThreads) dst[j] = hist[j];
}

// Group offsets in ONE launch of one workgroup: exclusive prefix over the chunks of every group column (in place),
// exclusive prefix of the column totals -> tile_start[g * kCoarseTiles] (a group's region starts where its first
// list does), tile_start[T] = grand total, and tile_offsets_kernel's other duties: the sort counter word, the
// capacity guard, all lists emptied on overflow.  tile_bins and the tile_start entries inside a group are the fine
// hop's; a frame that lists nothing at all gets them here, because its caller may skip the scatter.
// Columns: thread (column, row group) of a 256 x 4 layout loads its <= kGoPer counts (coalesced across columns, all
// loads issued before the first use), scans them in registers; row-group sums meet in LDS.  Frames with more than
// 256 columns or 256 chunks take several such steps.  counts == nullptr: column_scan_kernel has run over the B x G
// matrix (B x G > kGoSingleMax ints: too many bytes for one CU's load path) and col_total holds its totals.
constexpr int kGoThreads = 1024;
constexpr int kGoCols = 256;
constexpr int kGoRows = kGoThreads / kGoCols;
constexpr int kGoPer = 64;
constexpr int kGoLdsGroups = 2048;
constexpr int kGoSingleMax = 1 << 17;
// BASES = false (ONE WALK, below): the counts are left as they are - every chunk already knows where it writes - and a
// negative total is refused whatever the capacity, because the emit launch in front has placed nothing for it.
template <bool BASES = true>
__global__ __launch_bounds__(kGoThreads) void group_tile_offsets_kernel(
    int num_tiles, int groups, int chunks, int* __restrict__ counts, const int* col_total,
    int* __restrict__ tile_start, int* __restrict__ tile_bins, int* __restrict__ spare,
    const int* __restrict__ total_ptr, long long capacity, int* __restrict__ longest_out) {
    __shared__ int rsum[kGoRows][kGoCols];
    __shared__ int gtot[kGoLdsGroups];
    __shared__ int carry, over;
    const int tid = threadIdx.x;
    if (tid == 0) {
        carry = 0;
        arm_guard(over, spare, total_ptr, capacity, /*refuse_negative=*/!BASES);
    }
    __syncthreads();
    if (!over) {
        const int* tot = col_total;
        if (counts && !BASES) {
            // column totals only: thread (column, row residue) adds every kGoRows-th count of its column
            const int gl = tid & (kGoCols - 1), r = tid / kGoCols;
#pragma unroll 1
            for (int c0 = 0; c0 < groups; c0 += kGoCols) {
                const int g = c0 + gl;
                int sum = 0;
                if (g < groups) {
#pragma unroll 8
                    for (int b = r; b < chunks; b += kGoRows) sum += counts[(unsigned int)(b * groups + g)];
                }
                rsum[r][gl] = sum;
                __syncthreads();
                if (r == 0 && g < groups) {
                    int all = 0;
#pragma unroll
                    for (int q = 0; q < kGoRows; ++q) all += rsum[q][gl];
                    gtot[g] = all;
                }
                __syncthreads();                           // rsum is rewritten by the next step
            }
            tot = gtot;
        } else if (counts) {
            const int gl = tid & (kGoCols - 1), r = tid / kGoCols;
#pragma unroll 1
            for (int c0 = 0; c0 < groups; c0 += kGoCols) {
                const int g = c0 + gl;
                int colbase = 0;                           // (the same in the kGoRows threads of a column)
#pragma unroll 1
                for (int r0 = 0; r0 < chunks; r0 += kGoRows * kGoPer) {
                    const int b0 = r0 + r * kGoPer;
                    int c[kGoPer];
                    int sum = 0;
                    const unsigned int col = (unsigned int)(b0 * groups + g);     // (B x G <= kGoSingleMax: 32 bits)
                    if (g < groups) {
#pragma unroll
                        for (int j = 0; j < kGoPer; ++j) c[j] = (b0 + j < chunks) ? counts[col + (unsigned int)(j * groups)] : 0;
#pragma unroll
                        for (int j = 0; j < kGoPer; ++j) {
                            const int v = c[j];
                            c[j] = sum;
                            sum += v;
                        }
                    }
                    rsum[r][gl] = sum;
                    __syncthreads();
                    int base = colbase, all = 0;
#pragma unroll
                    for (int q = 0; q < kGoRows; ++q) {
                        const int v = rsum[q][gl];
                        if (q < r) base += v;
                        all += v;
                    }
                    if (g < groups) {
#pragma unroll
                        for (int j = 0; j < kGoPer; ++j)
                            if (b0 + j < chunks) counts[col + (unsigned int)(j * groups)] = base + c[j];
                    }
                    colbase += all;
                    __syncthreads();                       // rsum is rewritten by the next step
                }
                if (r == 0 && g < groups) gtot[g] = colbase;
            }
            __syncthreads();
            tot = gtot;
        }
        for (int base = 0; base < groups; base += kGoThreads) {
            const int g = base + tid;
            const int v = g < groups ? tot[g] : 0;
            int total;
            const int inc = block_inclusive_scan<kGoThreads / 64>(v, &total);
            if (g < groups) tile_start[g << kCoarseShift] = carry + inc - v;
            __syncthreads();
            if (tid == 0) carry += total;
            __syncthreads();
        }
        if (tid == 0) tile_start[num_tiles] = carry;         // tile_start[T]: end of the last bucket
        if (carry != 0) return;
        if (tid == 0 && longest_out) *longest_out = 0;       // nothing listed: no later launch may come to say so
    }
    empty_every_list<kGoThreads>(num_tiles, tile_start, tile_bins);     // overflow, or nothing listed
}

template <bool BAL, bool GROUPS = false>
__global__ __launch_bounds__(kBinThreads) void bin_scatter_coarse_kernel(
    int n, int chunk, const float* __restrict__ xys, const int* __restrict__ radii,
    const float4* __restrict__ splats, const ts_camera cam, int num_tiles, const int* __restrict__ bases,
    const int* __restrict__ tile_start, int* __restrict__ scratch) {
    extern __shared__ int cursor[];
    if (tile_start[num_tiles + 1] != 0) return;              // capacity guard (tile_offsets_kernel)
    const int groups = (num_tiles + kCoarseTiles - 1) >> kCoarseShift;
    if (GROUPS) {
        // the chunk's row of the B x G base matrix: one value per cursor
        const int* src = bases + (size_t)blockIdx.x * groups;
        for (int g = threadIdx.x; g < groups; g += kBinThreads) cursor[g] = tile_start[g << kCoarseShift] + src[g];
    } else {
        // cursor[g] = start of the group's region + the entries earlier chunks put into the group's tiles; the chunk's
        // row of the base matrix is read coalesced by the whole workgroup and summed per group with LDS atomics
        const int* src = bases + (size_t)blockIdx.x * num_tiles;
        for (int g = threadIdx.x; g < groups; g += kBinThreads) cursor[g] = tile_start[g << kCoarseShift];
        __syncthreads();
        for (int t = threadIdx.x; t < num_tiles; t += kBinThreads) {
            const int v = src[t];
            if (v) atomicAdd(&cursor[t >> kCoarseShift], v);
        }
    }
    __syncthreads();
    const int g0 = blockIdx.x * chunk, g1 = min(n, g0 + chunk);
    auto emit = [&](int t, int i) {
        scratch[atomicAdd(&cursor[t >> kCoarseShift], 1)] = i | ((t & (kCoarseTiles - 1)) << kCoarseIdBits);
    };
    if (BAL) walk_chunk_balanced(g0, g1, xys, radii, splats, cam, emit);
    else walk_chunk(g0, g1, xys, radii, splats, cam, emit);
}

#ifndef TS_FINE_THREADS
#define TS_FINE_THREADS 1024
#endif
#ifndef TS_FINE_AHEAD
#define TS_FINE_AHEAD 8
#endif
constexpr int kFineThreads = TS_FINE_THREADS;
constexpr int kFineAhead = TS_FINE_AHEAD;
constexpr int kFinePass = kFineThreads * kFineAhead;     // entries handled together
// THE FINE HOP: one workgroup per tile group takes the group's entries in passes.  A pass is reordered by tile in LDS
// before it is written (rank inside the tile from a returning LDS atomic, tile offsets from a 32-entry scan), so that
// consecutive lanes store consecutive words of one bucket: with one 4-byte store per entry straight from the stream a
// wave's store touched ~32 different lines, and the kernel was bound by those write transactions (137 us for 250 MB on
// config 5), not by bytes.  The order inside a bucket is arbitrary, as before; ts_sort_tiles follows.
// The three kernels of the hop (one per form) share everything below and differ in two things only:
//   where the entries come from   one contiguous region of the scratch buffer (matrix and group forms), or one run per
//                                 chunk (one walk)
//   where the cursors come from   tile_start, which tile_offsets_kernel filled (matrix form), or the kernel's own count:
//                                 the tile-in-group sits in the top kCoarseShift bits of every scratch word, so the
//                                 workgroup counts its 32 lists, scans the counts and PUBLISHES what tile_offsets_kernel
//                                 publishes in the matrix form - tile_bins[t] ((0, 0) for an empty list), tile_start[t] -
//                                 plus the group's longest list.  A group of one pass is counted by the placing pass
//                                 itself (one read); a longer one is streamed twice (the second time out of the L2)
constexpr unsigned int kCoarseIdMask = (1u << kCoarseIdBits) - 1u;
struct FineGroup {                                       // LDS of a fine-hop workgroup beside the pass itself
    int cursor[kCoarseTiles];                            // next free word of every bucket of the group
    int hist[kCoarseTiles];                              // entries per list: of the group while it is counted, of a pass while it is placed
    int loff[kCoarseTiles + 1];                          // where a list's entries start in the reordered pass ...
    int gbase[kCoarseTiles];                             // ... and in bucket_ids
};
struct GroupLists {                                      // what a workgroup that counts its lists itself publishes
    int t0, t1, begin;                                   // the group's lists, and where its entries begin in bucket_ids
    int* tile_start;
    int* tile_bins;
    int* group_max;
};

// wave 0, lane t: c = entries of list t (0 beyond the 32 lists) -> entries of the lists before it
__device__ __forceinline__ int scan_lists(const int* hist, int t, int& c) {
    c = t < kCoarseTiles ? hist[t] : 0;
    int inc = c;                                         // inclusive scan over the first 32 lanes
#pragma unroll
    for (int d = 1; d < kCoarseTiles; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (t >= d) inc += o;
    }
    return inc - c;
}

// wave 0, lane t: list t of the group has c entries, ex in the lists before it
__device__ __forceinline__ void publish_lists(FineGroup& sh, const GroupLists& g, int t, int c, int ex) {
    const int s = g.begin + ex;
    if (t < g.t1 - g.t0) {
        sh.cursor[t] = s;
        if (t > 0) g.tile_start[g.t0 + t] = s;           // ([t0] is the group's start: there since the offsets launch)
        reinterpret_cast<int2*>(g.tile_bins)[g.t0 + t] = c > 0 ? make_int2(s, s + c) : make_int2(0, 0);
    }
    int longest = c;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) longest = max(longest, __shfl_xor(longest, d, 64));
    if (t == 0) g.group_max[blockIdx.x] = longest;
}

// a group counted ahead of its placing passes: sh.hist holds the lists' counts
__device__ __forceinline__ void publish_counted(FineGroup& sh, const GroupLists& g) {
    __syncthreads();
    if ((int)threadIdx.x < 64) {
        int c;
        const int ex = scan_lists(sh.hist, threadIdx.x, c);
        publish_lists(sh, g, threadIdx.x, c, ex);
        if ((int)threadIdx.x < kCoarseTiles) sh.hist[threadIdx.x] = 0;
    }
    __syncthreads();
}

// The ranks of a thread's ITEMS entries inside their lists while a pass is placed: two 16-bit ranks per register (a
// rank is < 65536: place_pass asserts the pass size)
template <int ITEMS>
struct PassRanks {
    unsigned int r[(ITEMS + 1) / 2];
    __device__ __forceinline__ PassRanks() {
#pragma unroll
        for (int u = 0; u < (ITEMS + 1) / 2; ++u) r[u] = 0u;
    }
    __device__ __forceinline__ void set(int u, int v) { r[u / 2] |= (unsigned int)v << (16 * (u & 1)); }
    __device__ __forceinline__ int get(int u) const { return (int)((r[u / 2] >> (16 * (u & 1))) & 0xffffu); }
};

// Places one pass of m <= ITEMS * kFineThreads entries, load(k) being entry k: rank inside the list by LDS atomic, the
// pass's offsets per list, the lists' cursors moved on, the pass reordered by tile in buf (LDS, one word per entry: the
// tile travels with the id) and stored with consecutive lanes on consecutive words.  publish: the pass is the whole
// group and its counts are the lists', published to g.  load may read buf (everything is loaded before anything is put).
// One representation of a pass for all three kernels: measured against ids[] + tiles[] with a rank per register,
// profiles/r20_one_fine_hop.txt.
template <int ITEMS, typename Load>
__device__ __forceinline__ void place_pass(FineGroup& sh, unsigned int* buf, int m, Load load, bool publish,
                                           const GroupLists& g, int* __restrict__ bucket_ids) {
    static_assert(ITEMS * kFineThreads <= 65536, "16-bit ranks inside a pass");
    const int tid = threadIdx.x;
    unsigned int w[ITEMS];
    PassRanks<ITEMS> rank;
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
        const int k = u * kFineThreads + tid;
        if (k < m) w[u] = load(k);
    }
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
        const int k = u * kFineThreads + tid;
        if (k < m) rank.set(u, atomicAdd(&sh.hist[w[u] >> kCoarseIdBits], 1));
    }
    __syncthreads();
    if (tid < 64) {                                                   // one wave: offsets of the pass, bases, reset
        int c;
        const int ex = scan_lists(sh.hist, tid, c);
        if (publish) publish_lists(sh, g, tid, c, ex);
        if (tid < kCoarseTiles) {
            sh.loff[tid] = ex;
            sh.gbase[tid] = sh.cursor[tid];
            sh.cursor[tid] += c;
            sh.hist[tid] = 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
        const int k = u * kFineThreads + tid;
        if (k < m) buf[sh.loff[w[u] >> kCoarseIdBits] + rank.get(u)] = w[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
        const int k = u * kFineThreads + tid;
        if (k < m) {
            const unsigned int e = buf[k];
            const int t = (int)(e >> kCoarseIdBits);
            bucket_ids[sh.gbase[t] + (k - sh.loff[t])] = (int)(e & kCoarseIdMask);
        }
    }
    __syncthreads();                                                  // buf and loff are rewritten by the next pass
}

// Fine hop of the MATRIX form: a linear region, cursors from tile_start.
__global__ __launch_bounds__(kFineThreads) void bin_scatter_fine_kernel(int num_tiles,
                                                                        const int* __restrict__ tile_start,
                                                                        const int* __restrict__ scratch,
                                                                        int* __restrict__ bucket_ids) {
    __shared__ FineGroup sh;
    __shared__ unsigned int buf[kFinePass];
    const int t0 = blockIdx.x << kCoarseShift, t1 = min(num_tiles, t0 + kCoarseTiles);
    if ((int)threadIdx.x < t1 - t0) sh.cursor[threadIdx.x] = tile_start[t0 + threadIdx.x];
    const int begin = tile_start[t0], end = tile_start[t1];
    if ((int)threadIdx.x < kCoarseTiles) sh.hist[threadIdx.x] = 0;
    __syncthreads();
    for (int c0 = begin; c0 < end; c0 += kFinePass)
        place_pass<kFineAhead>(sh, buf, min(kFinePass, end - c0),
                               [&](int k) { return (unsigned int)scratch[c0 + k]; }, false, GroupLists{}, bucket_ids);
}

// Fine hop of the GROUP form: a linear region of which the workgroup knows only where it begins and ends (tile_start at
// the group boundaries, group_tile_offsets_kernel); it counts its lists itself.
__global__ __launch_bounds__(kFineThreads) void bin_scatter_fine_groups_kernel(int num_tiles,
                                                                               int* __restrict__ tile_start,
                                                                               int* __restrict__ tile_bins,
                                                                               int* __restrict__ group_max,
                                                                               const int* __restrict__ scratch,
                                                                               int* __restrict__ bucket_ids) {
    if (tile_start[num_tiles + 1] != 0) return;          // capacity guard: every list was emptied already
    __shared__ FineGroup sh;
    __shared__ unsigned int buf[kFinePass];
    const int t0 = blockIdx.x << kCoarseShift, t1 = min(num_tiles, t0 + kCoarseTiles);
    const int begin = tile_start[t0], end = tile_start[t1];
    if ((int)threadIdx.x < kCoarseTiles) {
        sh.hist[threadIdx.x] = 0;
        sh.cursor[threadIdx.x] = 0;
    }
    __syncthreads();
    const GroupLists lists{t0, t1, begin, tile_start, tile_bins, group_max};
    const bool counted = end - begin > kFinePass || end == begin;
    if (counted) {
        for (int c0 = begin; c0 < end; c0 += kFinePass) {
            const int m = min(kFinePass, end - c0);
            unsigned int w[kFineAhead];
#pragma unroll
            for (int u = 0; u < kFineAhead; ++u) {
                const int k = u * kFineThreads + (int)threadIdx.x;
                if (k < m) w[u] = (unsigned int)scratch[c0 + k];
            }
#pragma unroll
            for (int u = 0; u < kFineAhead; ++u) {
                const int k = u * kFineThreads + (int)threadIdx.x;
                if (k < m) atomicAdd(&sh.hist[w[u] >> kCoarseIdBits], 1);
            }
        }
        publish_counted(sh, lists);
    }
    for (int c0 = begin; c0 < end; c0 += kFinePass)
        place_pass<kFineAhead>(sh, buf, min(kFinePass, end - c0),
                               [&](int k) { return (unsigned int)scratch[c0 + k]; }, !counted, lists, bucket_ids);
}

// ONE WALK (ts_bin_emit_groups -> ts_emit_offsets -> ts_bin_gather_groups).  The group form still walks every chunk
// twice with identical decisions: once to count, once to store at the bases the count gave.  A chunk's destination can
// be fixed before anything is counted: cum_tiles_hit gives every Gaussian a private range of bounding-box slots, the
// walk lists at most that many pairs per Gaussian (same ts::tile_bbox, row_range clamped to the box - what
// reduce_partials relies on for its row slots), and the scratch buffer is sized by the bounding-box total.  So chunk b
// writes its entries, ordered by group, contiguously from cum_tiles_hit[g0 - 1] on, and leaves two rows of B x G words:
// how many entries it has per group and where each of those runs starts.  The fine hop gathers its group's runs.
// During the walk an emitted pair bumps the chunk's per-group histogram and is appended to a staging buffer in LDS
// (one LDS atomic per wave and emit step: the active lanes take consecutive slots).  A chunk that fits the buffer
// scans the histogram and places the staged words; one that does not - the append notices, the histogram counts
// everything regardless - walks a second time and places from the then complete histogram: what two launches did.
#ifndef TS_STAGE_CAP
#define TS_STAGE_CAP 20480
#endif
constexpr int kStageCap = TS_STAGE_CAP;                  // staged pairs per chunk: 6 bytes each (word + group index)
constexpr int kEmitMaxGroups = 2048;                     // histogram + cursors: 8 bytes per group; 136 KiB in all
// dynamic LDS of an emit workgroup, as EmitChunk carves it: hist[groups], cursor[groups], words[kStageCap], grp[kStageCap]
constexpr size_t emit_lds_bytes(int groups) { return (size_t)groups * 8 + (size_t)kStageCap * 6; }
static_assert(emit_lds_bytes(kEmitMaxGroups) <= 144 * 1024, "LDS budget of a binning workgroup");
static_assert(kEmitMaxGroups <= 2 * kBinThreads && kEmitMaxGroups <= 65536, "two groups per thread, 16-bit group index");
static_assert(kEmitMaxGroups <= kGoLdsGroups, "the offsets launch keeps the column totals in LDS");

// THE WORKSPACE AND THE GEOMETRY of a frame's list building, derived once per entry from (n, num_tiles).  B chunks of
// `chunk` Gaussians, T lists, G groups of kCoarseTiles lists; every member below that names a place is a word offset into
// bin_ws, whose ts_bin_ws_ints(n, T) = (B + 1) T + 3 words are laid out as
//   all forms   [B*T .. B*T + T]         tile_start[T + 1]: where every list starts, [T] = all entries
//               [B*T + T + 1]            guard: set where the frame exceeds the caller's capacity (every list is left empty)
//               [B*T + T + 2]            spare: zero behind the offsets launch; ts_sort_tiles' counter of oversized tiles
//   matrix      [0 .. B*T)               counts[b][t] -> bases
//   group       [0 .. B*G)               counts[b][g] -> bases (dead once the coarse hop has run)
//               [B*G .. B*G + G)         group_totals: column totals where the columns are scanned by a launch of their own
//   one walk    [T+1+G .. +B*G)          counts[b][g]: entries of chunk b in group g
//               [.. +B*G)                starts[b][g]: where that run begins in the scratch buffer
//               [.. +G) = rows_end       col_total (only with the column-scan launch)
//   group and   [0 .. T+1)               what ts_sort_tiles may use (the bases are dead by then)
//   one walk    [T+1 .. T+1+G)           group_max: longest list of every group (fine hop -> the sort launch, ListStats)
// A two-hop frame has at least four chunks, so T + 1 + G words fit in front of tile_start; the one-walk rows fit where
// one_walk_form says so.
struct BinGeometry {
    int chunks, chunk, groups;
    long long tile_start, guard, spare;
    long long group_totals, group_max;
    long long counts, starts, col_total, rows_end;
};
inline BinGeometry bin_geometry(int n, int num_tiles) {
    const long long nt = num_tiles < 0 ? 0 : num_tiles;
    BinGeometry g;
    g.chunks = bin_num_chunks(n);
    g.chunk = n > 0 ? (n + g.chunks - 1) / g.chunks : 1;
    g.groups = (int)((nt + kCoarseTiles - 1) >> kCoarseShift);
    const long long rows = (long long)g.chunks * g.groups;
    g.tile_start = g.chunks * nt;
    g.guard = g.tile_start + nt + 1;
    g.spare = g.guard + 1;
    g.group_totals = rows;
    g.group_max = nt + 1;
    g.counts = g.group_max + g.groups;
    g.starts = g.counts + rows;
    g.col_total = g.starts + rows;
    g.rows_end = g.col_total + g.groups;
    return g;
}
// THE predicate of the one-walk form: a two-hop frame whose groups fit the emit launch's LDS and whose rows fit in
// front of tile_start
inline bool one_walk_form(int n, int num_tiles) {
    if (!two_hop(n) || num_tiles <= 0) return false;
    const BinGeometry g = bin_geometry(n, num_tiles);
    return g.groups <= kEmitMaxGroups && g.rows_end <= g.tile_start;
}

// SPAN WALK of the emit launch (row_spans.h).  The colour stage has left one 16-byte record per Gaussian with the tile
// columns of every row of its box - computed there by the very code walk_chunk runs, in the shadow of that launch's
// coefficient stream - so the walk here is one load per Gaussian, all kSpanPre of a thread up front, and two loops.  It
// reads neither xys nor radii nor the records, except for a Gaussian whose record says it is not representable (more
// than six rows, a column from 256 on): that lane computes the Gaussian as walk_chunk does.  The same lists as walk_chunk,
// emitted a run at a time.
constexpr int kSpanPre = 4;                              // a chunk of <= 4096 Gaussians in one round
template <typename Emit>
__device__ __forceinline__ void walk_gaussian(int i, const float* __restrict__ xys, const int* __restrict__ radii,
                                              const float4* __restrict__ splats, const ts_camera& cam, Emit emit) {
    const int ws = cam.wide_tiles ? 1 : 0;
    const int tbx = (cam.tile_bounds_x + ws) >> ws;
    const int r = radii[i];
    if (r <= 0) return;
    const float2 xy = reinterpret_cast<const float2*>(xys)[i];
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    if (splats) { q0 = splats[3 * (size_t)i]; q1 = splats[3 * (size_t)i + 1]; }
    walk_one(splats != nullptr, i, r, xy, q0, q1, cam, ws, tbx, emit);
}
// emit(t, len, i): the Gaussian enters the len <= 32 consecutive lists from t on, all of one group of kCoarseTiles lists -
// a row of a record is a run of consecutive lists already, cut here where it crosses into the next group.
template <typename Emit>
__device__ __forceinline__ void walk_spans(int g0, int g1, const int4* __restrict__ spans,
                                           const float* __restrict__ xys, const int* __restrict__ radii,
                                           const float4* __restrict__ splats, const ts_camera& cam, Emit emit) {
    const int ws = cam.wide_tiles ? 1 : 0;
    const int tbx = (cam.tile_bounds_x + ws) >> ws;
    for (int base = g0 + threadIdx.x; base < g1; base += kSpanPre * kBinThreads) {
        int4 rec[kSpanPre];
#pragma unroll
        for (int u = 0; u < kSpanPre; ++u) {
            const int i = base + u * kBinThreads;
            rec[u] = i < g1 ? spans[i] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kSpanPre; ++u) {
            ts::RowSpans s;
            s.w[0] = (unsigned int)rec[u].x; s.w[1] = (unsigned int)rec[u].y;
            s.w[2] = (unsigned int)rec[u].z; s.w[3] = (unsigned int)rec[u].w;
            const int rows = ts::spans_rows(s);
            if (rows == 0) continue;
            const int i = base + u * kBinThreads;
            if (rows == ts::kSpanFallback) {
                walk_gaussian(i, xys, radii, splats, cam, [&](int t, int id) { emit(t, 1, id); });
                continue;
            }
            int t0 = ts::spans_first_row(s) * tbx;       // first list of the row
            for (int k = 0; k < rows; ++k, t0 += tbx) {
                int lo, hi;
                ts::spans_pop_row(s, lo, hi);
                if (hi <= lo) continue;
                const int last = t0 + ((hi - 1) >> ws);
                for (int t = t0 + (lo >> ws); t <= last;) {
                    const int len = min(last - t + 1, kCoarseTiles - (t & (kCoarseTiles - 1)));
                    emit(t, len, i);
                    t += len;
                }
            }
        }
    }
}

// THE CHUNK EPILOGUE (and prologue) of the two emit kernels below, which differ in what they walk, in what a staged item
// is (a pair, a run) and therefore in how staged items are placed, and in nothing else.
struct EmitChunk {
    int g0, g1;                                          // the chunk's Gaussians
    int chunk_base, room;                                // its bounding-box slots in the scratch buffer: first, how many
    int* hist;                                           // [groups] what the chunk lists per group
    int* cursor;                                         // [groups] next free word of a group's run, from chunk_base
    unsigned int* words;                                 // [kStageCap] the staged words; then the region ordered by group
    unsigned short* grp;                                 // [kStageCap] a staged word's group (+ the kernel's own bits)
};
constexpr int kStagePer = kStageCap / kBinThreads;       // staged words per thread
static_assert(kStageCap % kBinThreads == 0, "whole staging rounds");

// Chunk bounds, the LDS carve-up (emit_lds_bytes), histogram and append counter cleared.  False: the frame trips the
// capacity guard and the launch places nothing
__device__ __forceinline__ bool emit_chunk_begin(EmitChunk& c, int* lds, int* staged, int n, int chunk, int groups,
                                                 const int* __restrict__ cum, long long capacity) {
    // capacity guard, read here because the offsets launch runs behind this one; a wrapped total places nothing either.
    // (The three words of cum_tiles_hit are in flight together, while the histogram is cleared)
    c.g0 = min(n, (int)blockIdx.x * chunk);
    c.g1 = min(n, c.g0 + chunk);
    const int total = cum[n - 1];
    c.chunk_base = c.g0 > 0 ? cum[c.g0 - 1] : 0;
    const int chunk_end = c.g1 > c.g0 ? cum[c.g1 - 1] : c.chunk_base;
    c.hist = lds;
    c.cursor = lds + groups;
    c.words = reinterpret_cast<unsigned int*>(lds + 2 * groups);
    c.grp = reinterpret_cast<unsigned short*>(c.words + kStageCap);
    for (int j = threadIdx.x; j < groups; j += kBinThreads) c.hist[j] = 0;
    if (threadIdx.x == 0) *staged = 0;
    __syncthreads();
    c.room = chunk_end - c.chunk_base;
    return total < 0 || (capacity >= 0 && (long long)total > capacity);
}

// The append of one staged item: one LDS atomic per wave and emit step, the active lanes take consecutive slots (a slot
// from kStageCap on is not stored: the chunk will walk a second time)
__device__ __forceinline__ int stage_slot(int* staged) {
    const unsigned long long m = __ballot(1);                         // the lanes that emit in this step
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    int base = 0;
    if (rank == 0) base = atomicAdd(staged, (int)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);                      // (the first active lane is the one of rank 0)
    return base + rank;
}

// Behind the walk: exclusive scan of the histogram, two groups per thread -> the cursors and the chunk's two rows.
// Returns everything the chunk lists (the histogram's total).  sound: a chunk cannot list more than its bounding-box
// slots; were it ever to, it lists nothing (zero counts) rather than write beyond its region
__device__ __forceinline__ int emit_chunk_rows(const EmitChunk& c, int groups, int* __restrict__ counts,
                                               int* __restrict__ starts, bool& sound) {
    __syncthreads();
    const int a = 2 * threadIdx.x;
    const int h0 = a < groups ? c.hist[a] : 0, h1 = a + 1 < groups ? c.hist[a + 1] : 0;
    int pairs;
    const int ex = block_inclusive_scan<kBinThreads / 64>(h0 + h1, &pairs) - h0 - h1;
    sound = pairs <= c.room;
    int* crow = counts + (size_t)blockIdx.x * groups;
    int* srow = starts + (size_t)blockIdx.x * groups;
    if (a < groups) {
        c.cursor[a] = ex;
        crow[a] = sound ? h0 : 0;
        srow[a] = c.chunk_base + ex;
    }
    if (a + 1 < groups) {
        c.cursor[a + 1] = ex + h0;
        crow[a + 1] = sound ? h1 : 0;
        srow[a + 1] = c.chunk_base + ex + h0;
    }
    __syncthreads();
    return pairs;
}

// The chunk's region, ordered by group in c.words, goes out: consecutive lanes store consecutive words
__device__ __forceinline__ void emit_copy_out(const EmitChunk& c, int pairs, int* __restrict__ dst) {
#pragma unroll
    for (int u = 0; u < kStagePer; ++u) {
        const int j = u * kBinThreads + (int)threadIdx.x;
        if (j < pairs) dst[j] = (int)c.words[j];
    }
}

__global__ __launch_bounds__(kBinThreads) void bin_scatter_emit_kernel(
    int n, int chunk, const float* __restrict__ xys, const int* __restrict__ radii,
    const float4* __restrict__ splats, const ts_camera cam, int groups, const int* __restrict__ cum,
    long long capacity, int* __restrict__ counts, int* __restrict__ starts, int* __restrict__ scratch) {
    extern __shared__ int lds[];
    __shared__ int staged;
    EmitChunk c;
    if (emit_chunk_begin(c, lds, &staged, n, chunk, groups, cum, capacity)) return;      // over capacity
    walk_chunk(c.g0, c.g1, xys, radii, splats, cam, [&](int t, int i) {
        const int g = t >> kCoarseShift;
        atomicAdd(&c.hist[g], 1);
        const int slot = stage_slot(&staged);
        if (slot < kStageCap) {
            c.words[slot] = (unsigned int)i | ((unsigned int)(t & (kCoarseTiles - 1)) << kCoarseIdBits);
            c.grp[slot] = (unsigned short)g;
        }
    });
    bool sound;
    const int pairs = emit_chunk_rows(c, groups, counts, starts, sound);      // (= staged: one pair per append)
    if (!sound) return;
    int* dst = scratch + c.chunk_base;
    if (pairs <= kStageCap) {
        // ordered by group inside LDS first (every thread keeps its entries and their places in registers while the
        // buffer changes hands), then copied out: consecutive lanes store consecutive words of the chunk's region.
        // Straight from the staging order a wave's store touched up to 64 lines, 16 k such words in one burst
        const int tid = threadIdx.x;
        unsigned int w[kStagePer];
        int at[kStagePer];
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            const int j = u * kBinThreads + tid;
            if (j < pairs) {
                w[u] = c.words[j];
                at[u] = atomicAdd(&c.cursor[c.grp[j]], 1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kStagePer; ++u)
            if (u * kBinThreads + tid < pairs) c.words[at[u]] = w[u];
        __syncthreads();
        emit_copy_out(c, pairs, dst);
    } else {
        walk_chunk(c.g0, c.g1, xys, radii, splats, cam, [&](int t, int i) {
            dst[atomicAdd(&c.cursor[t >> kCoarseShift], 1)] = i | ((t & (kCoarseTiles - 1)) << kCoarseIdBits);
        });
    }
}

// The emit launch over SPAN RECORDS: bin_scatter_emit_kernel with walk_spans in both of its walks and ONE STAGED ITEM PER
// RUN.  (A kernel of its own beside the one above, not a template of it: run staging in the shared body cost the
// launch without records 2.4 us, profiles/r26_row_spans.txt.  That covers what is staged and how it is placed, and those
// are what the two kernels spell out; the rest is the EmitChunk pieces, profiles/r27_binning_shared.txt.)
__global__ __launch_bounds__(kBinThreads) void bin_scatter_spans_kernel(
    int n, int chunk, const float* __restrict__ xys, const int* __restrict__ radii,
    const float4* __restrict__ splats, const int4* __restrict__ spans, const ts_camera cam, int groups,
    const int* __restrict__ cum, long long capacity, int* __restrict__ counts, int* __restrict__ starts,
    int* __restrict__ scratch) {
    extern __shared__ int lds[];
    __shared__ int staged;
    EmitChunk c;
    if (emit_chunk_begin(c, lds, &staged, n, chunk, groups, cum, capacity)) return;      // over capacity
    auto walk = [&](auto emit) { walk_spans(c.g0, c.g1, spans, xys, radii, splats, cam, emit); };     // emit(t, len, i)
    // ONE STAGED ITEM PER RUN: the word carries the id and the first tile-in-group, the 5 spare bits of the 16-bit group
    // index carry len - 1; the histogram takes the whole run in one atomic, the append happens once per run
    static_assert(kEmitMaxGroups <= (1 << 11) && kCoarseTiles <= 32, "group index in 11 bits, len - 1 in 5");
    walk([&](int t, int len, int i) {
        const int g = t >> kCoarseShift;
        atomicAdd(&c.hist[g], len);
        const int slot = stage_slot(&staged);
        if (slot < kStageCap) {
            c.words[slot] = (unsigned int)i | ((unsigned int)(t & (kCoarseTiles - 1)) << kCoarseIdBits);
            c.grp[slot] = (unsigned short)(g | ((len - 1) << 11));
        }
    });
    bool sound;
    const int pairs = emit_chunk_rows(c, groups, counts, starts, sound);
    const int items = staged;                                         // runs the chunk lists
    if (!sound) return;
    int* dst = scratch + c.chunk_base;
    if (items <= kStageCap && pairs <= kStageCap) {
        // bin_scatter_emit_kernel's placement, a run at a time
        const int tid = threadIdx.x;
        unsigned int w[kStagePer];
        int at[kStagePer];                                            // place of the run's first word | (len - 1) << 16
        static_assert(kStageCap <= 65536, "a place in 16 bits");
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            const int j = u * kBinThreads + tid;
            if (j < items) {
                w[u] = c.words[j];
                const int gl = c.grp[j], len1 = gl >> 11;
                at[u] = atomicAdd(&c.cursor[gl & 2047], len1 + 1) | (len1 << 16);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kStagePer; ++u)
            if (u * kBinThreads + tid < items) {
                // the run expanded into its words: tile-in-group first, first + 1, ... (<= 31: a run ends with its group)
                const int first = at[u] & 0xffff, len1 = at[u] >> 16;
                for (int q = 0; q <= len1; ++q) c.words[first + q] = w[u] + ((unsigned int)q << kCoarseIdBits);
            }
        __syncthreads();
        emit_copy_out(c, pairs, dst);
    } else {
        walk([&](int t, int len, int i) {
            const int at = atomicAdd(&c.cursor[t >> kCoarseShift], len);
            for (int q = 0; q < len; ++q) dst[at + q] = i | (((t + q) & (kCoarseTiles - 1)) << kCoarseIdBits);
        });
    }
}

// Fine hop of the ONE WALK form: the group's entries are one run per chunk (starts[b][g], counts[b][g]) instead of one
// region, and the workgroup counts its lists itself.  The run table goes to LDS (one chunk per thread, a workgroup scan of
// the lengths); a pass of kRunPass entries is gathered into LDS by whole waves, a run at a time and kRunAhead runs in
// flight per wave, and placed from there.  A group of more than one pass counts its lists from the runs first.
#ifndef TS_RUN_AHEAD
#define TS_RUN_AHEAD 20
#endif
constexpr int kRunItems = TS_RUN_AHEAD;                  // entries per thread and pass
constexpr int kRunPass = kFineThreads * kRunItems;       // 20480 entries, 80 KiB: config 3's ~16 k per group in one pass
                                                         // (24 items per thread spill registers at 1024 threads)
#ifndef TS_RUNS_IN_FLIGHT
#define TS_RUNS_IN_FLIGHT 8
#endif
constexpr int kRunAhead = TS_RUNS_IN_FLIGHT;             // runs a wave has in flight
__global__ __launch_bounds__(kFineThreads) void bin_scatter_fine_runs_kernel(
    int num_tiles, int groups, int chunks, const int* __restrict__ counts, const int* __restrict__ starts,
    int* __restrict__ tile_start, int* __restrict__ tile_bins, int* __restrict__ group_max,
    const int* __restrict__ scratch, int* __restrict__ bucket_ids) {
    extern __shared__ unsigned int buf[];                // kRunPass words: the pass, then the pass ordered by tile
    // (the group's column of the two matrices is asked for before the guard word is looked at: stale words where the
    // guard tripped, never used)
    const int my_count = (int)threadIdx.x < chunks ? counts[(size_t)threadIdx.x * groups + blockIdx.x] : 0;
    const int my_start = (int)threadIdx.x < chunks ? starts[(size_t)threadIdx.x * groups + blockIdx.x] : 0;
    const int begin = tile_start[min(num_tiles, (int)(blockIdx.x << kCoarseShift))];
    if (tile_start[num_tiles + 1] != 0) return;          // capacity guard: every list was emptied already
    __shared__ FineGroup sh;
    __shared__ int roff[kBinMaxChunks + 1], rsrc[kBinMaxChunks];
    constexpr int kWaves = kFineThreads / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x << kCoarseShift, t1 = min(num_tiles, t0 + kCoarseTiles);
    if (tid < kCoarseTiles) {
        sh.hist[tid] = 0;
        sh.cursor[tid] = 0;
    }
    int total;
    {
        const int c = my_count;
        const int inc = block_inclusive_scan<kWaves>(c, &total);
        if (tid < chunks) {
            roff[tid] = inc - c;
            rsrc[tid] = my_start;
        }
        if (tid == 0) roff[chunks] = total;
    }
    __syncthreads();
    // the window [c0, c0 + m) of the group's entries, run by run: op(position in the window, scratch word)
    auto for_runs = [&](int c0, int m, auto op) {
#pragma unroll 1
        for (int b0 = wave; b0 < chunks; b0 += kWaves * kRunAhead) {
            int len[kRunAhead], src[kRunAhead], dst[kRunAhead];         // this lane's first entry of the run and what is left
            unsigned int v[kRunAhead];
#pragma unroll
            for (int u = 0; u < kRunAhead; ++u) {
                const int b = b0 + u * kWaves;
                len[u] = src[u] = dst[u] = 0;
                if (b < chunks) {
                    const int o = roff[b], c = roff[b + 1] - o;
                    const int lo = max(0, c0 - o) + lane;
                    len[u] = min(c, c0 + m - o) - lo;
                    src[u] = rsrc[b] + lo;
                    dst[u] = o - c0 + lo;
                }
            }
#pragma unroll
            for (int u = 0; u < kRunAhead; ++u)
                if (len[u] > 0) v[u] = (unsigned int)scratch[src[u]];
#pragma unroll
            for (int u = 0; u < kRunAhead; ++u)
                if (len[u] > 0) op(dst[u], v[u]);
#pragma unroll
            for (int u = 0; u < kRunAhead; ++u)
                for (int j = 64; j < len[u]; j += 64) op(dst[u] + j, (unsigned int)scratch[src[u] + j]);
        }
    };
    const GroupLists lists{t0, t1, begin, tile_start, tile_bins, group_max};
    const bool counted = total > kRunPass || total == 0;
    if (counted) {
        for_runs(0, total, [&](int, unsigned int w) { atomicAdd(&sh.hist[w >> kCoarseIdBits], 1); });
        publish_counted(sh, lists);
    }
    for (int c0 = 0; c0 < total; c0 += kRunPass) {
        const int m = min(kRunPass, total - c0);                      // entries of this pass
        for_runs(c0, m, [&](int k, unsigned int w) { buf[k] = w; });
        __syncthreads();
        place_pass<kRunItems>(sh, buf, m, [&](int k) { return buf[k]; }, !counted, lists, bucket_ids);
    }
}

// The frame's longest list in the group form: the fine hop left one maximum per group, and the first workgroup of
// the sort launch that follows it anyway reduces them into the caller's word (no launch of its own, no device-scope
// atomics).  Nothing is stored for a frame that tripped the capacity guard, as in the matrix form.
struct ListStats {
    const int* group_max;       // null: no statistic asked for
    const int* guard;
    int* longest_out;
    int groups;
};
__device__ __forceinline__ void store_longest(const ListStats& st) {
    __shared__ int longest;
    if (threadIdx.x == 0) longest = 0;
    __syncthreads();
    int m = 0;
    for (int g = threadIdx.x; g < st.groups; g += kThreads) m = max(m, st.group_max[g]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&longest, m);             // (LDS)
    __syncthreads();
    if (threadIdx.x == 0 && *st.guard == 0) *st.longest_out = longest;
}

// ---- per-tile bitonic sort ---------------------------------------------------------------------
constexpr int kSortCap = 4096;   // keys held in LDS (32 KiB); larger buckets sort in global memory

#include "sort_network.h"

struct IdKeyArray {                 // in-place view of a bucket of ids compared through their keys
    volatile int* ids;
    const float* depths;
};

__device__ __forceinline__ void cmpswap(IdKeyArray a, int i, int j) {
    const int x = a.ids[i], y = a.ids[j];
    if (make_key(a.depths, x) > make_key(a.depths, y)) { a.ids[i] = y; a.ids[j] = x; }
}

template <typename Ptr>
__device__ __forceinline__ void bitonic_network(Ptr a, int n) {
    int lg = 0;                                   // npad = 2^lg >= n
    while ((1 << lg) < n) ++lg;
    const int half = (1 << lg) >> 1;
    // all strides are powers of two: index arithmetic is shifts and masks (no integer division)
    for (int lk = 1; lk <= lg; ++lk) {            // merge blocks of size k = 2^lk
        const int k = 1 << lk, hk = k >> 1;
        for (int p = threadIdx.x; p < half; p += kThreads) {          // flip
            const int base = (p >> (lk - 1)) << lk, off = p & (hk - 1);
            const int i = base + off, j = base + k - 1 - off;
            if (j < n) cmpswap(a, i, j);
        }
        __syncthreads();
        for (int ld = lk - 2; ld >= 0; --ld) {                        // disperse, stride d = 2^ld
            const int d = 1 << ld;
            for (int p = threadIdx.x; p < half; p += kThreads) {
                const int i = ((p >> ld) << (ld + 1)) | (p & (d - 1)), j = i + d;
                if (j < n) cmpswap(a, i, j);
            }
            __syncthreads();
        }
    }
}

// Register-resident bitonic sort of one bucket of ids by the whole workgroup (n <= 256 E): in-thread
// stages are pure register work, in-wave stages 64-bit lane exchanges through the LDS crossbar, and
// only partner distances >= 64 E (at most 3 of the 55 stages of a 1024-key sort) take an LDS round
// trip with a barrier.  `g` and `out` may alias (everything is loaded before anything is stored).
template <int E>
__device__ __forceinline__ void sort_tile_regs(const int* g, const float* __restrict__ depths,
                                               int* out, int n, unsigned long long* lds) {
    const int t = threadIdx.x;
    unsigned long long k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t * E + e;
        k[e] = i < n ? make_key(depths, g[i]) : ~0ull;
    }
    __syncthreads();                                  // aliasing callers: all loads before any store
    bitonic_regs<E, kThreads>(k, t, min(pow2_at_least(n), kThreads * E), lds);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t * E + e;
        if (i < n) out[i] = (int)(unsigned int)k[e];
    }
}

__device__ __forceinline__ void sort_bucket_block(const int* g, const float* __restrict__ depths,
                                                  int* out, int n, unsigned long long* lds) {
    if (n <= kThreads) sort_tile_regs<1>(g, depths, out, n, lds);
    else if (n <= 2 * kThreads) sort_tile_regs<2>(g, depths, out, n, lds);
    else if (n <= 4 * kThreads) sort_tile_regs<4>(g, depths, out, n, lds);
    else if (n <= 8 * kThreads) sort_tile_regs<8>(g, depths, out, n, lds);
    else sort_tile_regs<16>(g, depths, out, n, lds);
}

// Tiles of more than kSampleMin keys (beyond the register network): per-tile SAMPLE SORT,
// O(n log n), streaming the tile's ids from global memory.  Measured on config 5 (2.5 k keys per
// tile) the network with its 16 independent keys per lane is 3x faster than this latency-chained
// scheme, so the network keeps every tile it can hold; the sample sort is the robust path for very
// dense tiles, replacing a global-memory network whose every stage is a barrier plus HBM round trips.
//   1. a regular sample of NS keys (256, or 1024 for n > 8192) is sorted with the network;
//   2. B - 1 splitters taken evenly from the sorted sample cut the key range into B sub-buckets of
//      ~96 keys on average (keys are unique, so equal depths cannot pile up in one sub-bucket);
//   3. two passes over the tile's ids: LDS histogram of sub-bucket sizes, then LDS cursors scatter
//      the ids into `out` grouped by sub-bucket;
//   4. each wave sorts whole sub-buckets (<= 256 keys) on its own, in place; the rare larger ones are
//      sorted afterwards by the whole workgroup.
// LDS (u64 units): scratch[4096] sample[1024] tables[1024] = 48 KiB.
// tiles up to kSortCap keys use the plain network (one wave up to kWaveSortMax, the workgroup beyond)
constexpr int kMaxSub = 512;              // sub-buckets per tile
constexpr int kSubTarget = 96;            // mean keys per sub-bucket aimed at
constexpr int kLargeLdsU64 = kSortCap + 2048;

__device__ __forceinline__ void sort_tile_sample(const int* __restrict__ g,
                                                 const float* __restrict__ depths,
                                                 int* __restrict__ out, int n,
                                                 unsigned long long* lds) {
    unsigned long long* scratch = lds;
    unsigned long long* smp = lds + kSortCap;
    int* start = reinterpret_cast<int*>(lds + kSortCap + 1024);       // [kMaxSub + 1]
    int* cursor = start + (kMaxSub + 1);                              // [kMaxSub]
    int* big = cursor + kMaxSub;                                      // [kMaxSub] oversize list
    __shared__ int nbig;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ns = n > 8192 ? 1024 : 256;
    int nb = n / kSubTarget;
    nb = nb < 2 ? 2 : (nb > kMaxSub ? kMaxSub : nb);

    if (ns == 1024) {                                                 // sorted sample
        unsigned long long k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            k[e] = make_key(depths, g[(int)(((long long)(t * 4 + e) * n) >> 10)]);
        bitonic_regs<4, kThreads>(k, t, 1024, scratch);
#pragma unroll
        for (int e = 0; e < 4; ++e) smp[t * 4 + e] = k[e];
    } else {
        unsigned long long k[1];
        k[0] = make_key(depths, g[(int)(((long long)t * n) >> 8)]);
        bitonic_regs<1, kThreads>(k, t, 256, scratch);
        smp[t] = k[0];
    }
    for (int b = t; b < nb; b += kThreads) cursor[b] = 0;
    if (t == 0) nbig = 0;
    __syncthreads();

    // sub-bucket of a key = number of splitters <= key; splitter j = smp[((j + 1) * ns) / nb]
    auto sub_of = [&](unsigned long long key) {
        int lo = 0, hi = nb - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (smp[((mid + 1) * ns) / nb] <= key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    for (int i = t; i < n; i += kThreads) atomicAdd(&cursor[sub_of(make_key(depths, g[i]))], 1);
    __syncthreads();
    {   // exclusive scan of nb <= 512 counts: two per thread
        const int c0 = (2 * t < nb) ? cursor[2 * t] : 0, c1 = (2 * t + 1 < nb) ? cursor[2 * t + 1] : 0;
        int total;
        const int inc = block_inclusive_scan(c0 + c1, &total);
        const int ex = inc - (c0 + c1);
        if (2 * t < nb) start[2 * t] = ex;
        if (2 * t + 1 < nb) start[2 * t + 1] = ex + c0;
        if (t == 0) start[nb] = n;
    }
    __syncthreads();
    for (int b = t; b < nb; b += kThreads) cursor[b] = start[b];
    __syncthreads();
    for (int i = t; i < n; i += kThreads) {
        const int id = g[i];
        out[atomicAdd(&cursor[sub_of(make_key(depths, id))], 1)] = id;
    }
    __threadfence_block();
    __syncthreads();
    for (int b = wave; b < nb; b += kThreads / 64) {                 // wave-level sorts, in place
        const int s0 = start[b], m = start[b + 1] - s0;
        if (m <= 1) continue;
        if (m <= 256) {
            unsigned long long k[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = lane * 4 + e;
                k[e] = i < m ? make_key(depths, out[s0 + i]) : ~0ull;
            }
            bitonic_regs<4, 64>(k, lane, min(pow2_at_least(m), 256), nullptr);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = lane * 4 + e;
                if (i < m) out[s0 + i] = (int)(unsigned int)k[e];
            }
        } else if (lane == 0) {
            big[atomicAdd(&nbig, 1)] = b;
        }
    }
    __syncthreads();
    const int nbg = nbig;
    for (int q = 0; q < nbg; ++q) {                                   // rare: oversize sub-buckets
        const int b = big[q];
        const int s0 = start[b], m = start[b + 1] - s0;
        __syncthreads();
        if (m <= kSortCap) {
            sort_bucket_block(out + s0, depths, out + s0, m, scratch);
        } else {
            IdKeyArray a{out + s0, depths};
            bitonic_network(a, m);
        }
        __syncthreads();
    }
}

// Three launches: the first kernel gives every tile of up to kWaveSortMax keys to one wave (four tiles per
// workgroup) and queues those beyond kSortCap; the second sorts the tiles in between with one workgroup per
// tile; the third walks the queue (sample sort).
__global__ __launch_bounds__(kThreads) void sort_tiles_small_kernel(
    int num_tiles, const int* __restrict__ tile_bins, const float* __restrict__ depths,
    const int* __restrict__ bucket_ids, int* __restrict__ ids_sorted, int* __restrict__ large_count,
    int* __restrict__ large_list, const ListStats stats) {
    if (stats.group_max && blockIdx.x == 0) store_longest(stats);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (tile >= num_tiles) return;
    const int2 range = reinterpret_cast<const int2*>(tile_bins)[tile];
    const int n = range.y - range.x;
    if (n <= 0) return;
    if (n > kWaveSortMax) {                      // (kWaveSortMax, kSortCap]: sort_tiles_mid_kernel; beyond: queued
        if (n > kSortCap && lane == 0) large_list[atomicAdd(large_count, 1)] = tile;
        return;
    }
    const int* g = bucket_ids + range.x;
    int* out = ids_sorted + range.x;
    if (n <= 64) sort_tile_wave<1>(g, depths, out, n, lane);
    else if (n <= 128) sort_tile_wave<2>(g, depths, out, n, lane);
    else if (n <= 256) sort_tile_wave<4>(g, depths, out, n, lane);
    else if (n <= 512) sort_tile_wave<8>(g, depths, out, n, lane);
    else sort_tile_wave<16>(g, depths, out, n, lane);
}

// Tiles beyond one wave's network.  Up to kSortCap keys: one workgroup per tile, the register network with LDS
// for the cross-wave stages (32 KiB of LDS: five workgroups per CU), launched over ALL tiles - a workgroup whose
// tile belongs to another kernel leaves at once.  Walking a queue of such tiles from a persistent grid instead
// (one launch for everything above a wave's network, tried in round 3) saved 5 us on config 3 and ran config 5's
// sort - 14 k tiles of ~1 900 keys - at 0.78 - 0.89 instead of 0.55 ms.  Beyond kSortCap: the sample sort
// (48 KiB), a small persistent grid over the queue that sort_tiles_small_kernel filled.
// large_count / large_list (ts_sort_tiles_above: no sort_tiles_small_kernel runs): this kernel queues the tiles
// beyond kSortCap for the sample sort itself.
__global__ __launch_bounds__(kThreads) void sort_tiles_mid_kernel(
    const int* __restrict__ tile_bins, const float* __restrict__ depths,
    const int* __restrict__ bucket_ids, int* __restrict__ ids_sorted, int* __restrict__ large_count,
    int* __restrict__ large_list) {
    __shared__ unsigned long long lk[kSortCap / 2];
    const int2 range = reinterpret_cast<const int2*>(tile_bins)[blockIdx.x];
    const int n = range.y - range.x;
    if (n > kSortCap && large_count && threadIdx.x == 0) large_list[atomicAdd(large_count, 1)] = blockIdx.x;
    if (n <= kWaveSortMax || n > kSortCap) return;
    sort_bucket_block(bucket_ids + range.x, depths, ids_sorted + range.x, n, lk);
}

__global__ __launch_bounds__(kThreads) void sort_tiles_large_kernel(
    const int* __restrict__ tile_bins, const float* __restrict__ depths,
    const int* __restrict__ bucket_ids, int* __restrict__ ids_sorted,
    const int* __restrict__ large_count, const int* __restrict__ large_list) {
    __shared__ unsigned long long lds_large[kLargeLdsU64];
    const int count = *large_count;
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int2 range = reinterpret_cast<const int2*>(tile_bins)[large_list[q]];
        const int n = range.y - range.x;
        if (n <= kSortCap) continue;
        __syncthreads();
        sort_tile_sample(bucket_ids + range.x, depths, ids_sorted + range.x, n, lds_large);
    }
}

// ts_sort_tiles_above in ONE launch (the companion of ts_raster_fwd_sort, which sorts the lists of up to kWaveSortMax
// entries itself): one workgroup per tile, which leaves at once unless its list is longer - then the register
// network with LDS stages (up to kSortCap keys) or the sample sort, on the same 48 KiB.  On frames that take this path
// (16x16 lists: fewer than ~1 000 pairs per tile on average) long lists are the exception, so the sample sort's LDS
// footprint costs nothing here, and the queue of oversized tiles with its second launch is gone.
__global__ __launch_bounds__(kThreads) void sort_tiles_above_kernel(
    const int* __restrict__ tile_bins, const float* __restrict__ depths,
    const int* __restrict__ bucket_ids, int* __restrict__ ids_sorted, const ListStats stats) {
    __shared__ unsigned long long lds_u64[kLargeLdsU64 > kSortCap / 2 ? kLargeLdsU64 : kSortCap / 2];
    if (stats.group_max && blockIdx.x == 0) store_longest(stats);
    const int2 range = reinterpret_cast<const int2*>(tile_bins)[blockIdx.x];
    const int n = range.y - range.x;
    if (n <= kWaveSortMax) return;
    if (n <= kSortCap) sort_bucket_block(bucket_ids + range.x, depths, ids_sorted + range.x, n, lds_u64);
    else sort_tile_sample(bucket_ids + range.x, depths, ids_sorted + range.x, n, lds_u64);
}

__global__ __launch_bounds__(kThreads) void pack_splats_kernel(int n, const ts::PackArgs a,
                                                              const float* __restrict__ colors) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (a.radii[i] <= 0) return;
    float c0, c1, c2, c3 = 0.0f;
    if (a.channels == 4 && a.depths == nullptr) {
        const float4 c = reinterpret_cast<const float4*>(colors)[i];
        c0 = c.x; c1 = c.y; c2 = c.z; c3 = c.w;
    } else {             // [n,3] colours; channel 3 of an RGB + depth frame = depths (rasterize.py:48-50)
        c0 = colors[3 * i]; c1 = colors[3 * i + 1]; c2 = colors[3 * i + 2];
        if (a.channels == 4) c3 = a.depths[i];
    }
    ts::pack_one(a, i, c0, c1, c2, c3);
}

// A launch with `lds` bytes of dynamic LDS: beyond 64 KiB the kernel has to be told so first (the emit launches and the
// one-walk fine hop are beyond it at the default kStageCap and kRunItems; the window launches on large frames)
template <typename... Params, typename... Args>
void launch_with_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

}  // namespace

extern "C" {

int32_t ts_num_tiles(const ts_camera* cam) {
    if (!cam) return 0;
    const int tbx = cam->wide_tiles ? (cam->tile_bounds_x + 1) / 2 : cam->tile_bounds_x;
    return cam->tile_rows * tbx;
}

int64_t ts_scan_ws_ints(int32_t n) {
    return n <= 0 ? 1 : (int64_t)((n + kScanBlock - 1) / kScanBlock);
}

int ts_scan_tiles(int32_t n, const int32_t* num_tiles_hit, int32_t* cum_tiles_hit,
                  int32_t* scan_ws, int32_t* total_out, void* stream) {
    if (n < 0) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!num_tiles_hit || !cum_tiles_hit || !scan_ws) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = (n + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(scan_local_kernel, dim3(nb), dim3(kThreads), 0, s, n, num_tiles_hit,
                       cum_tiles_hit, scan_ws, total_out);
    if (nb > 1)
        hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(kThreads), 0, s, n, cum_tiles_hit, scan_ws,
                           total_out);
    return launch_status();
}

int64_t ts_bin_ws_ints(int32_t n, int32_t num_tiles) { return bin_geometry(n, num_tiles).spare + 1; }

int ts_bin_count(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                 const ts_camera* cam, int32_t* bin_ws, void* stream) {
    if (n < 0 || !cam || !bin_ws) return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (nt <= 0) return 0;
    if (n > 0 && (!xys || !radii)) return TS_E_BADARG;
    const BinGeometry g = bin_geometry(n, nt);
    const int window = bin_window_tiles(n, nt);
    const int windows = (nt + window - 1) / window;
    launch_with_lds(bin_count_kernel, dim3(g.chunks, windows), dim3(kBinThreads), (size_t)window * sizeof(int),
                    (hipStream_t)stream, n, g.chunk, xys, radii, reinterpret_cast<const float4*>(splats), *cam, nt,
                    window, bin_ws);
    return launch_status();
}

int ts_tile_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                    const int32_t* cum_tiles_hit, int64_t capacity, void* stream) {
    return ts_tile_offsets_stats(n, num_tiles, bin_ws, tile_bins, cum_tiles_hit, capacity, nullptr, stream);
}

int ts_tile_offsets_stats(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                          const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream) {
    if (n < 0 || num_tiles < 0) return TS_E_BADARG;
    if (num_tiles == 0) return 0;
    if (!bin_ws || !tile_bins) return TS_E_BADARG;
    const BinGeometry g = bin_geometry(n, num_tiles);
    int* tile_total = bin_ws + g.tile_start;                    // [T + 1]: becomes tile_start, [T] = grand total
    const int per_group = (g.chunks + kScanGroups - 1) / kScanGroups;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(column_scan_kernel, dim3((num_tiles + kColTiles - 1) / kColTiles),
                       dim3(kColTiles * kScanGroups), 0, s, num_tiles, g.chunks, per_group, bin_ws, tile_total, true);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(kOffsetsThreads), 0, s, num_tiles, tile_total,
                       tile_bins, bin_ws + g.spare,
                       (cum_tiles_hit && n > 0) ? cum_tiles_hit + (n - 1) : nullptr, (long long)capacity, longest_list);
    return launch_status();
}

int32_t ts_bin_group_form(int32_t n) { return two_hop(n) ? 1 : 0; }

int ts_bin_count_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                        const ts_camera* cam, int32_t* bin_ws, void* stream) {
    if (!cam || !bin_ws || !xys || !radii || !two_hop(n)) return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (nt <= 0) return 0;
    const BinGeometry g = bin_geometry(n, nt);
    hipLaunchKernelGGL(group_bin_count_kernel, dim3(g.chunks), dim3(kBinThreads), (size_t)g.groups * sizeof(int),
                       (hipStream_t)stream, n, g.chunk, xys, radii, reinterpret_cast<const float4*>(splats), *cam,
                       g.groups, bin_ws);
    return launch_status();
}

}  // extern "C"

namespace {
// The offsets launch of the group form (BASES: the counts at the front of the workspace become bases) and of the
// one-walk form (its counts row stays as it is).  One workgroup scans the columns too while the B x G matrix is small
// (config 3: 245 x 255 ints = 250 KB); beyond kGoSingleMax ints (config 5: 512 x 507) the columns get
// column_scan_kernel's many workgroups first.  (One walk: the column totals of a frame that tripped the guard are sums
// of stale words, and the offsets launch never reads them; its groups fit the LDS by one_walk_form.)
template <bool BASES>
int group_offsets(const BinGeometry& g, int num_tiles, int* bin_ws, int* tile_bins, const int* total_ptr,
                  long long capacity, int* longest_list, hipStream_t s) {
    int* counts = bin_ws + (BASES ? 0 : g.counts);
    int* col_total = nullptr;
    if ((long long)g.chunks * g.groups > kGoSingleMax || g.groups > kGoLdsGroups) {
        col_total = bin_ws + (BASES ? g.group_totals : g.col_total);
        const int per_group = (g.chunks + kScanGroups - 1) / kScanGroups;
        hipLaunchKernelGGL(column_scan_kernel, dim3((g.groups + kColTiles - 1) / kColTiles),
                           dim3(kColTiles * kScanGroups), 0, s, g.groups, g.chunks, per_group, counts, col_total, BASES);
        counts = nullptr;
    }
    hipLaunchKernelGGL(group_tile_offsets_kernel<BASES>, dim3(1), dim3(kGoThreads), 0, s, num_tiles, g.groups, g.chunks,
                       counts, (const int*)col_total, bin_ws + g.tile_start, tile_bins, bin_ws + g.spare, total_ptr,
                       capacity, longest_list);
    return launch_status();
}
}  // namespace

extern "C" {

int ts_group_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                     const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream) {
    if (num_tiles < 0 || !two_hop(n)) return TS_E_BADARG;
    if (num_tiles == 0) return 0;
    if (!bin_ws || !tile_bins) return TS_E_BADARG;
    return group_offsets<true>(bin_geometry(n, num_tiles), num_tiles, bin_ws, tile_bins,
                               cum_tiles_hit ? cum_tiles_hit + (n - 1) : nullptr, (long long)capacity, longest_list,
                               (hipStream_t)stream);
}

int ts_bin_scatter_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                          const ts_camera* cam, int32_t* bin_ws, int32_t* tile_bins, int32_t* bucket_ids,
                          int32_t* scratch, void* stream) {
    if (!cam || !xys || !radii || !bin_ws || !tile_bins || !bucket_ids || !scratch || !two_hop(n))
        return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (nt <= 0) return 0;
    const BinGeometry g = bin_geometry(n, nt);
    int* tile_start = bin_ws + g.tile_start;
    hipStream_t s = (hipStream_t)stream;
    const auto coarse = (cam->hints & TS_HINT_BALANCED_WALK) ? bin_scatter_coarse_kernel<true, true>
                                                             : bin_scatter_coarse_kernel<false, true>;
    hipLaunchKernelGGL(coarse, dim3(g.chunks), dim3(kBinThreads), (size_t)g.groups * sizeof(int), s, n, g.chunk, xys,
                       radii, reinterpret_cast<const float4*>(splats), *cam, nt, (const int*)bin_ws,
                       (const int*)tile_start, scratch);
    hipLaunchKernelGGL(bin_scatter_fine_groups_kernel, dim3(g.groups), dim3(kFineThreads), 0, s, nt, tile_start,
                       tile_bins, bin_ws + g.group_max, (const int*)scratch, bucket_ids);
    return launch_status();
}

int32_t ts_bin_one_walk_form(int32_t n, int32_t num_tiles) { return one_walk_form(n, num_tiles) ? 1 : 0; }

int32_t ts_bin_stage_capacity(void) { return kStageCap; }

int ts_bin_emit_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                       const ts_camera* cam, const int32_t* cum_tiles_hit, int64_t capacity, int32_t* bin_ws,
                       int32_t* scratch, void* stream) {
    return ts_bin_emit_groups_spans(n, xys, radii, splats, nullptr, cam, cum_tiles_hit, capacity, bin_ws, scratch,
                                    stream);
}

int ts_bin_emit_groups_spans(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                             const int32_t* row_spans, const ts_camera* cam, const int32_t* cum_tiles_hit,
                             int64_t capacity, int32_t* bin_ws, int32_t* scratch, void* stream) {
    if (!cam || !xys || !radii || !cum_tiles_hit || !bin_ws || !scratch) return TS_E_BADARG;
    if (row_spans && ((uintptr_t)row_spans & 15)) return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (!one_walk_form(n, nt) || (cam->hints & TS_HINT_BALANCED_WALK)) return TS_E_BADARG;
    const BinGeometry g = bin_geometry(n, nt);
    // one launch, with or without records: the two kernels take the same arguments behind (kernel, records)
    auto emit = [&](auto kernel, auto... records) {
        launch_with_lds(kernel, dim3(g.chunks), dim3(kBinThreads), emit_lds_bytes(g.groups), (hipStream_t)stream, n,
                        g.chunk, xys, radii, reinterpret_cast<const float4*>(splats), records..., *cam, g.groups,
                        cum_tiles_hit, (long long)capacity, bin_ws + g.counts, bin_ws + g.starts, scratch);
    };
    if (row_spans) emit(bin_scatter_spans_kernel, reinterpret_cast<const int4*>(row_spans));
    else emit(bin_scatter_emit_kernel);
    return launch_status();
}

int ts_emit_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                    const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream) {
    if (!one_walk_form(n, num_tiles) || !bin_ws || !tile_bins || !cum_tiles_hit) return TS_E_BADARG;
    return group_offsets<false>(bin_geometry(n, num_tiles), num_tiles, bin_ws, tile_bins, cum_tiles_hit + (n - 1),
                                (long long)capacity, longest_list, (hipStream_t)stream);
}

int ts_bin_gather_groups(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins, int32_t* bucket_ids,
                         const int32_t* scratch, void* stream) {
    if (!one_walk_form(n, num_tiles) || !bin_ws || !tile_bins || !bucket_ids || !scratch) return TS_E_BADARG;
    const BinGeometry g = bin_geometry(n, num_tiles);
    launch_with_lds(bin_scatter_fine_runs_kernel, dim3(g.groups), dim3(kFineThreads), (size_t)kRunPass * sizeof(int),
                    (hipStream_t)stream, num_tiles, g.groups, g.chunks, (const int*)(bin_ws + g.counts),
                    (const int*)(bin_ws + g.starts), bin_ws + g.tile_start, tile_bins, bin_ws + g.group_max, scratch,
                    bucket_ids);
    return launch_status();
}

int ts_bin_scatter(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                   const ts_camera* cam, const int32_t* bin_ws, int32_t* bucket_ids, int32_t* scratch,
                   void* stream) {
    if (n < 0 || !cam) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!xys || !radii || !bin_ws || !bucket_ids) return TS_E_BADARG;
    const int nt = ts_num_tiles(cam);
    if (nt <= 0) return 0;
    const BinGeometry g = bin_geometry(n, nt);
    const int* tile_start = bin_ws + g.tile_start;
    hipStream_t s = (hipStream_t)stream;
    // two coalesced hops (see bin_scatter_coarse_kernel) where the write amplification of the direct scatter is what
    // binds; a small launch (a 100 k scene, the ~125 k records of one rank of a sharded frame) is latency-bound and
    // the second launch costs more than it saves (34 vs 12 us on a 1/8 stripe of config 3)
    if (scratch && two_hop(n)) {
        // load-balanced walk where the caller says a Gaussian covers many tiles (ts_camera.hints & TS_HINT_BALANCED_WALK):
        // config 5 (16 bounding-box tiles per Gaussian) coarse hop 369 -> 274 us; config 3 (6 tiles) 51 -> 56 us
        const auto coarse = (cam->hints & TS_HINT_BALANCED_WALK) ? bin_scatter_coarse_kernel<true, false>
                                                                 : bin_scatter_coarse_kernel<false, false>;
        hipLaunchKernelGGL(coarse, dim3(g.chunks), dim3(kBinThreads), (size_t)g.groups * sizeof(int), s, n, g.chunk, xys,
                           radii, reinterpret_cast<const float4*>(splats), *cam, nt, bin_ws, tile_start, scratch);
        hipLaunchKernelGGL(bin_scatter_fine_kernel, dim3(g.groups), dim3(kFineThreads), 0, s, nt, tile_start,
                           (const int*)scratch, bucket_ids);
        return launch_status();
    }
    const int window = bin_window_tiles(n, nt);
    const int windows = (nt + window - 1) / window;
    launch_with_lds(bin_scatter_kernel, dim3(g.chunks, windows), dim3(kBinThreads), (size_t)window * sizeof(int), s, n,
                    g.chunk, xys, radii, reinterpret_cast<const float4*>(splats), *cam, nt, window, bin_ws, tile_start,
                    bucket_ids);
    return launch_status();
}

}  // extern "C"

namespace {
// what the sort launch of a group-form or one-walk frame needs for the longest-list word (BinGeometry: group_max, guard)
inline bool list_stats(int n, int num_tiles, const int32_t* bin_ws, int32_t* longest_list, ListStats* st) {
    *st = ListStats{nullptr, nullptr, nullptr, 0};
    if (!longest_list) return true;
    if (!bin_ws || !two_hop(n) || num_tiles <= 0) return false;
    const BinGeometry g = bin_geometry(n, num_tiles);
    *st = ListStats{bin_ws + g.group_max, bin_ws + g.guard, longest_list, g.groups};
    return true;
}
}  // namespace

extern "C" {

int ts_sort_tiles(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                  const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                  int32_t* zeroed_counter, void* stream) {
    return ts_sort_tiles_stats(num_tiles, tile_bins, depths, bucket_ids, gaussian_ids_sorted, sort_ws, zeroed_counter,
                               0, nullptr, nullptr, stream);
}

int ts_sort_tiles_stats(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                        const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                        int32_t* zeroed_counter, int32_t n, const int32_t* bin_ws, int32_t* longest_list,
                        void* stream) {
    if (num_tiles < 0) return TS_E_BADARG;
    if (num_tiles == 0) return 0;
    if (!tile_bins || !depths || !bucket_ids || !gaussian_ids_sorted || !sort_ws) return TS_E_BADARG;
    ListStats stats;
    if (!list_stats(n, num_tiles, bin_ws, longest_list, &stats)) return TS_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    // counter + list of the tiles beyond the sorting network.  zeroed_counter: a word the caller knows to
    // be zero (ts_tile_offsets leaves the last word of its workspace so) - saves a 4-byte memset launch
    int32_t* counter = zeroed_counter ? zeroed_counter : sort_ws;
    int32_t* list = zeroed_counter ? sort_ws : sort_ws + 1;
    if (!zeroed_counter) {
        hipError_t e = hipMemsetAsync(sort_ws, 0, sizeof(int32_t), s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(sort_tiles_small_kernel, dim3((num_tiles + kThreads / 64 - 1) / (kThreads / 64)),
                       dim3(kThreads), 0, s, (int)num_tiles, tile_bins, depths, bucket_ids,
                       gaussian_ids_sorted, counter, list, stats);
    hipLaunchKernelGGL(sort_tiles_mid_kernel, dim3(num_tiles), dim3(kThreads), 0, s, tile_bins, depths,
                       bucket_ids, gaussian_ids_sorted, (int*)nullptr, (int*)nullptr);
    const int grid = num_tiles < 768 ? num_tiles : 768;
    hipLaunchKernelGGL(sort_tiles_large_kernel, dim3(grid), dim3(kThreads), 0, s, tile_bins, depths,
                       bucket_ids, gaussian_ids_sorted, counter, list);
    return launch_status();
}

int ts_sort_tiles_above(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                        const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                        int32_t* zeroed_counter, void* stream) {
    (void)sort_ws; (void)zeroed_counter;        // (no queue of oversized tiles any more: every tile has its workgroup)
    return ts_sort_tiles_above_stats(num_tiles, tile_bins, depths, bucket_ids, gaussian_ids_sorted, 0, nullptr, nullptr,
                                     stream);
}

int ts_sort_tiles_above_stats(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                              const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t n,
                              const int32_t* bin_ws, int32_t* longest_list, void* stream) {
    if (num_tiles < 0) return TS_E_BADARG;
    if (num_tiles == 0) return 0;
    if (!tile_bins || !depths || !bucket_ids || !gaussian_ids_sorted) return TS_E_BADARG;
    ListStats stats;
    if (!list_stats(n, num_tiles, bin_ws, longest_list, &stats)) return TS_E_BADARG;
    hipLaunchKernelGGL(sort_tiles_above_kernel, dim3(num_tiles), dim3(kThreads), 0, (hipStream_t)stream, tile_bins,
                       depths, bucket_ids, gaussian_ids_sorted, stats);
    return launch_status();
}

int ts_pack_splats(int32_t n, int32_t channels, int32_t flags, const float* xys, const int32_t* radii,
                   const float* conics, const float* colors, const float* opacity,
                   const int32_t* cum_tiles_hit, const ts_camera* cam, const float* depths, float* splats,
                   void* stream) {
    if (n < 0 || !cam || (channels != 3 && channels != 4)) return TS_E_BADARG;
    if (n == 0) return 0;
    if (!xys || !radii || !conics || !colors || !opacity || !cum_tiles_hit || !splats)
        return TS_E_BADARG;
    ts::PackArgs a;
    a.channels = channels; a.flags = (int)flags; a.xys = xys; a.radii = radii; a.conics = conics;
    a.opacity = opacity; a.cum_tiles_hit = cum_tiles_hit; a.depths = depths;
    a.splats = reinterpret_cast<float4*>(splats); a.cam = *cam;
    hipLaunchKernelGGL(pack_splats_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       (hipStream_t)stream, n, a, colors);
    return launch_status();
}

}  // extern "C"
