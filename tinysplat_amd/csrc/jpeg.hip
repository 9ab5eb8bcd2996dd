// jpeg.hip - baseline JPEG of a frame where the compositing kernel left it (the arithmetic, the tables
// and the per-coefficient rule: jpeg_math.h).  Only the compressed bytes leave the device.
//
//   transform   8 threads per 8x8 block, 32 blocks per workgroup: a thread transforms one row, the rows meet in LDS, the same
//               thread transforms one column, quantises it and drops it at its zigzag place; the workgroup's 4 KiB of int16
//               leave as 16-byte words.  Blocks lie in scan order, 128 bytes each.
//   bits        one wave per block, lane = zigzag index: a ballot of the non-zero AC lanes gives each lane its run (the
//               distance to the next lower set bit), so a lane knows its ZRLs, symbol and amplitude bits (<= 59) without a
//               loop over the block; lane 0 codes the DC difference.  The first launch stores the block's bit length; an
//               extra workgroup writes the header meanwhile.
//   scan        ts_scan_tiles over the bit lengths: a block's place in its restart segment is a difference of two sums.
//   place       the bits kernel again: the wave's prefix sum places the lanes' pieces in LDS (ds_or on zeroed words), the
//               wave stores whole words to the segment's stream and ORs the first and last, which it shares with its
//               neighbours, into zeroed memory.  Segment s starts at word (bits before it) / 32 + s, so segments never share
//               a word; the last block pads its segment's last byte with ones.
//   stuff       one wave per segment, twice: count the 0xFF bytes, then (after ts_scan_tiles over the segment sizes) write
//               bytes, stuffed zeros and the RSTm / EOI marker behind the header; the last segment stores the file's size.
//
// Integer OR is the only atomic: the result does not depend on order, so the file is the same on every run, and no stage's
// result depends on the launch shape.
#include <hip/hip_runtime.h>

#include "../../include/tinysplat_hip.h"
#include "host_util.h"
#include "jpeg_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 32;          // blocks per workgroup of the transform
constexpr int kWaveWords = 64;      // a block's bit string: <= 31 + TS_JPEG_BLOCK_BITS + 7 bits = 54 words

struct Image {
    const void* data;
    int dtype, pixel_stride, width, height, quality, subsampling;
};

__device__ __forceinline__ int wave_inclusive(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void jpeg_transform_kernel(const ts_jpeg_shape s, const Image im,
                                                                  int16_t* __restrict__ coef) {
    __shared__ float quant[2][64];
    __shared__ float rows[kGroup][8][9];
    __shared__ __align__(16) int16_t zig[kGroup][64];
    const int tid = threadIdx.x, g = tid >> 3, r = tid & 7;
    if (tid < 128) quant[tid >> 6][tid & 63] = (float)ts_jpeg_quant(tid >> 6, tid & 63, im.quality);
    const int64_t b = (int64_t)blockIdx.x * kGroup + g;
    const bool live = b < s.blocks;
    int comp = 0, x0 = 0, y0 = 0;
    if (live) {
        ts_jpeg_block_place(s, b, &comp, &x0, &y0);
        const int step = (s.per_mcu == 6 && comp != 0) ? 2 : 1;
        float smp[8], o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            smp[c] = ts_jpeg_sample(im.data, im.dtype, im.pixel_stride, im.width, im.height, comp, step, x0, y0, r, c);
        ts_jpeg_dct8(smp, o);
#pragma unroll
        for (int u = 0; u < 8; ++u) rows[g][r][u] = o[u];
    }
    __syncthreads();
    if (live) {
        float col[8], res[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) col[y] = rows[g][y][r];
        ts_jpeg_dct8(col, res);
#pragma unroll
        for (int v = 0; v < 8; ++v)
            zig[g][ts_jpeg::kZigzagOf[v * 8 + r]] = (int16_t)ts_jpeg_quantise(res[v], quant[comp != 0][v * 8 + r]);
    }
    __syncthreads();
    const int64_t word = (int64_t)blockIdx.x * kThreads + tid;          // 16 bytes: 8 coefficients
    if (word < s.blocks * 8) reinterpret_cast<uint4*>(coef)[word] = reinterpret_cast<const uint4*>(&zig[0][0])[tid];
}

struct HeaderArgs {
    uint8_t* out;
    int width, height, quality, subsampling;
};

// PLACE = false: bits[b] <- the block's bit length (and the last workgroup writes the header).  PLACE = true: the block's
// bit string goes to its place in the segment's stream; incl: the inclusive sums of bits.
template <bool PLACE>
__global__ __launch_bounds__(kThreads) void jpeg_bits_kernel(const ts_jpeg_shape s, const int16_t* __restrict__ coef,
                                                             int32_t* __restrict__ bits, const int32_t* __restrict__ incl,
                                                             uint32_t* __restrict__ stream, int64_t stream_words,
                                                             const HeaderArgs h) {
    __shared__ uint32_t dc[2][16], ac[2][256];
    __shared__ uint32_t words[kThreads / 64][kWaveWords];
    __shared__ uint8_t header[TS_JPEG_HEADER_BYTES + 3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (!PLACE && blockIdx.x == gridDim.x - 1) {
        if (tid == 0) ts_jpeg_write_header(header, h.width, h.height, h.quality, h.subsampling, s.restart);
        __syncthreads();
        for (int i = tid; i < TS_JPEG_HEADER_BYTES; i += kThreads) h.out[i] = header[i];
        return;
    }
    ac[0][tid] = 0;
    ac[1][tid] = 0;
    if (tid < 32) dc[tid >> 4][tid & 15] = 0;
    words[wave][lane] = 0;
    __syncthreads();
    for (int t = 0; t < 2; ++t) {
        if (tid < 12) dc[t][ts_jpeg_table_symbol(2 * t, tid)] = ts_jpeg_table_code(2 * t, tid);
        if (tid < 162) ac[t][ts_jpeg_table_symbol(2 * t + 1, tid)] = ts_jpeg_table_code(2 * t + 1, tid);
    }
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * (kThreads / 64) + wave;
    const bool live = b < s.blocks;                        // the same for every lane of a wave
    ts_jpeg_piece piece{0, 0};
    if (live) {
        const int c = coef[b * 64 + lane];
        const uint64_t nonzero = __ballot(lane >= 1 && c != 0);
        int value = c;
        if (lane == 0) {
            const int64_t pred = ts_jpeg_dc_predecessor(s, b);
            if (pred >= 0) value -= coef[pred * 64];
        }
        int comp, x0, y0;
        ts_jpeg_block_place(s, b, &comp, &x0, &y0);
        piece = ts_jpeg_piece_of(lane, value, nonzero, dc[comp != 0], ac[comp != 0]);
    }
    const int inc = wave_inclusive(piece.len);
    const int total = __shfl(inc, 63, 64);
    if (!PLACE) {
        if (live && lane == 0) bits[b] = total;
        return;
    }
    int64_t base = 0;
    int offset = 0, pad = 0;
    if (live) {
        const int64_t seg = (b / s.per_mcu) / s.restart;
        const int64_t first = seg * s.restart * s.per_mcu;
        int64_t last = first + (int64_t)s.restart * s.per_mcu;
        if (last > s.blocks) last = s.blocks;
        const int seg_start = first ? incl[first - 1] : 0;
        const int rel = (b ? incl[b - 1] : 0) - seg_start;
        base = (int64_t)(seg_start >> 5) + seg + (rel >> 5);
        offset = rel & 31;
        if (piece.len) {
            const int p = offset + inc - piece.len;
            const uint64_t v = piece.bits << (64 - piece.len);
            const int sh = p & 31, w0 = p >> 5;
            const uint32_t a = (uint32_t)(v >> (32 + sh)), m = (uint32_t)(v >> sh);
            const uint32_t z = sh ? (uint32_t)(v << (32 - sh)) : 0u;
            if (a && w0 < kWaveWords) atomicOr(&words[wave][w0], a);
            if (m && w0 + 1 < kWaveWords) atomicOr(&words[wave][w0 + 1], m);
            if (z && w0 + 2 < kWaveWords) atomicOr(&words[wave][w0 + 2], z);
        }
        if (b == last - 1) pad = (8 - ((rel + total) & 7)) & 7;          // the segment's last byte is filled with ones
        const int end = offset + total;
        if (lane == 0 && pad && (end >> 5) < kWaveWords) {
            atomicOr(&words[wave][end >> 5], ((1u << pad) - 1u) << (32 - (end & 31) - pad));
        }
    }
    __syncthreads();
    if (live) {
        const int nwords = (offset + total + pad + 31) >> 5;
        if (lane < nwords && base + lane < stream_words) {       // (a block's words never pass either bound)
            const uint32_t v = words[wave][lane];
            if (lane == 0 || lane == nwords - 1) {
                if (v) atomicOr(&stream[base + lane], v);
            } else {
                stream[base + lane] = v;
            }
        }
    }
}

// the words the place stage ORs into: everything up to the last segment's end
__global__ __launch_bounds__(kThreads) void jpeg_zero_kernel(const ts_jpeg_shape s, const int32_t* __restrict__ incl,
                                                             uint32_t* __restrict__ stream, int64_t capacity_words) {
    int64_t n = (int64_t)(incl[s.blocks - 1] >> 5) + s.segments + 2;
    if (n > capacity_words) n = capacity_words;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) stream[i] = 0u;
}

// WRITE = false: seg_size[seg] <- the segment's bytes, stuffed, with its marker.  WRITE = true: the bytes themselves;
// seg_end: the inclusive sums of seg_size.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void jpeg_stuff_kernel(const ts_jpeg_shape s, const int32_t* __restrict__ incl,
                                                              const uint32_t* __restrict__ stream, int64_t stream_words,
                                                              int32_t* __restrict__ seg_size, const int32_t* __restrict__ seg_end,
                                                              uint8_t* __restrict__ out, int32_t* __restrict__ size_word) {
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (seg >= s.segments) return;
    const int64_t first = seg * s.restart * s.per_mcu;
    int64_t last = first + (int64_t)s.restart * s.per_mcu;
    if (last > s.blocks) last = s.blocks;
    const int start = first ? incl[first - 1] : 0;
    const int nbytes = (incl[last - 1] - start + 7) >> 3;
    const int64_t base = (int64_t)(start >> 5) + seg;
    const int nwords = (nbytes + 3) >> 2;
    int pos = WRITE ? TS_JPEG_HEADER_BYTES + seg_end[seg] - seg_size[seg] : 0;
    for (int i0 = 0; i0 < nwords; i0 += 64) {
        const int i = i0 + lane;
        int nb = nbytes - 4 * i;
        nb = nb < 0 ? 0 : nb > 4 ? 4 : nb;
        const uint32_t w = nb && base + i < stream_words ? stream[base + i] : 0u;
        int count = 0;
        for (int j = 0; j < nb; ++j) count += 1 + (((w >> (24 - 8 * j)) & 255u) == 255u);
        const int inc = wave_inclusive(count);
        if (WRITE) {
            int o = pos + inc - count;
            for (int j = 0; j < nb; ++j) {
                const uint32_t byte = (w >> (24 - 8 * j)) & 255u;
                out[o++] = (uint8_t)byte;
                if (byte == 255u) out[o++] = 0;
            }
        }
        pos += __shfl(inc, 63, 64);
    }
    if (lane != 0) return;
    if (!WRITE) {
        seg_size[seg] = pos + 2;
        return;
    }
    out[pos] = 0xFF;
    out[pos + 1] = seg + 1 < s.segments ? (uint8_t)(0xD0 + (seg & 7)) : (uint8_t)0xD9;
    if (seg + 1 == s.segments) *size_word = pos + 2;
}

struct Workspace {
    int64_t coef, bits, incl, seg_size, seg_end, scan, stream, stream_words, total;
};

Workspace carve(const ts_jpeg_shape& s) {
    Workspace w;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        const int64_t here = at;
        at += align256(bytes);
        return here;
    };
    w.coef = take(s.blocks * 128);
    w.bits = take(s.blocks * 4);
    w.incl = take(s.blocks * 4);
    w.seg_size = take(s.segments * 4);
    w.seg_end = take(s.segments * 4);
    w.scan = take(ts_scan_ws_ints((int32_t)(s.blocks > s.segments ? s.blocks : s.segments)) * 4);
    w.stream_words = s.blocks * ((TS_JPEG_BLOCK_BITS + 31) / 32) + s.segments + 8;
    w.stream = take(w.stream_words * 4);
    w.total = at;
    return w;
}

}  // namespace

extern "C" {

int64_t ts_jpeg_ws_bytes(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return TS_E_BADARG;
    return carve(s).total;
}

int64_t ts_jpeg_max_bytes(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return TS_E_BADARG;
    return ts_jpeg_worst_bytes(s);
}

int64_t ts_jpeg_header(int32_t width, int32_t height, int32_t quality, int32_t subsampling, int32_t restart_interval,
                       uint8_t* out, int64_t out_capacity) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return TS_E_BADARG;
    if (quality < 1 || quality > 100 || !out || out_capacity < TS_JPEG_HEADER_BYTES) return TS_E_BADARG;
    return ts_jpeg_write_header(out, width, height, quality, subsampling, s.restart);
}

int ts_jpeg_encode(const void* image, int32_t dtype, int32_t pixel_stride, int32_t width, int32_t height, int32_t quality,
                   int32_t subsampling, int32_t restart_interval, void* workspace, uint8_t* out, int64_t out_capacity,
                   int32_t* size_word, int16_t* coefficients, void* stream) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return TS_E_BADARG;
    if (quality < 1 || quality > 100) return TS_E_BADARG;
    if (!(dtype == TS_JPEG_U8 && pixel_stride == 3) && !(dtype == TS_JPEG_F32 && (pixel_stride == 3 || pixel_stride == 4)))
        return TS_E_BADARG;
    if (!image || !workspace || !out || !size_word || ((uintptr_t)workspace & 255u)) return TS_E_BADARG;
    if (out_capacity < ts_jpeg_worst_bytes(s)) return TS_E_BADARG;          // the kernels do not check: refuse here
    const Workspace w = carve(s);
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)(ws + w.coef);
    int32_t* bits = (int32_t*)(ws + w.bits);
    int32_t* incl = (int32_t*)(ws + w.incl);
    int32_t* seg_size = (int32_t*)(ws + w.seg_size);
    int32_t* seg_end = (int32_t*)(ws + w.seg_end);
    int32_t* scan = (int32_t*)(ws + w.scan);
    uint32_t* words = (uint32_t*)(ws + w.stream);
    hipStream_t st = (hipStream_t)stream;
    const Image im{image, dtype, pixel_stride, width, height, quality, subsampling};
    const HeaderArgs h{out, width, height, quality, subsampling};
    const unsigned waves = (unsigned)nblocks(s.blocks, kThreads / 64);
    const unsigned seg_groups = (unsigned)nblocks(s.segments, kThreads / 64);

    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)nblocks(s.blocks, kGroup)), dim3(kThreads), 0, st, s, im, coef);
    if (coefficients) {
        const hipError_t e = hipMemcpyAsync(coefficients, coef, (size_t)s.blocks * 128, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(jpeg_bits_kernel<false>, dim3(waves + 1), dim3(kThreads), 0, st, s, coef, bits, incl, words,
                       w.stream_words, h);
    int rc = ts_scan_tiles((int32_t)s.blocks, bits, incl, scan, nullptr, stream);
    if (rc) return rc;
    const int64_t zero_groups = nblocks(w.stream_words, kThreads * 4);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3((unsigned)(zero_groups > 1024 ? 1024 : zero_groups)), dim3(kThreads), 0, st, s,
                       incl, words, w.stream_words);
    hipLaunchKernelGGL(jpeg_bits_kernel<true>, dim3(waves), dim3(kThreads), 0, st, s, coef, bits, incl, words,
                       w.stream_words, h);
    hipLaunchKernelGGL(jpeg_stuff_kernel<false>, dim3(seg_groups), dim3(kThreads), 0, st, s, incl, words, w.stream_words, seg_size,
                       seg_end,
                       out, size_word);
    rc = ts_scan_tiles((int32_t)s.segments, seg_size, seg_end, scan, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_stuff_kernel<true>, dim3(seg_groups), dim3(kThreads), 0, st, s, incl, words, w.stream_words, seg_size,
                       seg_end,
                       out, size_word);
    return launch_status();
}

}  // extern "C"
