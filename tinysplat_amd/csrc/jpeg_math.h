// jpeg_math.h - the arithmetic and the tables of the baseline JPEG encoder (jpeg.hip), for host and
// device: the colour transform, the 8-point DCT, the quantisation, the zigzag order, libjpeg's table scaling, the Annex K
// Huffman tables with their code lookup, the bits one coefficient contributes to the scan, and the header writer.
//
//   samples   uint8 as they are; float32 x -> rint(clamp(255 x, 0, 255)) (a NaN is 0)
//   colour    Y = ((0.299 R + 0.587 G) + 0.114 B) - 128, Cb = (-0.168735892 R - 0.331264108 G) + 0.5 B,
//             Cr = (0.5 R - 0.418687589 G) - 0.081312411 B; 4:2:0 chroma = ((c00 + c01) + (c10 + c11)) * 0.25
//   DCT       out[u] = sum over x, in index order, of C[u][x] s[x]; rows first, then columns
//   quantise  rint(c / q), q = clamp((base s + 50) / 100, 1, 255), s = 5000 / quality below 50, else 200 - 2 quality
//   scan      lane k of a block (zigzag index) contributes: k = 0 the DC difference's code and amplitude; a non-zero AC
//             coefficient one ZRL per 16 zeros since the previous non-zero one, the (run, size) code and the amplitude
//             (at most 3 * 11 + 16 + 10 = 59 bits); k = 63 holding zero the EOB; every other zero nothing
//
// Every float32 operation is rounded on its own (compiled with -ffp-contract=off): the kernel's coefficients are the
// host build's bit for bit.
#ifndef TINYSPLAT_JPEG_MATH_H
#define TINYSPLAT_JPEG_MATH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_JPEG_HD __host__ __device__ inline
#else
#define TS_JPEG_HD inline
#endif

#define TS_JPEG_444 0
#define TS_JPEG_420 1
#define TS_JPEG_U8 0
#define TS_JPEG_F32 1
#define TS_JPEG_HEADER_BYTES 629        // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
#define TS_JPEG_BLOCK_BITS 1660         // a block's longest bit string: 22 for the DC, 26 for each of 63 AC coefficients

namespace ts_jpeg {

// zigzag index k -> natural index v * 8 + u, and its inverse
static constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static constexpr uint8_t kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                          41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                          46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// ITU-T T.81 Annex K.1 and K.2, natural order
static constexpr uint8_t kQuant[2][64] = {
    {16, 11, 10, 16, 24, 40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51, 87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3 - K.6: the number of codes of each length 1..16, and the symbols in code order.  Tables 0 DC luma, 1 AC luma,
// 2 DC chroma, 3 AC chroma.
static constexpr uint8_t kBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// C[u][x] = a(u) cos((2 x + 1) u pi / 16), a(0) = sqrt(1/8), a(u > 0) = 1/2: the orthonormal DCT-II
#define TS_JPEG_C0 0.353553391f
#define TS_JPEG_C1 0.490392640f
#define TS_JPEG_C2 0.461939766f
#define TS_JPEG_C3 0.415734806f
#define TS_JPEG_C5 0.277785117f
#define TS_JPEG_C6 0.191341716f
#define TS_JPEG_C7 0.0975451610f

}  // namespace ts_jpeg

// ---------------------------------------------------------------------------------------------------------------- shape
struct ts_jpeg_shape {
    int mcu;            // the MCU's side in pixels: 16 (4:2:0) or 8 (4:4:4)
    int mcus_x, mcus_y;
    int per_mcu;        // blocks per MCU: 6 or 3
    int restart;        // MCUs per restart segment
    int64_t mcus, blocks, segments;
};

// restart_interval 0: one MCU row.  false: a size outside 1..65535, an unknown subsampling, an interval outside 0..65535,
// or more blocks than a 32-bit count of the scan's bits can hold
TS_JPEG_HD bool ts_jpeg_make_shape(int width, int height, int subsampling, int restart_interval, ts_jpeg_shape* s) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return false;
    if (subsampling != TS_JPEG_444 && subsampling != TS_JPEG_420) return false;
    if (restart_interval < 0 || restart_interval > 65535) return false;
    s->mcu = subsampling == TS_JPEG_420 ? 16 : 8;
    s->per_mcu = subsampling == TS_JPEG_420 ? 6 : 3;
    s->mcus_x = (width + s->mcu - 1) / s->mcu;
    s->mcus_y = (height + s->mcu - 1) / s->mcu;
    s->restart = restart_interval ? restart_interval : s->mcus_x;
    s->mcus = (int64_t)s->mcus_x * s->mcus_y;
    s->blocks = s->mcus * s->per_mcu;
    s->segments = (s->mcus + s->restart - 1) / s->restart;
    return s->blocks * (TS_JPEG_BLOCK_BITS + 4) + 64 * s->segments < ((int64_t)1 << 31);
}

// the file's largest size: every block at its longest, every byte stuffed, a padding byte (stuffed) and a marker per segment
TS_JPEG_HD int64_t ts_jpeg_worst_bytes(const ts_jpeg_shape& s) {
    return TS_JPEG_HEADER_BYTES + s.blocks * (2 * ((TS_JPEG_BLOCK_BITS + 7) / 8)) + 4 * s.segments;
}

// -------------------------------------------------------------------------------------------------------------- samples
TS_JPEG_HD float ts_jpeg_level(float x) {
    const float v = 255.0f * x;
    return rintf(fminf(fmaxf(v, 0.0f), 255.0f));
}
TS_JPEG_HD float ts_jpeg_y(float r, float g, float b) { return ((0.299f * r + 0.587f * g) + 0.114f * b) - 128.0f; }
TS_JPEG_HD float ts_jpeg_cb(float r, float g, float b) { return (-0.168735892f * r - 0.331264108f * g) + 0.5f * b; }
TS_JPEG_HD float ts_jpeg_cr(float r, float g, float b) { return (0.5f * r - 0.418687589f * g) - 0.081312411f * b; }
TS_JPEG_HD float ts_jpeg_component(int comp, float r, float g, float b) {
    return comp == 0 ? ts_jpeg_y(r, g, b) : comp == 1 ? ts_jpeg_cb(r, g, b) : ts_jpeg_cr(r, g, b);
}
TS_JPEG_HD float ts_jpeg_mean4(float c00, float c01, float c10, float c11) { return ((c00 + c01) + (c10 + c11)) * 0.25f; }

// pixel (x, y) of the image, coordinates clamped to the frame (the padding repeats the last column and row) -> levels 0..255
TS_JPEG_HD void ts_jpeg_fetch(const void* image, int dtype, int pixel_stride, int width, int height, int x, int y, float rgb[3]) {
    x = x < width ? x : width - 1;
    y = y < height ? y : height - 1;
    const int64_t at = ((int64_t)y * width + x) * pixel_stride;
    if (dtype == TS_JPEG_U8) {
        const uint8_t* p = (const uint8_t*)image + at;
        rgb[0] = (float)p[0]; rgb[1] = (float)p[1]; rgb[2] = (float)p[2];
    } else {
        const float* p = (const float*)image + at;
        rgb[0] = ts_jpeg_level(p[0]); rgb[1] = ts_jpeg_level(p[1]); rgb[2] = ts_jpeg_level(p[2]);
    }
}
// sample (row r, column c) of the block of component comp whose first sample is pixel (x0, y0); step 2: a 4:2:0 chroma block
TS_JPEG_HD float ts_jpeg_sample(const void* image, int dtype, int pixel_stride, int width, int height, int comp, int step,
                                int x0, int y0, int r, int c) {
    float p[3];
    if (step == 1) {
        ts_jpeg_fetch(image, dtype, pixel_stride, width, height, x0 + c, y0 + r, p);
        return ts_jpeg_component(comp, p[0], p[1], p[2]);
    }
    float v[4];
    for (int j = 0; j < 4; ++j) {
        ts_jpeg_fetch(image, dtype, pixel_stride, width, height, x0 + 2 * c + (j & 1), y0 + 2 * r + (j >> 1), p);
        v[j] = ts_jpeg_component(comp, p[0], p[1], p[2]);
    }
    return ts_jpeg_mean4(v[0], v[1], v[2], v[3]);
}

// one pass of the separable DCT over eight samples; the sums run in index order
TS_JPEG_HD void ts_jpeg_dct8(const float s[8], float o[8]) {
    using namespace ts_jpeg;
#define TS_JPEG_ROW(a0, a1, a2, a3, a4, a5, a6, a7) \
    (((((((a0 * s[0] + a1 * s[1]) + a2 * s[2]) + a3 * s[3]) + a4 * s[4]) + a5 * s[5]) + a6 * s[6]) + a7 * s[7])
    o[0] = TS_JPEG_ROW(TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0);
    o[1] = TS_JPEG_ROW(TS_JPEG_C1, TS_JPEG_C3, TS_JPEG_C5, TS_JPEG_C7, -TS_JPEG_C7, -TS_JPEG_C5, -TS_JPEG_C3, -TS_JPEG_C1);
    o[2] = TS_JPEG_ROW(TS_JPEG_C2, TS_JPEG_C6, -TS_JPEG_C6, -TS_JPEG_C2, -TS_JPEG_C2, -TS_JPEG_C6, TS_JPEG_C6, TS_JPEG_C2);
    o[3] = TS_JPEG_ROW(TS_JPEG_C3, -TS_JPEG_C7, -TS_JPEG_C1, -TS_JPEG_C5, TS_JPEG_C5, TS_JPEG_C1, TS_JPEG_C7, -TS_JPEG_C3);
    o[4] = TS_JPEG_ROW(TS_JPEG_C0, -TS_JPEG_C0, -TS_JPEG_C0, TS_JPEG_C0, TS_JPEG_C0, -TS_JPEG_C0, -TS_JPEG_C0, TS_JPEG_C0);
    o[5] = TS_JPEG_ROW(TS_JPEG_C5, -TS_JPEG_C1, TS_JPEG_C7, TS_JPEG_C3, -TS_JPEG_C3, -TS_JPEG_C7, TS_JPEG_C1, -TS_JPEG_C5);
    o[6] = TS_JPEG_ROW(TS_JPEG_C6, -TS_JPEG_C2, TS_JPEG_C2, -TS_JPEG_C6, -TS_JPEG_C6, TS_JPEG_C2, -TS_JPEG_C2, TS_JPEG_C6);
    o[7] = TS_JPEG_ROW(TS_JPEG_C7, -TS_JPEG_C5, TS_JPEG_C3, -TS_JPEG_C1, TS_JPEG_C1, -TS_JPEG_C3, TS_JPEG_C5, -TS_JPEG_C7);
#undef TS_JPEG_ROW
}

// entry `natural` (v * 8 + u) of table 0 (luma) or 1 (chroma) at a quality of 1..100
TS_JPEG_HD int ts_jpeg_quant(int table, int natural, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = ((int)ts_jpeg::kQuant[table][natural] * s + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}
TS_JPEG_HD int ts_jpeg_quantise(float c, float q) { return (int)rintf(c / q); }

// ---------------------------------------------------------------------------------------------------------------- codes
TS_JPEG_HD int ts_jpeg_table_size(int table) { return (table & 1) ? 162 : 12; }
TS_JPEG_HD int ts_jpeg_table_symbol(int table, int i) {
    return (table & 1) ? ts_jpeg::kAcVals[table >> 1][i] : ts_jpeg::kDcVals[i];
}
// the i-th symbol of a table in code order -> length << 16 | code (T.81 Annex C)
TS_JPEG_HD uint32_t ts_jpeg_table_code(int table, int i) {
    uint32_t code = 0;
    int before = 0;
    for (int length = 1; length <= 16; ++length) {
        const int count = ts_jpeg::kBits[table][length - 1];
        if (i < before + count) return ((uint32_t)length << 16) | (code + (uint32_t)(i - before));
        code = (code + (uint32_t)count) << 1;
        before += count;
    }
    return 0;
}
// lut[symbol] <- length << 16 | code for every symbol of the table (the other entries stay as they are)
TS_JPEG_HD void ts_jpeg_fill_codes(int table, uint32_t* lut) {
    for (int i = 0; i < ts_jpeg_table_size(table); ++i) lut[ts_jpeg_table_symbol(table, i)] = ts_jpeg_table_code(table, i);
}

struct ts_jpeg_piece {
    uint64_t bits;      // right-aligned
    int len;
};

TS_JPEG_HD int ts_jpeg_size_of(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// What zigzag position k of a block contributes to the scan.  value: the DC difference for k = 0, else the coefficient;
// nonzero: bit j set where AC coefficient j (1..63) is not zero; dc_lut / ac_lut: ts_jpeg_fill_codes of the component's
// tables.
TS_JPEG_HD ts_jpeg_piece ts_jpeg_piece_of(int k, int value, uint64_t nonzero, const uint32_t* dc_lut, const uint32_t* ac_lut) {
    ts_jpeg_piece p{0, 0};
    if (k != 0 && value == 0) {
        if (k == 63) {                                   // the block ends in zeros: EOB
            p.bits = ac_lut[0] & 0xffffu;
            p.len = (int)(ac_lut[0] >> 16);
        }
        return p;
    }
    const int size = ts_jpeg_size_of(value);
    const uint32_t amplitude = (uint32_t)(value < 0 ? value + (1 << size) - 1 : value);
    uint32_t code;
    if (k == 0) {
        code = dc_lut[size];
    } else {
        const uint64_t below = nonzero & (((uint64_t)1 << k) - 1) & ~(uint64_t)1;
        const int prev = below ? 63 - __builtin_clzll(below) : 0;      // the previous non-zero AC position, or the DC
        const int run = k - prev - 1;
        const uint32_t zrl = ac_lut[0xF0];
        for (int z = 0; z < (run >> 4); ++z) {
            p.bits = (p.bits << (zrl >> 16)) | (zrl & 0xffffu);
            p.len += (int)(zrl >> 16);
        }
        code = ac_lut[((run & 15) << 4) | size];
    }
    p.bits = (((p.bits << (code >> 16)) | (code & 0xffffu)) << size) | amplitude;
    p.len += (int)(code >> 16) + size;
    return p;
}

// --------------------------------------------------------------------------------------------------------------- header
// SOI, APP0 (JFIF 1.01), DQT 0 and 1, SOF0, the four DHT, DRI, SOS: TS_JPEG_HEADER_BYTES bytes
TS_JPEG_HD int ts_jpeg_write_header(uint8_t* out, int width, int height, int quality, int subsampling, int restart) {
    int n = 0;
#define TS_JPEG_PUT(b) out[n++] = (uint8_t)(b)
#define TS_JPEG_PUT16(v) do { TS_JPEG_PUT((v) >> 8); TS_JPEG_PUT((v) & 255); } while (0)
    TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xD8);
    TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xE0); TS_JPEG_PUT16(16);
    TS_JPEG_PUT('J'); TS_JPEG_PUT('F'); TS_JPEG_PUT('I'); TS_JPEG_PUT('F'); TS_JPEG_PUT(0);
    TS_JPEG_PUT(1); TS_JPEG_PUT(1); TS_JPEG_PUT(0); TS_JPEG_PUT16(1); TS_JPEG_PUT16(1); TS_JPEG_PUT(0); TS_JPEG_PUT(0);
    for (int t = 0; t < 2; ++t) {
        TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xDB); TS_JPEG_PUT16(67); TS_JPEG_PUT(t);
        for (int k = 0; k < 64; ++k) TS_JPEG_PUT(ts_jpeg_quant(t, ts_jpeg::kZigzag[k], quality));
    }
    TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xC0); TS_JPEG_PUT16(17); TS_JPEG_PUT(8); TS_JPEG_PUT16(height); TS_JPEG_PUT16(width);
    TS_JPEG_PUT(3);
    TS_JPEG_PUT(1); TS_JPEG_PUT(subsampling == TS_JPEG_420 ? 0x22 : 0x11); TS_JPEG_PUT(0);
    TS_JPEG_PUT(2); TS_JPEG_PUT(0x11); TS_JPEG_PUT(1);
    TS_JPEG_PUT(3); TS_JPEG_PUT(0x11); TS_JPEG_PUT(1);
    for (int t = 0; t < 4; ++t) {                        // DC luma 0x00, AC luma 0x10, DC chroma 0x01, AC chroma 0x11
        TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xC4); TS_JPEG_PUT16(19 + ts_jpeg_table_size(t));
        TS_JPEG_PUT(((t & 1) << 4) | (t >> 1));
        for (int l = 0; l < 16; ++l) TS_JPEG_PUT(ts_jpeg::kBits[t][l]);
        for (int i = 0; i < ts_jpeg_table_size(t); ++i) TS_JPEG_PUT(ts_jpeg_table_symbol(t, i));
    }
    TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xDD); TS_JPEG_PUT16(4); TS_JPEG_PUT16(restart);
    TS_JPEG_PUT(0xFF); TS_JPEG_PUT(0xDA); TS_JPEG_PUT16(12); TS_JPEG_PUT(3);
    TS_JPEG_PUT(1); TS_JPEG_PUT(0x00); TS_JPEG_PUT(2); TS_JPEG_PUT(0x11); TS_JPEG_PUT(3); TS_JPEG_PUT(0x11);
    TS_JPEG_PUT(0); TS_JPEG_PUT(63); TS_JPEG_PUT(0);
#undef TS_JPEG_PUT16
#undef TS_JPEG_PUT
    return n;
}

// ----------------------------------------------------------------------------------------------------------- scan order
// block b of the scan -> its component (0 Y, 1 Cb, 2 Cr), the pixel of its first sample and the block that holds the DC
// predictor (-1: the first of its component in the restart segment)
TS_JPEG_HD void ts_jpeg_block_place(const ts_jpeg_shape& s, int64_t b, int* comp, int* x0, int* y0) {
    const int64_t m = b / s.per_mcu;
    const int k = (int)(b - m * s.per_mcu);
    const int mx = (int)(m % s.mcus_x), my = (int)(m / s.mcus_x);
    if (s.per_mcu == 3) {
        *comp = k;
        *x0 = mx * 8;
        *y0 = my * 8;
    } else {
        *comp = k < 4 ? 0 : k - 3;
        *x0 = mx * 16 + (k < 4 ? (k & 1) * 8 : 0);
        *y0 = my * 16 + (k < 4 ? (k >> 1) * 8 : 0);
    }
}
TS_JPEG_HD int64_t ts_jpeg_dc_predecessor(const ts_jpeg_shape& s, int64_t b) {
    const int64_t m = b / s.per_mcu;
    const int k = (int)(b - m * s.per_mcu);
    if (s.per_mcu == 6 && k >= 1 && k < 4) return b - 1;                 // Y01 Y10 Y11 follow the Y before them
    if (m % s.restart == 0) return -1;
    return s.per_mcu == 3 ? b - 3 : k == 0 ? b - 3 : b - 6;              // Y00 follows the previous MCU's Y11
}

#endif  // TINYSPLAT_JPEG_MATH_H
