// Host build of csrc/jpeg_math.h for tests/test_jpeg_cpu.py: the functions the kernels of csrc/jpeg.hip call, behind a C
// interface (compiled with -ffp-contract=off, as the kernels are), around a plain sequential bit writer.
#include "../../tinysplat_amd/csrc/jpeg_math.h"

#include <vector>

extern "C" {

int64_t jh_blocks(int width, int height, int subsampling) {
    ts_jpeg_shape s;
    return ts_jpeg_make_shape(width, height, subsampling, 0, &s) ? s.blocks : -1;
}

int jh_header(int width, int height, int quality, int subsampling, int restart_interval, uint8_t* out) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return -1;
    return ts_jpeg_write_header(out, width, height, quality, subsampling, s.restart);
}

// image -> int16 [blocks, 64]: the quantised coefficients, zigzag order, blocks in scan order
int jh_coefficients(const void* image, int dtype, int pixel_stride, int width, int height, int quality, int subsampling,
                    int16_t* out) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, 0, &s)) return -1;
    for (int64_t b = 0; b < s.blocks; ++b) {
        int comp, x0, y0;
        ts_jpeg_block_place(s, b, &comp, &x0, &y0);
        const int step = (s.per_mcu == 6 && comp != 0) ? 2 : 1;
        float rows[8][8], cols[8], res[8];
        for (int r = 0; r < 8; ++r) {
            float smp[8];
            for (int c = 0; c < 8; ++c)
                smp[c] = ts_jpeg_sample(image, dtype, pixel_stride, width, height, comp, step, x0, y0, r, c);
            ts_jpeg_dct8(smp, rows[r]);
        }
        for (int u = 0; u < 8; ++u) {
            for (int y = 0; y < 8; ++y) cols[y] = rows[y][u];
            ts_jpeg_dct8(cols, res);
            for (int v = 0; v < 8; ++v) {
                const float q = (float)ts_jpeg_quant(comp != 0, v * 8 + u, quality);
                out[64 * b + ts_jpeg::kZigzagOf[v * 8 + u]] = (int16_t)ts_jpeg_quantise(res[v], q);
            }
        }
    }
    return 0;
}

// coefficients as jh_coefficients wrote them -> the file; returns its size, or -1 where `capacity` is too small
int64_t jh_encode(const int16_t* coef, int width, int height, int quality, int subsampling, int restart_interval,
                  uint8_t* out, int64_t capacity) {
    ts_jpeg_shape s;
    if (!ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s)) return -1;
    std::vector<uint32_t> dc[2] = {std::vector<uint32_t>(16, 0), std::vector<uint32_t>(16, 0)};
    std::vector<uint32_t> ac[2] = {std::vector<uint32_t>(256, 0), std::vector<uint32_t>(256, 0)};
    for (int t = 0; t < 2; ++t) {
        ts_jpeg_fill_codes(2 * t, dc[t].data());
        ts_jpeg_fill_codes(2 * t + 1, ac[t].data());
    }
    std::vector<uint8_t> file(TS_JPEG_HEADER_BYTES);
    ts_jpeg_write_header(file.data(), width, height, quality, subsampling, s.restart);
    for (int64_t seg = 0; seg < s.segments; ++seg) {
        uint64_t acc = 0;
        int held = 0;
        auto put = [&](uint64_t bits, int len) {
            for (int i = len - 1; i >= 0; --i) {
                acc = (acc << 1) | ((bits >> i) & 1);
                if (++held == 8) {
                    file.push_back((uint8_t)acc);
                    if (acc == 0xFF) file.push_back(0);
                    acc = 0;
                    held = 0;
                }
            }
        };
        const int64_t first = seg * s.restart * s.per_mcu;
        int64_t last = (seg + 1) * s.restart * s.per_mcu;
        if (last > s.blocks) last = s.blocks;
        for (int64_t b = first; b < last; ++b) {
            int comp, x0, y0;
            ts_jpeg_block_place(s, b, &comp, &x0, &y0);
            const int16_t* z = coef + 64 * b;
            uint64_t nonzero = 0;
            for (int k = 1; k < 64; ++k)
                if (z[k]) nonzero |= (uint64_t)1 << k;
            const int64_t pred = ts_jpeg_dc_predecessor(s, b);
            for (int k = 0; k < 64; ++k) {
                const int value = k == 0 ? z[0] - (pred < 0 ? 0 : coef[64 * pred]) : z[k];
                const ts_jpeg_piece p = ts_jpeg_piece_of(k, value, nonzero, dc[comp != 0].data(), ac[comp != 0].data());
                put(p.bits, p.len);
            }
        }
        if (held) put((1u << (8 - held)) - 1, 8 - held);
        file.push_back(0xFF);
        file.push_back(seg + 1 < s.segments ? (uint8_t)(0xD0 + (seg & 7)) : (uint8_t)0xD9);
    }
    if ((int64_t)file.size() > capacity) return -1;
    for (size_t i = 0; i < file.size(); ++i) out[i] = file[i];
    return (int64_t)file.size();
}

int64_t jh_worst_bytes(int width, int height, int subsampling, int restart_interval) {
    ts_jpeg_shape s;
    return ts_jpeg_make_shape(width, height, subsampling, restart_interval, &s) ? ts_jpeg_worst_bytes(s) : -1;
}

}  // extern "C"
