// A program of its own around tests/hostmath/row_spans.cpp: random Gaussians (round ones, needles, huge radii, faint
// ones) on three cameras, every record decoded by both decoders and compared with the plain loops.  This is the form in
// which csrc/row_spans.h runs under -fsanitize=address,undefined (g++ ... row_spans.cpp row_spans_main.cpp); the test
// suite builds it plainly (tests/test_row_spans_cpu.py).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" {
int rs_rows(void);
int rs_cols(void);
void rs_make(int n, const float* recs, int stride, const int32_t* radii, int tight, int tbx, int tby, int row0, int rows,
             uint32_t* spans);
int rs_decode(int n, const uint32_t* spans, int row0, int pop, int32_t* nrows, int32_t* triples);
void rs_reference(int n, const float* recs, int stride, const int32_t* radii, int tight, int tbx, int tby, int row0,
                  int rows, int cap, int32_t* nrows, int32_t* triples, int32_t* box);
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static double uniform() {                       // xorshift64*
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (double)((state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

int main() {
    const int n = 4096, cap = 64;
    struct Camera { int w, h, row0, rows; };
    const Camera cams[3] = {{1920, 1080, 0, 68}, {1920, 1080, 20, 11}, {4112, 48, 0, 3}};
    long checked = 0, fallback = 0;
    for (const Camera& c : cams) {
        for (int tight = 0; tight < 2; ++tight) {
            std::vector<float> recs((size_t)n * 6);
            std::vector<int32_t> radii(n);
            for (int i = 0; i < n; ++i) {
                const double s2 = exp(uniform() * 3.0 - 1.0), ratio = exp(uniform() * (i % 4 == 0 ? 5.5 : 1.0));
                const double s1 = s2 * ratio, th = uniform() * 3.141592653589793;
                const double ct = cos(th), st = sin(th), i1 = 1.0 / (s1 * s1), i2 = 1.0 / (s2 * s2);
                float* q = &recs[(size_t)i * 6];
                q[0] = (float)(uniform() * (c.w + 40) - 20.0);
                q[1] = (float)(uniform() * (c.h + 40) - 20.0);
                q[2] = i % 13 == 0 ? 6.1e-6f : (float)(0.004 + 0.99 * uniform());
                q[3] = (float)(ct * ct * i1 + st * st * i2);
                q[4] = (float)(ct * st * (i1 - i2));
                q[5] = (float)(st * st * i1 + ct * ct * i2);
                radii[i] = i % 17 == 0 ? 0 : (i % 19 == 0 ? 20000 : (int)ceil(3.0 * s1));
            }
            const int tbx = (c.w + 15) / 16, tby = (c.h + 15) / 16;
            std::vector<uint32_t> spans((size_t)n * 4);
            rs_make(n, recs.data(), 6, radii.data(), tight, tbx, tby, c.row0, c.rows, spans.data());
            std::vector<int32_t> want_n(n), want((size_t)n * cap * 3), box((size_t)n * 3);
            rs_reference(n, recs.data(), 6, radii.data(), tight, tbx, tby, c.row0, c.rows, cap, want_n.data(), want.data(),
                         box.data());
            for (int pop = 0; pop < 2; ++pop) {
                std::vector<int32_t> got_n(n), got((size_t)n * rs_rows() * 3);
                if (rs_decode(n, spans.data(), c.row0, pop, got_n.data(), got.data()) != 0) {
                    printf("the two decoders disagree\n");
                    return 1;
                }
                for (int i = 0; i < n; ++i) {
                    const bool fits = box[3 * i] <= rs_rows() && box[3 * i + 2] <= rs_cols() && box[3 * i + 1] <= 0xffff;
                    if ((got_n[i] < 0) != !fits) {
                        printf("Gaussian %d: fallback flag %d, representable %d\n", i, got_n[i] < 0, fits);
                        return 1;
                    }
                    if (!fits) { ++fallback; continue; }
                    bool same = got_n[i] == want_n[i];
                    for (int k = 0; same && k < 3 * want_n[i]; ++k)
                        same = got[(size_t)i * rs_rows() * 3 + k] == want[(size_t)i * cap * 3 + k];
                    if (!same) {
                        printf("Gaussian %d of camera %dx%d (tight %d): rows differ\n", i, c.w, c.h, tight);
                        return 1;
                    }
                    ++checked;
                }
            }
        }
    }
    printf("row spans ok: %ld records decoded, %ld fallbacks\n", checked, fallback);
    return 0;
}
