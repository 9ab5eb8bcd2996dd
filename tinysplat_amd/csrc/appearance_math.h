// appearance_math.h - the per-view colour model as the kernels of appearance.hip and a host build
// (tests/hostmath/appearance.cpp) share it: a bilateral grid of 3x4 affine colour matrices, sliced per pixel by position
// and luminance, its backward pass, the grid's total variation, and the 22 sums of a least-squares affine colour fit.
// This header is the only implementation of the definition in section 6s; both builds compile it with -ffp-contract=off,
// so every float32 product, sum and quotient below is rounded on its own in both.
//
//   grid      float32 [L, Gh, Gw, 12]; entry c = 4 r + k of a vertex is element (r, k) of a 3x4 matrix
//   axis      u = ((p + 0.5f) / P) * (G - 1); i0 = min((int)u, G - 2), i1 = i0 + 1, t = u - i0; G == 1: i0 = i1 = 0, t = 0
//   level     w = gray * (L - 1), gray = (0.299f r + 0.587f g) + 0.114f b; wc = w clamped to [0, L - 1] (not w > 0, NaN
//             included: 0); l0, l1, tz from wc as an axis takes them from u; inside = (w > 0 && w < L - 1)
//   slice     lerp(a, b, t) = a + t * (b - a), nested along x, then y, then z: a grid that is constant in space returns its
//             constant bit for bit (b - a == 0 exactly)
//   forward   out_r = ((A[4r] r + A[4r+1] g) + A[4r+2] b) + A[4r+3]
//   backward  vA[4r+k] = V_r * in_k, in = (r, g, b, 1);
//             v_in_k = ((A[k] V_0 + A[4+k] V_1) + A[8+k] V_2) + inside * ((L - 1) * lum_k) * sum_c vA[c] (A1_c - A0_c),
//             the sum taken in ascending c; v_G[vertex, c] = sum over pixels of vA[c] * fz * fy * fx, every factor t or
//             1 - t (float32), their product and the sum in double
#ifndef TINYSPLAT_APPEARANCE_MATH_H
#define TINYSPLAT_APPEARANCE_MATH_H

#include <math.h>
#include <stdint.h>

#ifndef TS_HD
#if defined(__HIPCC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif
#endif

#define TS_APP_ENTRIES 12                    // floats per vertex
#define TS_APP_TILE_W 64                     // the backward pass: pixels of a workgroup's tile, one wave per row segment
#define TS_APP_TILE_H 8
#define TS_APP_REDUCE_THREADS 1024           // threads of every one-workgroup sum (total variation, fit)
#define TS_APP_FIT_SUMS 22                   // 10 distinct sums of phi phi^T, 12 of phi t^T
#define TS_APP_FIT_LANE_PIXELS 32            // pixels per lane of a wave of the fit: a wave takes 2048 consecutive pixels

struct TsAppAxis { int i0, i1; float t; };
struct TsAppLevel { int l0, l1; float t; int inside; };

TS_HD float ts_app_lerp(float a, float b, float t) { return a + t * (b - a); }

// pixel p of P along an axis with G vertices
TS_HD TsAppAxis ts_app_axis(int p, int P, int G) {
    TsAppAxis a;
    a.i0 = 0; a.i1 = 0; a.t = 0.0f;
    if (G == 1) return a;
    const float u = (((float)p + 0.5f) / (float)P) * (float)(G - 1);
    int i0 = (int)u;
    if (i0 > G - 2) i0 = G - 2;
    a.i0 = i0; a.i1 = i0 + 1; a.t = u - (float)i0;
    return a;
}

TS_HD float ts_app_gray(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

TS_HD TsAppLevel ts_app_level(float gray, int L) {
    TsAppLevel z;
    const float top = (float)(L - 1);
    const float w = gray * top;
    float wc = w > 0.0f ? w : 0.0f;                      // NaN -> 0
    if (wc > top) wc = top;
    z.inside = (w > 0.0f && w < top) ? 1 : 0;
    z.l0 = 0; z.l1 = 0; z.t = 0.0f;
    if (L == 1) return z;
    int l0 = (int)wc;
    if (l0 > L - 2) l0 = L - 2;
    z.l0 = l0; z.l1 = l0 + 1; z.t = wc - (float)l0;
    return z;
}

// the 12 entries of one level at (x, y) from the level's four vertices: x, then y
TS_HD void ts_app_bilerp(const float* v00, const float* v01, const float* v10, const float* v11, float tx, float ty,
                         float* A) {
    for (int c = 0; c < TS_APP_ENTRIES; ++c) {
        const float top = ts_app_lerp(v00[c], v01[c], tx), bot = ts_app_lerp(v10[c], v11[c], tx);
        A[c] = ts_app_lerp(top, bot, ty);
    }
}

// vertex (l, j, i) of a grid -> its first float
TS_HD size_t ts_app_vertex(int Gh, int Gw, int l, int j, int i) {
    return (((size_t)l * Gh + j) * Gw + i) * TS_APP_ENTRIES;
}

TS_HD void ts_app_level_matrix(const float* G, int Gh, int Gw, int l, const TsAppAxis& ax, const TsAppAxis& ay, float* A) {
    ts_app_bilerp(G + ts_app_vertex(Gh, Gw, l, ay.i0, ax.i0), G + ts_app_vertex(Gh, Gw, l, ay.i0, ax.i1),
                  G + ts_app_vertex(Gh, Gw, l, ay.i1, ax.i0), G + ts_app_vertex(Gh, Gw, l, ay.i1, ax.i1), ax.t, ay.t, A);
}

TS_HD void ts_app_apply(const float* A, float r, float g, float b, float* out) {
    for (int q = 0; q < 3; ++q) out[q] = ((A[4 * q] * r + A[4 * q + 1] * g) + A[4 * q + 2] * b) + A[4 * q + 3];
}

// one pixel forward from the two level matrices
TS_HD void ts_app_pixel_fwd(const float* A0, const float* A1, float tz, float r, float g, float b, float* out) {
    float A[TS_APP_ENTRIES];
    for (int c = 0; c < TS_APP_ENTRIES; ++c) A[c] = ts_app_lerp(A0[c], A1[c], tz);
    ts_app_apply(A, r, g, b, out);
}

// one pixel backward: vA[12] and v_in[3] from the two level matrices, the pixel and V = d loss / d out
TS_HD void ts_app_pixel_bwd(const float* A0, const float* A1, const TsAppLevel& z, int L, float r, float g, float b,
                            const float* V, float* vA, float* v_in) {
    const float in[4] = {r, g, b, 1.0f};
    const float lum[3] = {0.299f, 0.587f, 0.114f};
    float A[TS_APP_ENTRIES];
    for (int c = 0; c < TS_APP_ENTRIES; ++c) A[c] = ts_app_lerp(A0[c], A1[c], z.t);
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 4; ++k) vA[4 * q + k] = V[q] * in[k];
    float s = vA[0] * (A1[0] - A0[0]);
    for (int c = 1; c < TS_APP_ENTRIES; ++c) s = s + vA[c] * (A1[c] - A0[c]);
    const float top = (float)(L - 1);
    for (int k = 0; k < 3; ++k) {
        const float direct = (A[k] * V[0] + A[4 + k] * V[1]) + A[8 + k] * V[2];
        v_in[k] = z.inside ? direct + (top * lum[k]) * s : direct;
    }
}

// the derivative of the nested lerp with respect to vertex index `v` of an axis: t or 1 - t, their sum where i0 == i1
TS_HD float ts_app_hat(int v, int i0, int i1, float t) {
    return (v == i0 ? 1.0f - t : 0.0f) + (v == i1 ? t : 0.0f);
}

// ---- the backward pass's tiles: the vertices along one axis that the pixels [tile * T, tile * T + T) can reach
TS_HD void ts_app_tile_reach(int tile, int T, int P, int G, int* lo, int* n) {
    const int p0 = tile * T, p1 = (p0 + T < P ? p0 + T : P) - 1;
    *lo = ts_app_axis(p0, P, G).i0;                     // (i0 does not decrease with p: every operation is monotone)
    *n = ts_app_axis(p1, P, G).i1 - *lo + 1;
}

TS_HD int ts_app_max_reach(int T, int P, int G) {
    int most = 1;
    for (int tile = 0; tile * T < P; ++tile) {
        int lo, n;
        ts_app_tile_reach(tile, T, P, G, &lo, &n);
        if (n > most) most = n;
    }
    return most;
}

// doubles of one workgroup's slab of partial v_G sums
TS_HD int64_t ts_app_slab_doubles(int H, int W, int L, int Gh, int Gw) {
    return (int64_t)ts_app_max_reach(TS_APP_TILE_H, H, Gh) * ts_app_max_reach(TS_APP_TILE_W, W, Gw) * L * TS_APP_ENTRIES;
}

TS_HD int64_t ts_app_tiles(int H, int W) {
    return (int64_t)((H + TS_APP_TILE_H - 1) / TS_APP_TILE_H) * ((W + TS_APP_TILE_W - 1) / TS_APP_TILE_W);
}

// ---- total variation: element e of the grid adds its squared differences to the next vertex along x, y, z to acc[0..2]
// and returns its gradient d tv / d G[e] (double); n[a] = 12 * (pairs along axis a), 0 for an axis of size 1
TS_HD void ts_app_tv_counts(int L, int Gh, int Gw, double* n) {
    n[0] = Gw > 1 ? (double)TS_APP_ENTRIES * L * Gh * (Gw - 1) : 0.0;
    n[1] = Gh > 1 ? (double)TS_APP_ENTRIES * L * (Gh - 1) * Gw : 0.0;
    n[2] = L > 1 ? (double)TS_APP_ENTRIES * (L - 1) * Gh * Gw : 0.0;
}

TS_HD double ts_app_tv_element(const float* G, int L, int Gh, int Gw, int e, const double* n, double* acc) {
    const unsigned v = (unsigned)e / TS_APP_ENTRIES;    // (the grid has fewer than 2^31 floats: 32-bit index arithmetic)
    const unsigned row = v / (unsigned)Gw;
    const int i = (int)(v - row * (unsigned)Gw), l = (int)(row / (unsigned)Gh), j = (int)(row - (unsigned)l * (unsigned)Gh);
    const int stride[3] = {TS_APP_ENTRIES, TS_APP_ENTRIES * Gw, TS_APP_ENTRIES * Gw * Gh};
    const int at[3] = {i, j, l}, size[3] = {Gw, Gh, L};
    const double here = (double)G[e];
    double grad = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (size[a] == 1) continue;
        double d = 0.0;                                  // (to the previous vertex) - (to the next vertex)
        if (at[a] > 0) d = here - (double)G[e - stride[a]];
        if (at[a] < size[a] - 1) {
            const double nx = (double)G[e + stride[a]] - here;
            acc[a] += nx * nx;
            d = d - nx;
        }
        grad = grad + (2.0 / n[a]) * d;
    }
    return grad;
}

TS_HD double ts_app_tv_value(const double* sums, const double* n) {
    double v = 0.0;
    for (int a = 0; a < 3; ++a)
        if (n[a] > 0.0) v = v + sums[a] / n[a];
    return v;
}

// ---- affine fit: the 22 products of one pixel, added to acc (phi = (r, g, b, 1), target t):
// acc[0..9] = rr rg rb r gg gb g bb b 1, acc[10 + 3 k + c] = phi_k t_c
TS_HD void ts_app_fit_pixel(float r, float g, float b, float t0, float t1, float t2, double* acc) {
    const double p[4] = {(double)r, (double)g, (double)b, 1.0}, t[3] = {(double)t0, (double)t1, (double)t2};
    int s = 0;
    for (int a = 0; a < 4; ++a)
        for (int q = a; q < 4; ++q) acc[s++] += p[a] * p[q];
    for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c) acc[s++] += p[k] * t[c];
}

TS_HD float ts_app_byte_to_float(uint8_t b) { return (float)b / 255.0f; }   // metrics_math.h's quotient

TS_HD int64_t ts_app_fit_waves(int64_t pixels) {
    const int64_t per_wave = 64 * (int64_t)TS_APP_FIT_LANE_PIXELS;
    return (pixels + per_wave - 1) / per_wave;
}

#endif  // TINYSPLAT_APPEARANCE_MATH_H
