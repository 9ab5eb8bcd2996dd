// Host build of csrc/row_spans.h for tests/test_row_spans_cpu.py and tests/test_gpu_row_spans.py: the routine the colour
// stage fills a span record with, the two decoders the emit launch and the tests use, and - as the reference - the plain
// loops of walk_chunk (csrc/binning.hip) over ts::tile_bbox, ts::TightTest and row_range, behind a C interface.
// recs: [n, stride] floats whose first six are the packed record's x, y, opacity, conic.xx, conic.xy, conic.yy.
#include "../../tinysplat_amd/csrc/row_spans.h"

extern "C" {

int rs_rows(void) { return ts::kSpanRows; }
int rs_cols(void) { return ts::kSpanCols; }
int rs_fallback(void) { return ts::kSpanFallback; }

// spans: [n, 4] words
void rs_make(int n, const float* recs, int stride, const int32_t* radii, int tight, int tbx, int tby, int row0, int rows,
             uint32_t* spans) {
    for (int i = 0; i < n; ++i) {
        const float* q = recs + (size_t)i * stride;
        const ts::RowSpans s = ts::make_row_spans(tight != 0, q[0], q[1], q[2], q[3], q[4], q[5], radii[i], tbx, tby, row0,
                                                  rows);
        for (int k = 0; k < 4; ++k) spans[4 * (size_t)i + k] = s.w[k];
    }
}

// nrows[i]: -1 for a record that is not representable, else its NON-EMPTY rows, whose (ty, lo, hi) go to
// triples[i][0 .. nrows[i]) ([n, 6, 3]); ty is the absolute tile row.  pop != 0: with the consuming decoder.
// Returns the number of records whose two decoders disagree.
int rs_decode(int n, const uint32_t* spans, int row0, int pop, int32_t* nrows, int32_t* triples) {
    int disagree = 0;
    for (int i = 0; i < n; ++i) {
        ts::RowSpans s, c;
        for (int k = 0; k < 4; ++k) s.w[k] = c.w[k] = spans[4 * (size_t)i + k];
        const int rows = ts::spans_rows(s);
        if (rows == ts::kSpanFallback) { nrows[i] = -1; continue; }
        int m = 0;
        bool same = true;
        for (int k = 0; k < rows && k < ts::kSpanRows; ++k) {
            int lo, hi, lo2, hi2;
            ts::spans_row(s, k, lo, hi);
            ts::spans_pop_row(c, lo2, hi2);
            same = same && lo == lo2 && hi == hi2;
            if (pop) { lo = lo2; hi = hi2; }
            if (hi <= lo) continue;
            int32_t* t = triples + ((size_t)i * ts::kSpanRows + m) * 3;
            t[0] = row0 + ts::spans_first_row(s) + k; t[1] = lo; t[2] = hi;
            ++m;
        }
        nrows[i] = m;
        disagree += same ? 0 : 1;
    }
    return disagree;
}

// walk_chunk's loops.  nrows[i]: the non-empty rows, the first `cap` of which go to triples ([n, cap, 3]);
// box[i] = {tile rows of the box the walk loops over (0: the Gaussian is skipped), first row - row0, largest hi}
void rs_reference(int n, const float* recs, int stride, const int32_t* radii, int tight, int tbx, int tby, int row0,
                  int rows, int cap, int32_t* nrows, int32_t* triples, int32_t* box) {
    for (int i = 0; i < n; ++i) {
        const float* q = recs + (size_t)i * stride;
        nrows[i] = 0;
        box[3 * i] = box[3 * i + 1] = box[3 * i + 2] = 0;
        const int r = radii[i];
        if (r <= 0) continue;
        const ts::TileBox b = ts::tile_bbox(q[0], q[1], (float)r, tbx, tby, row0, rows);
        if (b.maxy <= b.miny || b.maxx <= b.minx) continue;
        const ts::TightTest t(tight != 0, q[0], q[1], q[2], q[3], q[4], q[5], (float)r);
        if (t.cull_all) continue;
        box[3 * i] = b.maxy - b.miny;
        box[3 * i + 1] = b.miny - row0;
        int m = 0;
        for (int ty = b.miny; ty < b.maxy; ++ty) {
            int lo, hi;
            t.row_range(ty, b.minx, b.maxx, lo, hi);
            if (hi <= lo) continue;
            if (hi > box[3 * i + 2]) box[3 * i + 2] = hi;
            if (m < cap) {
                int32_t* o = triples + ((size_t)i * cap + m) * 3;
                o[0] = ty; o[1] = lo; o[2] = hi;
            }
            ++m;
        }
        nrows[i] = m;
    }
}

}  // extern "C"
