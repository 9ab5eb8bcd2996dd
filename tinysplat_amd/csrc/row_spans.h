// row_spans.h - the 16-byte SPAN RECORD of one Gaussian: the tile columns the one-walk list build (binning.hip:
// bin_scatter_spans_kernel) enters it in, row by row.  Written by the colour stage (project.hip), which has the operands
// of the tight test in registers and its vector pipe idle behind the coefficient stream; read by the emit launch with
// one 16-byte load instead of the centre, the radius and two record words, and instead of the arithmetic on them.
//
// Nothing is derived here: make_row_spans runs ts::tile_bbox, ts::TightTest and TightTest::row_range exactly as
// walk_chunk does, on the values exactly as they are packed, and stores what they return.  Both translation units
// build with -ffp-contract=off, so a record holds bit for bit what the walk would compute.  Compiles for the host too
// (tests/hostmath/row_spans.cpp).
//
//   w[0]      first tile row inside the launch's stripe (bits 0..15) | R << 16
//             R = 0         nothing listed: culled, outside the stripe, or TightTest::cull_all
//             R = 1..6      tile rows of the box
//             R = 0xff      NOT REPRESENTABLE (more than 6 rows, a column index >= 256, a first row >= 65536): the walk
//                           computes this Gaussian itself, as before
//   w[1..3]   six 16-bit rows, row k in bits 16 (k & 1) .. of w[1 + k / 2]: lo | (hi - 1) << 8 for the half-open range
//             [lo, hi) of 16x16 tile columns; an EMPTY row (row_range left nothing) is lo = 1, hi - 1 = 0
#pragma once

#include "splat_math.h"

namespace ts {

constexpr int kSpanRows = 6;                 // rows a record holds
constexpr int kSpanCols = 256;               // column indices a record holds: 0 .. 255
constexpr int kSpanFallback = 0xff;          // R of a record that is not representable
constexpr unsigned int kSpanEmptyRow = 1u;   // lo = 1 > hi - 1 = 0

struct RowSpans { unsigned int w[4]; };

TS_HD RowSpans spans_none() {
    RowSpans s;
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0u;
    return s;
}
TS_HD RowSpans spans_fallback() {
    RowSpans s = spans_none();
    s.w[0] = (unsigned int)kSpanFallback << 16;
    return s;
}
TS_HD int spans_rows(const RowSpans& s) { return (int)((s.w[0] >> 16) & 0xffu); }       // 0, 1..6 or kSpanFallback
TS_HD int spans_first_row(const RowSpans& s) { return (int)(s.w[0] & 0xffffu); }        // relative to cam.tile_row0
// row k < spans_rows(s): [lo, hi); hi <= lo for an empty row
TS_HD void spans_row(const RowSpans& s, int k, int& lo, int& hi) {
    const unsigned int v = (s.w[1 + (k >> 1)] >> (16 * (k & 1))) & 0xffffu;
    lo = (int)(v & 0xffu);
    hi = (int)(v >> 8) + 1;
}

// the same, consuming: the next row's range, the rows behind it moved down (no indexing by a run-time row in registers)
TS_HD void spans_pop_row(RowSpans& s, int& lo, int& hi) {
    lo = (int)(s.w[1] & 0xffu);
    hi = (int)((s.w[1] >> 8) & 0xffu) + 1;
    s.w[1] = (s.w[1] >> 16) | (s.w[2] << 16);
    s.w[2] = (s.w[2] >> 16) | (s.w[3] << 16);
    s.w[3] >>= 16;
}

// The record of a Gaussian from the operands of walk_chunk: (x, y) = xys[i] = words 0, 1 of the packed record, op, cxx,
// cxy, cyy = its words 2..5, radius = radii[i]; tight = the lists are tightened with the records (TS_FRAME_TIGHT).
TS_HD RowSpans make_row_spans(bool tight, float x, float y, float op, float cxx, float cxy, float cyy, int radius,
                              int tile_bounds_x, int tile_bounds_y, int tile_row0, int tile_rows) {
    if (radius <= 0) return spans_none();
    const TileBox b = tile_bbox(x, y, (float)radius, tile_bounds_x, tile_bounds_y, tile_row0, tile_rows);
    if (b.maxy <= b.miny || b.maxx <= b.minx) return spans_none();
    const TightTest t(tight, x, y, op, cxx, cxy, cyy, (float)radius);
    if (t.cull_all) return spans_none();
    const int rows = b.maxy - b.miny, first = b.miny - tile_row0;
    if (rows > kSpanRows || first > 0xffff) return spans_fallback();
    RowSpans s = spans_none();
    s.w[0] = (unsigned int)first | ((unsigned int)rows << 16);
    bool fits = true;
#pragma unroll
    for (int k = 0; k < kSpanRows; ++k) {
        if (k < rows) {
            int lo, hi;
            t.row_range(b.miny + k, b.minx, b.maxx, lo, hi);
            unsigned int v = kSpanEmptyRow;
            if (hi > lo) {
                fits = fits && hi <= kSpanCols;
                v = (unsigned int)lo | ((unsigned int)(hi - 1) << 8);
            }
            s.w[1 + (k >> 1)] |= (v & 0xffffu) << (16 * (k & 1));
        }
    }
    return fits ? s : spans_fallback();
}

}  // namespace ts
