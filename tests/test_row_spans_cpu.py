"""The span record (csrc/row_spans.h) on the host: tests/hostmath/row_spans.cpp compiles the header with g++ as
tests/test_hostmath.py compiles its library.  Decoding a record must reproduce exactly the (ty, lo, hi) triples of the
plain ts::tile_bbox + ts::TightTest + row_range loops of the walk, or the record carries the fallback flag - and carries
it exactly where six rows or 256 columns do not hold the Gaussian.  4096 Gaussians of the adversarial families of
tests/cull_cases.py (needles at 45 degrees, far-away and huge-radius ones among them), on a full frame, on a stripe, on
an image of 257 tile columns, and as bounding-box lists.  No GPU."""
import subprocess

import numpy as np
import pytest

import cull_cases as C
import row_spans_cases as R

W, H = 1920, 1080
FAMILIES = ["needle_45", "far", "radius_edge", "axis_ratio", "tangent_bands", "extreme_in_band", "faint", "grid_centres"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("row_spans"))


def _gaussians(w, h, seed=0):
    parts = [C.tile_cases(f, seed + 31 * k, 4096 // len(FAMILIES), w, h) for k, f in enumerate(FAMILIES)]
    recs, radii = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(recs) == 4096
    radii[::97] = 0                                            # culled by the projection
    recs[5::89, 2] = 6.1e-6                                    # sigmoid(-12): TightTest::cull_all
    return recs, radii


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("w,h,stripe", [(W, H, None), (W, H, (20, 31)), (4112, 48, None), (400, 304, (5, 12))])
def test_records_reproduce_the_loops(lib, w, h, stripe, tight):
    recs, radii = _gaussians(w, h)
    tbx, tby = (w + 15) // 16, (h + 15) // 16
    row0, rows = (stripe[0], stripe[1] - stripe[0]) if stripe else (0, tby)
    spans = R.host_spans(lib, recs, radii, tight, tbx, tby, row0, rows)
    st = R.check_against_loops(lib, spans, recs, radii, tight, tbx, tby, row0, rows)
    print(f"[row spans] {w}x{h} stripe {stripe} tight {tight}: rows {st['rows'].tolist()}, fallback {st['fallback']}, "
          f"skipped {st['skipped']}, empty rows {st['empty_rows']}, widest hi {st['widest']}")
    # every branch of the record is taken by these inputs
    assert st["skipped"] > 40 and st["rows"][1:min(rows, 6) + 1].min() > 0
    if h > 48:
        assert st["fallback"] > 0                              # boxes of more than six rows
    if tight and h > 48:
        assert st["empty_rows"] > 0                            # the ellipse leaves a row of its box empty
    if w == 4112:
        assert st["widest"] == 256 and st["fallback"] > 0      # column 255 is held, column 256 is not


def test_layout_words(lib):
    """the layout the kernels and the documentation state: R in bits 16..23 of word 0 over the first row, six 16-bit
    rows of lo | (hi - 1) << 8, an empty row as lo = 1 over hi - 1 = 0"""
    # one round Gaussian at (100, 100), radius 30: box rows 4..8, columns 4..8 (trunc(6.25 -+ 1.875 [+ 1]))
    recs = np.array([[100.0, 100.0, 0.9, 0.01, 0.0, 0.01]], np.float32)
    s = R.host_spans(lib, recs, np.array([30], np.int32), False, 25, 19, 0, 19)[0]
    assert s[0] == (4 | (5 << 16))
    row = 4 | (8 << 8)
    assert s[1] == (row | (row << 16)) and s[2] == s[1] and s[3] == row
    # the same Gaussian in the stripe of rows 6..19: first row 0 of the stripe, three rows
    s = R.host_spans(lib, recs, np.array([30], np.int32), False, 25, 19, 6, 13)[0]
    assert s[0] == (0 | (3 << 16)) and s[3] == 0
    # culled, and not representable
    assert not R.host_spans(lib, recs, np.array([0], np.int32), True, 25, 19, 0, 19).any()
    s = R.host_spans(lib, recs, np.array([60], np.int32), False, 25, 19, 0, 19)[0]
    assert s[0] == (lib.rs_fallback() << 16) and not s[1:].any()


def test_standalone_program(tmp_path):
    """tests/hostmath/row_spans_main.cpp: the same comparison as a program of its own (the form in which the header is
    run under -fsanitize=address,undefined); built plainly here"""
    exe = tmp_path / "row_spans_main"
    d = R.ROOT / "tests" / "hostmath"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", str(d / "row_spans.cpp"),
                    str(d / "row_spans_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "row spans ok" in out.stdout
