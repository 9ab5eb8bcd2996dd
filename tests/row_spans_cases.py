"""Scaffolding shared by the tests of the span records (csrc/row_spans.h): the header's host build behind ctypes, and the
comparison of a set of records with the plain loops of the walk they replace (ts::tile_bbox, ts::TightTest, row_range as
binning.hip's walk_chunk runs them), record by record."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
F32P, I32P, U32P = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_int32, ctypes.c_uint32))
REF_CAP = 64            # rows of a box the reference keeps per Gaussian (only boxes of <= 6 rows are compared row by row)


def build_host(directory):
    """g++ build of tests/hostmath/row_spans.cpp, as tests/test_hostmath.py builds its library"""
    so = Path(directory) / "_row_spans.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "row_spans.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.rs_make.restype = None
    lib.rs_make.argtypes = [ctypes.c_int, F32P, ctypes.c_int, I32P] + [ctypes.c_int] * 5 + [U32P]
    lib.rs_decode.restype = ctypes.c_int
    lib.rs_decode.argtypes = [ctypes.c_int, U32P, ctypes.c_int, ctypes.c_int, I32P, I32P]
    lib.rs_reference.restype = None
    lib.rs_reference.argtypes = [ctypes.c_int, F32P, ctypes.c_int, I32P] + [ctypes.c_int] * 6 + [I32P, I32P, I32P]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def host_spans(lib, recs, radii, tight, tbx, tby, row0, rows):
    """recs [n, >= 6] float32, radii [n] int32 -> the records the shared routine fills, [n, 4] uint32"""
    recs = np.ascontiguousarray(recs, dtype=np.float32)
    radii = np.ascontiguousarray(radii, dtype=np.int32)
    spans = np.zeros((len(recs), 4), np.uint32)
    lib.rs_make(len(recs), _p(recs, F32P), recs.shape[1], _p(radii, I32P), int(tight), tbx, tby, row0, rows,
                _p(spans, U32P))
    return spans


def check_against_loops(lib, spans, recs, radii, tight, tbx, tby, row0, rows):
    """every record reproduces the (ty, lo, hi) triples of the plain loops exactly - through both decoders - or carries
    the fallback flag, and carries it exactly where the record cannot hold the Gaussian -> statistics"""
    recs = np.ascontiguousarray(recs, dtype=np.float32)
    radii = np.ascontiguousarray(radii, dtype=np.int32)
    spans = np.ascontiguousarray(spans, dtype=np.uint32)
    n = len(recs)
    want_n, want = np.zeros(n, np.int32), np.zeros((n, REF_CAP, 3), np.int32)
    box = np.zeros((n, 3), np.int32)
    lib.rs_reference(n, _p(recs, F32P), recs.shape[1], _p(radii, I32P), int(tight), tbx, tby, row0, rows, REF_CAP,
                     _p(want_n, I32P), _p(want, I32P), _p(box, I32P))
    nmax, ncols, flag = lib.rs_rows(), lib.rs_cols(), lib.rs_fallback()
    representable = (box[:, 0] <= nmax) & (box[:, 2] <= ncols) & (box[:, 1] <= 0xffff)
    for pop in (0, 1):
        got_n, got = np.zeros(n, np.int32), np.zeros((n, nmax, 3), np.int32)
        assert lib.rs_decode(n, _p(spans, U32P), row0, pop, _p(got_n, I32P), _p(got, I32P)) == 0
        assert np.array_equal(got_n < 0, ~representable), "the fallback flag is set exactly where the record cannot hold the rows"
        ok = representable
        assert np.array_equal(got_n[ok], want_n[ok])
        live = np.arange(nmax)[None, :, None] < want_n[ok][:, None, None]
        assert np.array_equal(np.where(live, got[ok], 0), np.where(live, want[ok][:, :nmax], 0))
    r = (spans[:, 0] >> 16) & 0xff
    assert np.array_equal(r[representable], box[representable, 0])          # R = 0 exactly where the walk skips
    return dict(fallback=int((~representable).sum()), skipped=int((representable & (box[:, 0] == 0)).sum()),
                rows=np.bincount(box[representable, 0], minlength=nmax + 1), widest=int(box[representable, 2].max()),
                empty_rows=int((box[representable, 0] - want_n[representable]).sum()), flag=flag)
