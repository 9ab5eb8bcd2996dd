"""The undistortion arithmetic without a GPU: csrc/undistort_math.h, built for the host from
tests/hostmath/undistort.cpp, against the numpy oracle (tests/undistort_oracle.py) run in float32; the fixed-point inverse;
the two new camera matrices of tinysplat_amd/dataset.py; the border overshoot; the tolerance of the GPU tests; the C
entry's argument checks."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import undistort_cases as UC
import undistort_oracle as UO
from tinysplat_amd import dataset as D

ROOT = Path(__file__).resolve().parent.parent
F32P, F64P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
I32P, U8P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
W, H = UO.SIZE


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """g++ build of tests/hostmath/undistort.cpp: the kernel's header compiled for the host."""
    so = tmp_path_factory.mktemp("undistort") / "_undistort.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "undistort.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i, i64 = ctypes.c_int, ctypes.c_int64
    lib.ud_coefficients.restype, lib.ud_coefficients.argtypes = i, [i, F64P, F64P]
    lib.ud_supersample.restype, lib.ud_supersample.argtypes = i, [i, i, i, i]
    lib.ud_distort.restype, lib.ud_distort.argtypes = None, [i64, F32P, F32P, F32P, F32P, F32P]
    lib.ud_map.restype, lib.ud_map.argtypes = None, [i64, F32P, F32P, F32P, F32P, F32P, F32P, F32P, F32P, F32P]
    lib.ud_weights.restype, lib.ud_weights.argtypes = None, [i64, F32P, F32P, i, I32P, I32P, F32P]
    lib.ud_remap.restype, lib.ud_remap.argtypes = None, [U8P, i, i, F32P, F32P, F32P, i, i, F32P, U8P]
    return lib


def _p(a, t):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(t)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the header
@pytest.mark.parametrize("name", list(UO.CAMERAS))
def test_header_map_is_bit_equal_to_the_float32_oracle(host, name):
    k, d = UO.CAMERAS[name]
    sk, dk, dd = UO.as_kernel_inputs(k, UO.new_matrix_reference(k, d, W, H), d)
    rng = np.random.default_rng(list(UO.CAMERAS).index(name))
    n = 10_000
    u = _f32(rng.uniform(-3, W + 2, n))
    v = _f32(rng.uniform(-3, H + 2, n))
    u[:200], v[:200] = np.round(u[:200]), np.round(v[:200])                  # pixel centres, as the kernel asks at n = 1
    got = [np.zeros(n, np.float32) for _ in range(4)]
    host.ud_map(n, _p(_f32(sk), F32P), _p(_f32(dk), F32P), _p(_f32(dd), F32P), _p(u, F32P), _p(v, F32P),
                *[_p(g, F32P) for g in got])
    (sx, ex), (sy, ey) = UO.map_points(sk, dk, dd, u, v, np.float32)
    for g, want, what in zip(got, (sx, ex, sy, ey), ("sx", "ex", "sy", "ey")):
        assert want.dtype == np.float32 and np.array_equal(_bits(g), _bits(want)), (name, what)
    # the same points' distortion alone, and the weights of the clamped coordinates on both axes
    x, y = _f32((u - np.float32(dk[2])) / np.float32(dk[0])), _f32((v - np.float32(dk[3])) / np.float32(dk[1]))
    xd, yd = np.zeros(n, np.float32), np.zeros(n, np.float32)
    host.ud_distort(n, _p(_f32(dd), F32P), _p(x, F32P), _p(y, F32P), _p(xd, F32P), _p(yd, F32P))
    wx, wy = UO.distort(dd, x, y, np.float32)
    assert np.array_equal(_bits(xd), _bits(wx)) and np.array_equal(_bits(yd), _bits(wy))
    for s, e, size in ((sx, ex, W), (sy, ey, H)):
        i0, i1, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        host.ud_weights(n, _p(_f32(s), F32P), _p(_f32(e), F32P), size, _p(i0, I32P), _p(i1, I32P), _p(w, F32P))
        o0, o1, ow = UO._axis(s, e, size, np.float32)
        assert np.array_equal(i0, o0) and np.array_equal(i1, o1) and np.array_equal(_bits(w), _bits(ow))
        assert i0.min() >= 0 and i1.max() <= size - 1 and (i0 == 0).any() and (i1 == size - 1).any()


def test_header_weights_at_the_edges(host):
    """NaN and infinities, whole numbers with an error either side, a size past float32's integers: indices stay inside."""
    s = _f32([np.nan, -np.inf, np.inf, -1.0, 0.0, 0.0, 5.0, 5.0, 9.0, 9.0, 9.0, 8.9999990, 3.25, 1e30])
    e = _f32([np.nan, 0.0, np.nan, 0.0, -1e-8, 1e-8, -1e-7, 1e-7, -1e-7, 1e-7, 0.0, 5e-7, 0.0, 0.0])
    n = s.shape[0]
    for size in (10, 1, (1 << 25) + 1):
        i0, i1, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        host.ud_weights(n, _p(s, F32P), _p(e, F32P), size, _p(i0, I32P), _p(i1, I32P), _p(w, F32P))
        o0, o1, ow = UO._axis(s, e, size, np.float32)
        assert np.array_equal(i0, o0) and np.array_equal(i1, o1) and np.array_equal(_bits(w), _bits(ow)), size
        assert i0.min() >= 0 and i1.max() <= size - 1 and np.isfinite(w).all() and w.min() >= 0 and w.max() < 1
    i0, i1, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    host.ud_weights(n, _p(s, F32P), _p(e, F32P), 10, _p(i0, I32P), _p(i1, I32P), _p(w, F32P))
    assert i0[:6].tolist() == [0, 0, 9, 0, 0, 0] and w[:6].tolist() == [0, 0, 0, 0, 0, 0]
    assert (i0[6], i1[6]) == (4, 5) and w[6] == np.float32(1) - np.float32(1e-7)         # 5 - 1e-7: the cell below
    assert (i0[7], w[7]) == (5, np.float32(1e-7))
    assert (i0[8], i1[8]) == (8, 9) and (i0[9], i1[9], w[9]) == (9, 9, 0)               # 9 + 1e-7: past the border
    assert (i0[12], i1[12], w[12]) == (3, 4, 0.25) and (i0[13], w[13]) == (9, 0)


@pytest.mark.parametrize("name", list(UC.cases()))
def test_header_image_is_bit_equal_to_the_float32_oracle(host, name):
    """The whole pixel - sub-sample offsets, taps, sums, the division, the rounding to a byte - as the kernel calls it."""
    src, sk, dk, d, (ow, oh) = UC.cases()[name]
    h, w = src.shape[:2]
    assert host.ud_supersample(w, h, ow, oh) == UO.supersample(w, h, ow, oh)
    levels, got = np.zeros((oh, ow, 3), np.float32), np.zeros((oh, ow, 3), np.uint8)
    host.ud_remap(_p(src, U8P), h, w, _p(_f32(sk), F32P), _p(_f32(dk), F32P), _p(_f32(d), F32P), oh, ow,
                  _p(levels, F32P), _p(got, U8P))
    want = UO.remap(src, sk, dk, d, (ow, oh), np.float32)
    assert want.dtype == np.float32 and np.array_equal(_bits(levels), _bits(want))
    assert np.array_equal(got, UO.to_bytes(want))
    assert levels.min() >= 0 and levels.max() <= 255
    UO.check_uint8(got, UC.oracle(name), UC.TAU, f"host {name}")


def test_supersample_counts(host):
    for w, h, ow, oh in ((97, 61, 97, 61), (97, 61, 40, 25), (97, 61, 96, 60), (4000, 3000, 1600, 1200),
                         (4000, 3000, 100, 75), (10, 10, 20, 20), (97, 61, 1, 1)):
        assert host.ud_supersample(w, h, ow, oh) == UO.supersample(w, h, ow, oh)
    assert host.ud_supersample(97, 61, 40, 25) == 3 and host.ud_supersample(97, 61, 96, 60) == 2
    assert host.ud_supersample(4000, 3000, 100, 75) == 8 and host.ud_supersample(10, 10, 20, 20) == 1


def test_colmap_parameters_onto_coefficients(host):
    params = {0: [500.0, 320, 240], 1: [500.0, 510, 320, 240], 2: [500.0, 320, 240, -0.1],
              3: [500.0, 320, 240, -0.1, 0.02], 4: [500.0, 510, 320, 240, -0.1, 0.02, 0.003, -0.004],
              6: [500.0, 510, 320, 240, -0.1, 0.02, 0.003, -0.004, 0.001, 0.02, 0.005, 0.0007]}
    want = {0: [0] * 8, 1: [0] * 8, 2: [-0.1] + [0] * 7, 3: [-0.1, 0.02] + [0] * 6,
            4: [-0.1, 0.02, 0.003, -0.004, 0, 0, 0, 0], 6: [-0.1, 0.02, 0.003, -0.004, 0.001, 0.02, 0.005, 0.0007]}
    for model, p in params.items():
        got = D.distortion_coefficients(model, p)
        assert got.tolist() == [float(v) for v in want[model]], model
        extra = np.ascontiguousarray(p[D._MODELS[model][0] + 2:] + [0.0], dtype=np.float64)
        out = np.full(8, 7.0)
        assert host.ud_coefficients(model, _p(extra, F64P), _p(out, F64P)) == 0 and out.tolist() == got.tolist()
    for model in (5, 7, 8, 9, 10, 11):
        assert host.ud_coefficients(model, _p(np.zeros(12), F64P), _p(np.zeros(8), F64P)) == -1
        with pytest.raises(ValueError, match="not supported"):
            D.distortion_coefficients(model, np.zeros(12))
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        D.distortion_coefficients(5, np.zeros(8))


# ------------------------------------------------------------------------------------------------ inverse and matrices
@pytest.mark.parametrize("name", list(UO.CAMERAS))
def test_distort_inverts_undistort_on_the_grid(name):
    (fx, fy, cx, cy), d = UO.CAMERAS[name]
    i = np.arange(9)
    gx, gy = np.meshgrid(i * (W - 1) / 8, i * (H - 1) / 8)
    xd, yd = (gx - cx) / fx, (gy - cy) / fy
    for undistort in (lambda: UO.undistort(d, xd, yd)[:2], lambda: D.undistort_points(np.asarray(d, float), xd, yd)):
        x, y = undistort()
        bx, by = UO.distort(d, x, y)
        assert max(np.abs(bx - xd).max(), np.abs(by - yd).max()) < 1e-9
    its = UO.undistort(d, xd, yd)[2]
    print(f"{name}: the inverse took {its} iterations")
    assert its <= 20
    px, py = D.distort_points(np.asarray(d, float), x, y)
    assert np.abs(px - bx).max() < 1e-15 and np.abs(py - by).max() < 1e-15


@pytest.mark.parametrize("name", list(UO.CAMERAS))
def test_new_camera_matrices_match_the_restatement(name):
    k, d = UO.CAMERAS[name]
    k, d = np.asarray(k), np.asarray(d, dtype=float)
    ref, cen = D.optimal_new_camera_matrix(k, d, W, H), D.centered_camera_matrix(k, d, W, H)
    assert np.allclose(ref, UO.new_matrix_reference(k, d, W, H), rtol=1e-12, atol=0)
    assert np.allclose(cen, UO.new_matrix_center(k, d, W, H), rtol=1e-12, atol=0)
    assert cen[2] == (W - 1) / 2 and cen[3] == (H - 1) / 2
    # alpha = 0: the inner rectangle's sides land on the frame's sides
    (x0, x1, y0, y1), _ = UO.grid_rectangle(k, d, W, H)
    assert abs(ref[0] * x0 + ref[2]) < 1e-9 and abs(ref[0] * x1 + ref[2] - (W - 1)) < 1e-9
    assert abs(ref[1] * y0 + ref[3]) < 1e-9 and abs(ref[1] * y1 + ref[3] - (H - 1)) < 1e-9
    # the centred frame lies inside the rectangle and touches it on one side per axis
    sides = np.array([cen[0] * x0 + cen[2], W - 1 - (cen[0] * x1 + cen[2]), cen[1] * y0 + cen[3], H - 1 - (cen[1] * y1 + cen[3])])
    assert sides.max() < 1e-9 and abs(sides[:2].max()) < 1e-9 and abs(sides[2:].max()) < 1e-9


def test_matrix_of_the_undistorted_camera_is_the_identity():
    k, d = UO.CAMERAS["none"]
    assert np.abs(D.optimal_new_camera_matrix(np.asarray(k), np.zeros(8), W, H) - np.asarray(k)).max() < 1e-9
    assert np.abs(UO.new_matrix_reference(k, d, W, H) - np.asarray(k)).max() < 1e-9


@pytest.mark.parametrize("name", list(UO.CAMERAS))
def test_source_coordinates_stay_within_a_twentieth_of_a_pixel_of_the_frame(name):
    """The replicate border is read only where the inner rectangle, found on a 9 x 9 grid, bulges between grid points."""
    k, d = UO.CAMERAS[name]
    vv, uu = np.meshgrid(np.arange(H, dtype=float), np.arange(W, dtype=float), indexing="ij")
    worst = 0.0
    for dst in (UO.new_matrix_reference(k, d, W, H), UO.new_matrix_center(k, d, W, H)):
        (sx, ex), (sy, ey) = UO.map_points(k, dst, d, uu, vv)
        sx, sy = sx + ex, sy + ey
        worst = max(worst, -sx.min(), sx.max() - (W - 1), -sy.min(), sy.max() - (H - 1))
    print(f"{name}: overshoot {worst:.4f} px")
    assert worst <= 0.05


# ------------------------------------------------------------------------------------------------ the tolerance
def test_tolerance_is_four_times_the_float32_error():
    worst = {}
    for name, (src, sk, dk, d, size) in UC.cases().items():
        worst[name] = float(np.abs(UO.remap(src, sk, dk, d, size, np.float32).astype(np.float64) - UC.oracle(name)).max())
    print("float32 oracle against float64 oracle, levels: " + ", ".join(f"{k} {v:.5f}" for k, v in worst.items()))
    top = max(worst.values())
    assert 0.95 * UC.F32_ERROR <= top <= UC.F32_ERROR and UC.TAU == 4 * UC.F32_ERROR
    assert UC.TAU <= 0.02                               # 2 tau of the values may sit that close to a rounding boundary
    assert {n: UO.supersample(c[0].shape[1], c[0].shape[0], *c[4]) for n, c in UC.cases().items()} == {
        "barrel": 1, "pincushion": 1, "opencv": 1, "full": 1, "none": 1, "opencv_max40": 3, "opencv_max96": 2,
        "opencv_5x3": 1, "opencv_257x130": 1}
    assert UC.cases()["opencv_max40"][4] == (40, 25) and UC.cases()["opencv_max96"][4] == (96, 60)


# ------------------------------------------------------------------------------------------------ the entry, the wrapper
def test_entry_argument_checks():
    """None of these needs a device: every refusal returns before a launch."""
    from tinysplat_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    k, d = (ctypes.c_float * 4)(80, 78, 48, 30), (ctypes.c_float * 8)()
    # src, src_h, src_w, src_k, dst_k, dist, out_h, out_w, out_float, out, stream
    good = [p, 61, 97, k, k, d, 61, 97, 0, p, None]
    for i in (0, 3, 4, 5, 9):
        a = list(good)
        a[i] = None
        assert lib.ts_undistort_image(*a) == -1, i
    for i in (1, 2, 6, 7):
        for bad in (0, -5):
            a = list(good)
            a[i] = bad
            assert lib.ts_undistort_image(*a) == -1, (i, bad)
    for i, j in ((1, 2), (6, 7)):
        a = list(good)
        a[i], a[j] = 1 << 16, 1 << 15                                      # 2^31 pixels
        assert lib.ts_undistort_image(*a) == -1, (i, j)
    a = list(good)
    a[9] = ctypes.c_void_p(260)                                            # out not 16-byte aligned
    assert lib.ts_undistort_image(*a) == -1
    assert lib.ts_abi_version() == 9 == _lib.ABI_VERSION


def test_cpu_tensors_and_bad_arguments_are_refused():
    k = (80, 78, 48, 30)
    img = torch.zeros((61, 97, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.undistort_image(img, k, k, [0.0] * 8, (97, 61))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.undistort_image(img, k, k, [0.0] * 8, (97, 61), dtype=torch.float32)
