"""Seeded inputs of the appearance tests, their float64 references (computed once, shared and
read-only), the error bounds, and the g++ build of tests/hostmath/appearance.cpp that the CPU and GPU tests compare with."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np

import appearance_oracle as AO

ROOT = Path(__file__).resolve().parent.parent
DEFAULT = (8, 16, 16)
# 37x53 with the default grid: cells 2 to 4 pixels wide, odd sizes, one partial tile; 270x480: several workgroups feed one
# vertex (8 x 34 tiles); the three small grids have each axis at size 1 once
CASES = ((37, 53, DEFAULT), (270, 480, DEFAULT), (37, 53, (1, 1, 1)), (37, 53, (2, 1, 3)), (37, 53, (3, 2, 1)))
IDS = [f"{h}x{w}-{'x'.join(map(str, g))}" for h, w, g in CASES]

EPS = 2.0 ** -24
# K = the float32 roundings on a term's longest path in csrc/appearance_math.h, plus one (counted in the header's code):
#   out    the three nested lerps a + t * (b - a): 3 x (difference, product, sum) = 9; the product with in_k: 10; the three
#          sums of ts_app_apply: 13
K_OUT = 13 + 1
#   v_I    the guidance term: a level matrix (two lerps: 6), A1 - A0: 7, its product with vA: 8, the eleven sums behind the
#          first product: 19, the product with (L - 1) lum_k: 20, the sum with the direct term: 21 (the direct term alone: 13)
K_VI = 21 + 1
#   v_G    a term is fz fy fx vA: the three factors 1 - t (one rounding each; t is the definition's float32) and the product
#          vA = V_r in_k; the factors' product and the sums are double (2^-53 per operation: inside the "plus one")
K_VG = 4 + 1
PLANTED = ((0, 0, (0.0, 0.0, 0.0)), (1, 2, (1.0, 1.0, 1.0)), (2, 3, (40.0, -25.0, 7.0)))   # both clamps; far outside
MAX_EXCLUDED = 0.005                                     # of the pixels, from the v_I comparison


@functools.lru_cache(maxsize=None)
def inputs(h, w, grid):
    """-> (image [h, w, 3] uniform in [-0.2, 1.3] with the planted pixels, grid [L, Gh, Gw, 12] = identity + noise,
    v_out [h, w, 3]), float32 and read-only."""
    rng = np.random.default_rng(1000 * h + w + 7 * sum(grid))
    image = rng.uniform(-0.2, 1.3, (h, w, 3)).astype(np.float32)
    for y, x, value in PLANTED:
        image[y, x] = value
    G = identity(grid) + (0.3 * rng.standard_normal(grid + (12,))).astype(np.float32)
    v_out = rng.standard_normal((h, w, 3)).astype(np.float32)
    for a in (image, G, v_out):
        a.setflags(write=False)
    return image, G, v_out


def identity(grid):
    return np.broadcast_to(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), tuple(grid) + (12,)).copy()


@functools.lru_cache(maxsize=None)
def reference(h, w, grid):
    """The oracle on ``inputs(h, w, grid)``: dict(out, out_abs, v_image, v_image_abs, v_grid, v_grid_abs, compare) with
    ``compare`` the pixels whose v_I is compared: |w - rint(w)| > 4 2^-24 max(1, L - 1); with L = 1, where w = 0 for every
    pixel and the luminance has no cell to change, all of them."""
    image, G, v_out = inputs(h, w, grid)
    out, out_abs = AO.forward(image, G)
    ref = dict(AO.backward(image, G, v_out), out=out, out_abs=out_abs)
    lw = AO.level(image, grid[0])["w"].astype(np.float64)
    with np.errstate(all="ignore"):
        ref["compare"] = (np.abs(lw - np.rint(lw)) > 4 * EPS * max(1, grid[0] - 1)) | (grid[0] == 1)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check_against_oracle(ref, out=None, v_image=None, v_grid=None):
    """The float32 results against the float64 oracle at the bounds above; prints every figure before it asserts."""
    if out is not None:
        ratio = float(np.max(np.abs(out.astype(np.float64) - ref["out"]) / (EPS * ref["out_abs"] + 1e-300)))
        print(f"out: max error {ratio:.2f} x 2^-24 x sum|terms| (bound {K_OUT})")
        assert ratio <= K_OUT
    if v_image is not None:
        keep = ref["compare"]
        excluded = 1.0 - float(keep.mean())
        print(f"v_I: {int((~keep).sum())} of {keep.size} pixels excluded")
        assert excluded <= MAX_EXCLUDED, excluded
        err = np.abs(v_image.astype(np.float64) - ref["v_image"]) / (EPS * ref["v_image_abs"] + 1e-300)
        ratio = float(np.max(err[keep]))
        print(f"v_I: max error {ratio:.2f} x 2^-24 x sum|terms| (bound {K_VI})")
        assert ratio <= K_VI
    if v_grid is not None:
        bound = K_VG * EPS * ref["v_grid_abs"] + EPS * np.abs(ref["v_grid"])
        err = np.abs(v_grid.astype(np.float64) - ref["v_grid"])
        ratio = float(np.max(err / (bound + 1e-300)))
        print(f"v_G: max error {ratio:.3f} of the bound {K_VG} x 2^-24 x sum|terms| + 2^-24 |v_G|")
        assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------- the host build
F32P, F64P, I32P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def build_host(directory):
    """g++ build of tests/hostmath/appearance.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_appearance.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "appearance.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i, f, v = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    lib.ah_axis.restype, lib.ah_axis.argtypes = None, [i, i, i, I32P, I32P, F32P]
    lib.ah_level.restype, lib.ah_level.argtypes = None, [f, f, f, i, I32P, I32P, F32P, I32P]
    lib.ah_ws_bytes.restype, lib.ah_ws_bytes.argtypes = ctypes.c_int64, [i] * 5
    lib.ah_fwd.restype, lib.ah_fwd.argtypes = None, [i] * 5 + [F32P] * 3
    lib.ah_bwd.restype, lib.ah_bwd.argtypes = None, [i] * 5 + [F32P] * 5
    lib.ah_tv.restype, lib.ah_tv.argtypes = None, [i] * 3 + [F32P, f, F32P, F64P, F32P]
    lib.ah_fit_sums.restype, lib.ah_fit_sums.argtypes = None, [i, i, F32P, v, i, F64P]
    return lib


def _f(a):
    return a.ctypes.data_as(F32P)


def host_forward(lib, image, grid):
    image, grid = np.ascontiguousarray(image, np.float32), np.ascontiguousarray(grid, np.float32)
    out = np.empty_like(image)
    lib.ah_fwd(image.shape[0], image.shape[1], *grid.shape[:3], _f(image), _f(grid), _f(out))
    return out


def host_backward(lib, image, grid, v_out):
    image, grid, v_out = (np.ascontiguousarray(a, np.float32) for a in (image, grid, v_out))
    v_image, v_grid = np.empty_like(image), np.empty_like(grid)
    lib.ah_bwd(image.shape[0], image.shape[1], *grid.shape[:3], _f(image), _f(grid), _f(v_out), _f(v_image), _f(v_grid))
    return v_image, v_grid


def host_tv(lib, grid, weight=1.0, v_in=None):
    grid = np.ascontiguousarray(grid, np.float32)
    v_in = None if v_in is None else np.ascontiguousarray(v_in, np.float32)
    value, v_out = np.zeros(1, np.float64), np.empty_like(grid)
    lib.ah_tv(*grid.shape[:3], _f(grid), weight, None if v_in is None else _f(v_in), value.ctypes.data_as(F64P), _f(v_out))
    return float(value[0]), v_out


def host_fit_sums(lib, image, target):
    image, target = np.ascontiguousarray(image, np.float32), np.ascontiguousarray(target)
    out = np.zeros(22, np.float64)
    lib.ah_fit_sums(image.shape[0], image.shape[1], _f(image), target.ctypes.data, int(target.dtype == np.uint8),
                    out.ctypes.data_as(F64P))
    return out


@functools.lru_cache(maxsize=None)
def fit_inputs(h=61, w=83):
    """-> (image float32 [h, w, 3], float32 target, uint8 target): more than one wave of the fit (2048 pixels each)."""
    rng = np.random.default_rng(h * w)
    image = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    target = np.clip(0.8 * image + 0.1 + 0.05 * rng.standard_normal((h, w, 3)), 0, 1).astype(np.float32)
    u8 = np.rint(target * 255.0).astype(np.uint8)
    for a in (image, target, u8):
        a.setflags(write=False)
    return image, target, u8
