"""Seeded inputs of the depth-prior tests, their references (computed once and shared), the bound
of the fit, and the g++ build of tests/hostmath/depth_prior.cpp that the CPU tests compare with."""
import ctypes
import functools
import math
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import depth_prior_oracle as DO

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "depth_prior.npz"

SIZES = ((40, 24), (128, 96))                                   # (width, height)
COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 5000)    # survivors m: around the wave, the workgroup, many per thread
FAMILIES = ("outliers", "ties", "equal_x", "linear")
LINEAR_A, LINEAR_B, LINEAR_STEP = 1.75, 0.125, 0.25             # y = a x + b on x in multiples of LINEAR_STEP: exact in float32


# ---------------------------------------------------------------------------------------------------------- fit inputs
@functools.lru_cache(maxsize=None)
def fit_case(family, m):
    """-> (x float32 [m], z float32 [m], w float64 [m]); all read-only"""
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + m)
    w = 1.0 / rng.uniform(0.1, 2.0, m)
    if family == "outliers":                                    # smooth data, 20 % of it far off the line
        x = rng.uniform(0.5, 8.0, m)
        y = 1.6 * x + 0.4 + rng.normal(0.0, 0.02, m)
        out = rng.random(m) < 0.2
        y = np.where(out, y + rng.uniform(-3.0, 3.0, m), y)
        y = np.maximum(y, 0.05)
    elif family == "ties":                                      # x in quarters and y in eighths: many equal residuals
        x = np.round(rng.uniform(0.5, 8.0, m) * 4) / 4
        y = np.maximum(np.round((1.3 * x + 0.7 + rng.normal(0.0, 0.3, m)) * 8) / 8, 0.125)
    elif family == "equal_x":
        x = np.full(m, 2.5)
        y = rng.uniform(0.5, 9.0, m)
    else:                                                       # exactly linear: the optimum is 0 at (a, b)
        x = np.round(rng.uniform(0.25, 8.0, m) / LINEAR_STEP) * LINEAR_STEP
        if m >= 2:
            x[0], x[1] = 0.5, 7.75                              # never all equal
        y = LINEAR_A * x + LINEAR_B
    x, z = x.astype(np.float32), y.astype(np.float32)
    if family == "linear":
        assert np.all(z.astype(np.float64) == LINEAR_A * x.astype(np.float64) + LINEAR_B)
    for a in (x, z, w):
        a.setflags(write=False)
    return x, z, w


def fit_y(z, disparity=False):
    z = np.asarray(z).astype(np.float64)
    return 1.0 / z if disparity else z


@functools.lru_cache(maxsize=None)
def fit_reference(family, m, disparity=False):
    """-> (f*, s, t) of the oracle, None for m = 0"""
    if m == 0:
        return None
    x, z, w = fit_case(family, m)
    return DO.optimum(x, fit_y(z, disparity), w)


def fit_bound(s, x, w, f):
    """How far above the exact optimum a search that stops at adjacent doubles may end, plus the rounding of the sums:
    ulp(s) mean(w) (max x - min x) - g(s) = min_t f(s, t) is Lipschitz in s with the constant mean(w |x - x_k|) <=
    mean(w) (max x - min x) - and 4 m 2^-53 f."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return math.ulp(s) * float(np.mean(w)) * float(x.max() - x.min()) + 4 * len(x) * 2.0 ** -53 * f


def linear_bounds(x):
    """|s - a| and |t - b| allowed on the exactly linear family.  A residual y_i - s x_i is one fma, correct to half an
    ulp of its value ~ b, and rounding is monotone, so two residuals are never ordered wrongly; they can only tie where
    |s - a| |x_i - x_k| < ulp(b).  x comes in steps of LINEAR_STEP, so for |s - a| >= ulp(b) / LINEAR_STEP the derivative
    test sees every sign as it is and the bisection keeps a inside its bracket: it ends within that distance plus the one
    ulp of the adjacent doubles.  t is then a residual b - (s - a) x_k, rounded."""
    x = np.asarray(x, dtype=np.float64)
    tol_s = math.ulp(LINEAR_B) / LINEAR_STEP + math.ulp(LINEAR_A)
    return tol_s, tol_s * float(np.abs(x).max()) + math.ulp(LINEAR_B)


def concat_cases(cases):
    """[(x, z, w), ...] -> x, z, w, offsets (numpy) of one batch"""
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int64)
    return (np.concatenate([c[0] for c in cases]).astype(np.float32), np.concatenate([c[1] for c in cases]).astype(np.float32),
            np.concatenate([c[2] for c in cases]).astype(np.float64), offsets)


# -------------------------------------------------------------------------------------------------------------- scenes
def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def scene_case(width, height, n_points, seed=0):
    """One camera and ``n_points`` visible points, made by back-projecting pixel positions that stay 0.2 px clear of
    every rounding boundary (float32 evaluation order cannot move a pixel), with collisions (points drawn with replacement
    over the pixels), and a share of points that must be dropped: outside the image, behind the camera, and with an error
    of 0, a negative one, inf and NaN.  -> a namespace: view float32 [4, 4], f_x, f_y, width, height, xyz float64 [n, 3],
    errors float64 [n], ids int64 [n] (the camera's visible_point_ids, in list order; sparse and unsorted), dense float32
    [height, width]."""
    rng = np.random.default_rng(7919 * seed + 31 * width + n_points)
    rot, trans = _rotation(rng), rng.uniform(-1.0, 1.0, 3)
    f_x, f_y = 0.9 * width, 0.85 * width
    u = rng.integers(0, width, n_points) + rng.uniform(-0.3, 0.3, n_points)
    v = rng.integers(0, height, n_points) + rng.uniform(-0.3, 0.3, n_points)
    z = rng.uniform(1.0, 6.0, n_points)
    kind = rng.random(n_points)
    u = np.where(kind < 0.04, u + width * rng.choice([-1.0, 1.0], n_points), u)            # outside, left or right
    v = np.where((kind >= 0.04) & (kind < 0.08), v + height * rng.choice([-1.0, 1.0], n_points), v)
    z = np.where((kind >= 0.08) & (kind < 0.11), -z, z)                                    # behind the camera
    errors = rng.uniform(0.1, 2.0, n_points)
    for lo, bad in ((0.11, 0.0), (0.12, -0.5), (0.13, np.inf), (0.14, np.nan)):
        errors = np.where((kind >= lo) & (kind < lo + 0.01), bad, errors)
    cam = np.stack([(u - width / 2) / f_x * z, (v - height / 2) / f_y * z, z], axis=1)
    xyz = (cam - trans) @ rot                                                             # R^T (cam - t)
    view = np.eye(4)
    view[:3, :3], view[:3, 3] = rot, trans
    ids = rng.choice(50 * max(n_points, 1), n_points, replace=False).astype(np.int64) + (1 << 31)
    dense = rng.uniform(0.5, 5.0, (height, width)).astype(np.float32)
    case = SimpleNamespace(view=view.astype(np.float32), f_x=float(f_x), f_y=float(f_y), width=width, height=height,
                           xyz=xyz, errors=errors, ids=ids, dense=dense, name=f"cam_{width}x{height}_{n_points}_{seed}")
    for a in (case.view, xyz, errors, ids, dense):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def scene_reference(width, height, n_points, seed=0):
    """the oracle's float32 restatement on a scene: (pixel int64, z float32, weight float64), row-major"""
    c = scene_case(width, height, n_points, seed)
    # the point cloud holds float64 positions; the reference converts them to float32 first (depth.py:83)
    row, col, z, e = DO.sparse(c.view, np.float32(c.f_x), np.float32(c.f_y), width, height, c.xyz.astype(np.float32),
                               c.errors, np.float32)
    out = (row * width + col, z.astype(np.float32), 1.0 / e)
    for a in out:
        a.setflags(write=False)
    return out


def z_tolerance(view, xyz):
    """float32 evaluations of z = R_2 . xyz + t_2 that differ in summation order or in their use of fma (the reference's is
    a BLAS matrix product): each carries at most four roundings of partial sums bounded by sum |R_2j| |xyz_j| + |t_2|"""
    view = np.asarray(view, dtype=np.float64)
    return 2 * 4 * 2.0 ** -24 * float((np.abs(view[2, :3]) * np.abs(xyz).max(axis=0)).sum() + abs(view[2, 3]))


def sample_tolerance(h, w, span=4.5, top=5.0):
    """float32 bilinear sampling against float64 on a map with values in (top - span, top): the source coordinate carries
    about three float32 roundings of a value below max(h, w), which moves the sample by at most that times the map's
    largest step ``span``; the interpolation's own five roundings are of values below ``top``"""
    return 2.0 ** -24 * (3 * max(h, w) * span + 5 * top)


BATCH = ((40, 24, 5000, 1), (128, 96, 5000, 1), (40, 24, 0, 1), (128, 96, 1, 1), (40, 24, 3, 1), (128, 96, 300, 1),
         (40, 24, 65, 1))                                      # 7 cameras of different sizes and point counts


# ------------------------------------------------------------------------------------------------------- the host build
F32P = ctypes.POINTER(ctypes.c_float)


def build_host(directory):
    """g++ build of tests/hostmath/depth_prior.cpp: the kernels' header compiled for the host"""
    so = Path(directory) / "_depth_prior.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "depth_prior.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i32, i64, f32, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    lib.dh_project.restype, lib.dh_project.argtypes = i64, [F32P, i32, i32, f32, f32, f32, f64, F32P]
    lib.dh_no_pixel.restype, lib.dh_no_pixel.argtypes = i64, []
    lib.dh_key.restype, lib.dh_key.argtypes = i64, [i32, i64, i32]
    lib.dh_key_pixel.restype, lib.dh_key_pixel.argtypes = i64, [i64]
    lib.dh_key_camera.restype, lib.dh_key_camera.argtypes = i32, [i64]
    lib.dh_key_run.restype, lib.dh_key_run.argtypes = i64, [i64]
    lib.dh_sample.restype, lib.dh_sample.argtypes = f32, [F32P, i32, i32, i32, i32, i32, i32]
    lib.dh_order_key.restype, lib.dh_order_key.argtypes = ctypes.c_uint64, [f64]
    lib.dh_order_value.restype, lib.dh_order_value.argtypes = f64, [ctypes.c_uint64]
    lib.dh_apply.restype, lib.dh_apply.argtypes = f32, [f64, f64, f32, i32]
    return lib


def host_camera(case):
    """the 14 floats of a camera's row: the view matrix's 3 x 4 top, f_x, f_y"""
    row = np.concatenate([case.view[:3, :4].reshape(-1), [case.f_x, case.f_y]]).astype(np.float32)
    return row, row.ctypes.data_as(F32P)
