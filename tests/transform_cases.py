"""Scenes and transforms shared by tests/test_transform_cpu.py and tests/test_gpu_transform.py, the g++ build of
tests/hostmath/transform.cpp and the comparison of a result with the float64 oracle under the bounds of DESIGN.md 6t."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np

import transform_oracle as TO
from tinysplat_amd.edit import Sim3, kernel_arguments

ROOT = Path(__file__).resolve().parent.parent
F32P = ctypes.POINTER(ctypes.c_float)
U8P = ctypes.POINTER(ctypes.c_uint8)
FIELDS = ("means", "scales", "quats", "rest")

# the transform of the render checks: r ~ (0.3, -0.5, 0.7, 0.2), t = (0.5, -1, 2), s in {1, 2.5, 0.4}
QUAT = (0.3, -0.5, 0.7, 0.2)
TRANSLATION = (0.5, -1.0, 2.0)
SCALES = (1.0, 2.5, 0.4)


def sim3(scale=2.5):
    return Sim3.from_quat(QUAT, TRANSLATION, scale)


def k_rest(degree):
    return (degree + 1) ** 2 - 1


def random_scene(n, degree, seed):
    """float32 arrays of a model's four tensors that a transform changes: means N(0, 3), log-scales U(-6, 0), quats
    N(0, 1) (not normalised, as a model stores them), colors_rest N(0, 0.1)."""
    g = np.random.default_rng(seed)
    return {"means": (3.0 * g.normal(size=(n, 3))).astype(np.float32),
            "scales": g.uniform(-6.0, 0.0, size=(n, 3)).astype(np.float32),
            "quats": g.normal(size=(n, 4)).astype(np.float32),
            "rest": (0.1 * g.normal(size=(n, k_rest(degree), 3))).astype(np.float32)}


EDGE_ROWS = 12


def edge_scene(degree):
    """Twelve rows around the corners of float32: zero, NaN, Inf and huge quaternions, denormal means, +-0, rows whose SH
    are all zero (rows 0..5) and SH rows with a NaN, an Inf and values of 1e-30."""
    sc = random_scene(EDGE_ROWS, degree, seed=99)
    inf, nan, tiny = np.float32(np.inf), np.float32(np.nan), np.float32(1e-40)
    sc["quats"][0] = 0.0
    sc["quats"][1] = (nan, 0.5, 0.5, 0.5)
    sc["quats"][2] = (inf, 1.0, -1.0, 0.0)
    sc["quats"][3] = (1e30, -1e30, 3e29, 1e-30)
    sc["quats"][4] = (-0.0, 0.0, -0.0, 1.0)
    sc["means"][5] = (tiny, -tiny, 3 * tiny)
    sc["means"][6] = (0.0, -0.0, 0.0)
    sc["means"][7] = (nan, 1.0, 2.0)
    sc["means"][8] = (1.0, inf, 2.0)
    sc["means"][9] = (-inf, inf, 0.0)
    sc["scales"][6] = (-0.0, 0.0, -80.0)
    sc["scales"][7] = (nan, inf, -inf)
    sc["rest"][:6] = 0.0
    sc["rest"][4, :, 1] = -0.0
    if sc["rest"].shape[1]:
        sc["rest"][10, 0, 0] = nan
        sc["rest"][10, -1, 2] = inf
        sc["rest"][11, :, :] = 1e-30
    return sc


def with_edges(n, degree, seed):
    """A random scene of n >= 3 * EDGE_ROWS rows with the edge rows at its start, across the 64-row boundary and at its end."""
    sc, edge = random_scene(n, degree, seed), edge_scene(degree)
    for f in FIELDS:
        sc[f][:EDGE_ROWS] = edge[f]
        if n >= 64 + EDGE_ROWS:
            sc[f][58:58 + EDGE_ROWS] = edge[f]
        sc[f][n - EDGE_ROWS:] = edge[f]
    return sc


def arguments(t, degree):
    """``kernel_arguments`` with the SH matrices also as a list of float32 (2l+1)^2 arrays."""
    xform, quat, log_scale, sh = kernel_arguments(t, degree)
    mats, at = [], 0
    for l in range(1, degree + 1):
        w = 2 * l + 1
        mats.append(sh[at:at + w * w].reshape(w, w))
        at += w * w
    return xform, quat, log_scale, sh, mats


def build_host(directory):
    """g++ build of tests/hostmath/transform.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_transform.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "transform.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.xh_transform.restype = ctypes.c_int
    lib.xh_transform.argtypes = [ctypes.c_int64, ctypes.c_int, F32P, F32P, ctypes.c_float, F32P, U8P] + [F32P] * 8
    lib.xh_box_mask.restype, lib.xh_box_mask.argtypes = None, [ctypes.c_int64, F32P, F32P, U8P]
    return lib


def _f(a):
    return a.ctypes.data_as(F32P)


def host_transform(lib, scene, xform, quat, log_scale, sh, mask=None):
    """The host build on a scene -> dict of float32 arrays."""
    src = {f: np.ascontiguousarray(scene[f], dtype=np.float32) for f in FIELDS}
    out = {f: np.full_like(src[f], 7.0) for f in FIELDS}
    n, kr = src["means"].shape[0], src["rest"].shape[1]
    sh = np.ascontiguousarray(sh, dtype=np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    code = lib.xh_transform(n, kr, _f(np.ascontiguousarray(xform)), _f(np.ascontiguousarray(quat)), float(log_scale),
                            _f(sh) if sh.size else None, None if m is None else m.ctypes.data_as(U8P),
                            *[_f(src[f]) for f in FIELDS], *[_f(out[f]) for f in FIELDS])
    assert code == 0
    return out


def host_box_mask(lib, box, means):
    means = np.ascontiguousarray(means, dtype=np.float32)
    inside = np.zeros(means.shape[0], dtype=np.uint8)
    lib.xh_box_mask(means.shape[0], _f(np.ascontiguousarray(box, dtype=np.float32)), _f(means), inside.ctypes.data_as(U8P))
    return inside.astype(bool)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN: the payload and sign of a NaN an operation produces are not
    defined by IEEE 754 and differ between an x86 host and the GPU (inf - inf is 0xffc00000 on one, 0x7fc00000 on the other)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))


def _within(got, ref, bound, what):
    got = np.asarray(got, dtype=np.float64)
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaNs differ"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: infinities differ"
    err = np.abs(got[finite] - ref[finite])
    over = err > bound[finite]
    assert not over.any(), f"{what}: {int(over.sum())} entries over the bound, worst ratio {np.max(err[over] / bound[finite][over]):.3g}"
    ratio = err / np.maximum(bound[finite], np.finfo(np.float64).tiny)
    return float(ratio.max()) if ratio.size else 0.0


def check_against_oracle(got, scene, xform, quat, log_scale, mats):
    """The bounds of DESIGN.md 6t with u = 2^-24, evaluated in float64 with the factor 1 / (1 - n u):
    |m' - ref| <= 4u (sum_k |M_ik m_k| + |t_i|); scales' == fl32(s + log s); |q' - ref| <= 4u sum |products|;
    |c'_j - ref| <= (2l+1) u sum_k |D_jk c_k|.  NaN and Inf entries must agree.  -> the worst error / bound per tensor."""
    u = TO.U
    ref = TO.transform(xform, quat, log_scale, mats, scene["means"], scene["scales"], scene["quats"], scene["rest"])
    worst = {}
    with np.errstate(all="ignore"):
        worst["means"] = _within(got["means"], ref["means"], 4 * u / (1 - 4 * u) * ref["means_mag"], "means")
        want = (scene["scales"].astype(np.float32) + np.float32(log_scale)).astype(np.float32)
        assert same_bits(got["scales"], want), "scales differ from fl32(s + log s)"
        assert np.array_equal(want.astype(np.float64)[np.isfinite(want)], ref["scales"][np.isfinite(want)].astype(np.float32))
        worst["quats"] = _within(got["quats"], ref["quats"], 4 * u / (1 - 4 * u) * ref["quats_mag"], "quats")
        width = np.zeros(scene["rest"].shape[1])
        for l in range(1, len(mats) + 1):
            width[l * l - 1:(l + 1) * (l + 1) - 1] = 2 * l + 1
        bound = (width * u / (1 - width * u))[None, :, None] * ref["rest_mag"]
        worst["rest"] = _within(got["rest"], ref["rest"], bound, "colors_rest")
    return worst

