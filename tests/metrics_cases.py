"""Seeded inputs of the metrics tests, their float64 references (computed once and shared), the
tolerances, and the g++ build of tests/hostmath/metrics.cpp that the CPU tests compare with."""
import ctypes
import functools
import math
import subprocess
from pathlib import Path

import numpy as np
import torch

import metrics_oracle as MO

ROOT = Path(__file__).resolve().parent.parent

# a one-pixel map; one map column more than a 64-column block (with its 10 halo columns) holds; row widths with
# 3 W mod 4 != 0 (75, 131, 333: byte rows start at every alignment); more than one row segment (200 - 10 map rows in
# segments of 8); more than one column block (96, 131, 333)
SHAPES = ((11, 11), (12, 75), (40, 40), (64, 96), (77, 131), (200, 333))

# mse and l1: each term carries at most two float32 roundings (the difference; the byte's quotient), 2 x 2^-24 = 1.2e-7
# relative, everything after them is double; 1e-6 leaves eight times that
REL_MSE_L1 = 1e-6
ABS_SSIM = 2e-6                    # the bar tests/test_gpu_training.py sets for this SSIM on these inputs
ABS_PSNR_DB = 1e-5                 # 10 / ln 10 x the relative bound on mse = 4.3e-6 dB
PSNR_OF_BYTE_ROUNDING = 20.0 * math.log10(510.0)        # |error| <= 0.5 / 255 -> psnr >= 54.15 dB


@functools.lru_cache(maxsize=None)
def inputs(h, w):
    """-> (image float32 [h, w, 3], target float32 [h, w, 3], the target rounded to uint8), as tests/test_gpu_training.py
    draws them."""
    g = torch.Generator().manual_seed(h * w)
    img = torch.rand(h, w, 3, generator=g)
    tgt = (img + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    u8 = (tgt * 255.0).round().to(torch.uint8)
    return img, tgt, u8


def bytes_as_float(u8):
    """The float32 quotients b / 255 of a uint8 tensor ON THE HOST (IEEE division: the entry's definition of a byte, and
    what dataset.Targets hands out there; on the device torch multiplies by the reciprocal instead)."""
    assert not u8.is_cuda
    return u8.to(torch.float32) / 255.0


@functools.lru_cache(maxsize=None)
def reference(h, w, byte_target):
    img, tgt, u8 = inputs(h, w)
    ref = MO.metrics(img, bytes_as_float(u8) if byte_target else tgt)
    ref.setflags(write=False)
    return ref


def with_depth(img, seed=3):
    """[h, w, 3] -> [h, w, 4] with a garbage fourth channel (huge values, an inf and a NaN)."""
    h, w, _ = img.shape
    d = 1e30 * torch.randn(h, w, 1, generator=torch.Generator().manual_seed(seed))
    d[0, 0, 0], d[-1, -1, 0] = float("inf"), float("nan")
    return torch.cat([img, d], dim=2).contiguous()


def check(got, ref):
    """The four values against the float64 reference, at the tolerances above."""
    got = np.asarray(got, dtype=np.float64)
    mse, l1, ssim, psnr = (float(v) for v in got)
    assert abs(mse - ref[0]) <= REL_MSE_L1 * ref[0], (mse, ref[0])
    assert abs(l1 - ref[1]) <= REL_MSE_L1 * ref[1], (l1, ref[1])
    assert abs(ssim - ref[2]) < ABS_SSIM, (ssim, ref[2])
    if ref[0] > 0:
        assert abs(psnr - ref[3]) < ABS_PSNR_DB, (psnr, ref[3])
    else:
        assert psnr == math.inf


# ------------------------------------------------------------------------------------------------------- the host build
F32P, F64P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)


def build_host(directory):
    """g++ build of tests/hostmath/metrics.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_metrics.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "metrics.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i, f = ctypes.c_int, ctypes.c_float
    lib.mh_byte_to_float.restype, lib.mh_byte_to_float.argtypes = f, [i]
    lib.mh_ssim_term.restype, lib.mh_ssim_term.argtypes = f, [f] * 5
    lib.mh_psnr.restype, lib.mh_psnr.argtypes = ctypes.c_double, [ctypes.c_double]
    lib.mh_waves.restype, lib.mh_waves.argtypes = ctypes.c_int64, [i, i]
    lib.mh_segment_rows.restype, lib.mh_segment_rows.argtypes = i, [i, i]
    lib.mh_image_metrics.restype, lib.mh_image_metrics.argtypes = i, [i, i, i, F32P, ctypes.c_void_p, i, F64P]
    return lib


def host_metrics(lib, image, target):
    """image: float32 [h, w, 3 or 4] tensor; target: float32 or uint8 [h, w, 3] tensor -> float64 [4]."""
    image, target = image.contiguous().numpy(), target.contiguous().numpy()
    h, w, xs = image.shape
    out = np.zeros(4, np.float64)
    assert lib.mh_image_metrics(h, w, xs, image.ctypes.data_as(F32P), target.ctypes.data, int(target.dtype == np.uint8),
                                out.ctypes.data_as(F64P)) == 0
    return out
