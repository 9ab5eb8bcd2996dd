"""Seeded inputs of the JPEG tests, each with the property it is there to provoke, asserted on the
float64 oracle's own statistics (``check``); and the g++ build of tests/hostmath/jpeg.cpp that the CPU and the GPU tests
compare with."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np

import jpeg_oracle as JO

ROOT = Path(__file__).resolve().parent.parent
SUBSAMPLINGS = ("420", "444")
SUB_CODE = {"444": 0, "420": 1}


def noise(width=40, height=24, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def waves(width, height, seed=1):
    """A horizontal sinusoid of period 16 that fills the range (adjacent 8x8 blocks alternate bright and dark), a ramp
    down the rows and across the columns in two channels, and noise of sigma 4."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(width)[None, :, None], np.arange(height)[:, None, None]
    s = 127.5 + 125.0 * np.sin(2 * np.pi * (x + 0.5) / 16)
    ramp = np.array([0.0, 1.0, -1.0])[None, None, :] * (8.0 * y / max(height - 1, 1) - 4.0) \
        + np.array([1.0, 0.0, 1.0])[None, None, :] * (6.0 * x / max(width - 1, 1) - 3.0)
    return np.clip(np.rint(s + ramp + rng.normal(0.0, 4.0, (height, width, 3))), 0, 255).astype(np.uint8)


def constant(width=17, height=9):
    return np.full((height, width, 3), (200, 90, 30), np.uint8)


def checkerboard(side=32):
    x, y = np.arange(side)[None, :], np.arange(side)[:, None]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


# name -> (image, quality, restart interval or None for one MCU row)
CASES = {
    "noise_q25": (noise(), 25, None),
    "noise_q90": (noise(), 90, None),
    "noise_q100": (noise(), 100, None),
    "waves_130x70": (waves(130, 70), 90, None),
    "waves_72x16_q100_r2": (waves(72, 16), 100, 2),
    "waves_72x16_r1": (waves(72, 16), 90, 1),
    "constant_17x9": (constant(), 90, None),
    "one_pixel": (np.array([[[255, 0, 128]]], np.uint8), 90, None),
    "checkerboard_q100": (checkerboard(), 100, None),
}
NOISE_BELOW_Q90 = ("noise_q25",)                # left out of the comparison of decoded pixels with libjpeg's
HALF_INTEGERS = ("checkerboard_q100",)          # left out of the comparison of coefficients with the float64 ones


def check(name, subsampling, stats, blocks):
    """The oracle's statistics of a case say that it provokes what it is there for."""
    if name.startswith("noise"):
        assert stats["stuffed"] > 0 and (subsampling == "444" or 9 <= stats["stuffed"] <= 34), stats
        if name == "noise_q25" and subsampling == "444":
            assert stats["zrl"] == 42, stats
        if name == "noise_q100" and subsampling == "420":
            assert stats["dc_cat"] == 10 and stats["ac_cat"] == 9, stats
    elif name == "waves_130x70":
        assert 130 % 16 and 70 % 16 and 130 % 8 and 70 % 8
        assert stats["segments"] == (5 if subsampling == "420" else 9) and stats["zrl"] > 0, stats
    elif name == "waves_72x16_q100_r2":
        if subsampling == "444":
            assert stats["dc_cat"] == 11, stats
    elif name == "waves_72x16_r1":
        if subsampling == "444":
            assert stats["segments"] == 18, stats          # RSTm runs 0..7 0..7 0: the index wraps twice
    elif name == "constant_17x9":
        assert stats["eob"] == blocks and stats["ac_cat"] == 0 and stats["zrl"] == 0, stats
        assert stats["zero_dc_diff"] > 0, stats
    elif name == "checkerboard_q100":
        assert stats["ac_cat"] == 10 and stats["stuffed"] == (100 if subsampling == "444" else 76), stats


# ------------------------------------------------------------------------------------------------------- the host build
I16P, U8P = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_uint8)


def build_host(directory):
    """g++ build of tests/hostmath/jpeg.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_jpeg.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "jpeg.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i = ctypes.c_int
    lib.jh_blocks.restype, lib.jh_blocks.argtypes = ctypes.c_int64, [i, i, i]
    lib.jh_header.restype, lib.jh_header.argtypes = i, [i, i, i, i, i, U8P]
    lib.jh_coefficients.restype, lib.jh_coefficients.argtypes = i, [ctypes.c_void_p, i, i, i, i, i, i, I16P]
    lib.jh_encode.restype, lib.jh_encode.argtypes = ctypes.c_int64, [I16P, i, i, i, i, i, U8P, ctypes.c_int64]
    lib.jh_worst_bytes.restype, lib.jh_worst_bytes.argtypes = ctypes.c_int64, [i, i, i, i]
    return lib


def host_coefficients(lib, img, quality, subsampling):
    """-> int16 [blocks, 64], zigzag order, blocks in scan order.  img: uint8 [H, W, 3] or float32 [H, W, 3 or 4]."""
    img = np.ascontiguousarray(img)
    h, w, stride = img.shape
    out = np.zeros((lib.jh_blocks(w, h, SUB_CODE[subsampling]), 64), np.int16)
    assert lib.jh_coefficients(img.ctypes.data, int(img.dtype == np.float32), stride, w, h, quality,
                               SUB_CODE[subsampling], out.ctypes.data_as(I16P)) == 0
    return out


def host_encode(lib, coef, width, height, quality, subsampling, restart_interval=None):
    ri = restart_interval or 0
    cap = lib.jh_worst_bytes(width, height, SUB_CODE[subsampling], ri)
    out = np.zeros(cap, np.uint8)
    n = lib.jh_encode(np.ascontiguousarray(coef).ctypes.data_as(I16P), width, height, quality, SUB_CODE[subsampling], ri,
                      out.ctypes.data_as(U8P), cap)
    assert 0 < n <= cap
    return out[:n].tobytes()


def split_components(coef, width, height, subsampling):
    """int16 [blocks, 64] in scan order -> [Y, Cb, Cr], each [rows, cols, 64] (the oracle's layout)."""
    _, mx, my = JO.geometry(width, height, subsampling)
    if subsampling == "420":
        m = coef.reshape(my, mx, 6, 64)
        y = m[:, :, :4].reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
        return [y, m[:, :, 4], m[:, :, 5]]
    m = coef.reshape(my, mx, 3, 64)
    return [m[:, :, 0], m[:, :, 1], m[:, :, 2]]
