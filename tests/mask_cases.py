"""Seeded inputs of the mask tests: shapes, masks, the float64 references (computed once and
shared), and the g++ build of tests/hostmath/mask.cpp (csrc/mask_math.h compiled for the host)."""
import ctypes
import functools
import math
import subprocess
from pathlib import Path

import numpy as np
import torch

from oracle import train_oracle as TO

ROOT = Path(__file__).resolve().parent.parent

# The smallest shapes at which the kernels' partitioning can go wrong: one map location; 65 map columns (a second column
# block of one column, and the ten extra columns); exactly 64 map columns and 65 map rows (more rows than the longest
# segment, 64, so several row segments whatever the segmentation picks); three column blocks and a width that is no
# multiple of 4; and, for the backward pass's 32-pixel tiles, 42 and 43 (one tile + 10, + 11) beside the 75s above.
SHAPES = ((11, 11), (21, 75), (75, 74), (43, 140), (42, 43))
LAMBDA, LAMBDA_DEPTH = 0.2, 0.3
SEG_MIN = 8                      # the shortest row segment of the sliding-window pass: small images are cut every 8 map rows

# the bars of the unmasked tests, unchanged (tests/test_gpu_training.py: values 2e-6, the total 3e-6, the gradient
# 2e-8 + 1e-4 max|grad|; tests/metrics_cases.py for the metrics)
BAR_VALUE, BAR_LOSS = 2e-6, 3e-6


def gradient_bar(ref_grad) -> float:
    return 2e-8 + 1e-4 * float(ref_grad.abs().max())


@functools.lru_cache(maxsize=None)
def inputs(h, w):
    """-> (frame float32 [h, w, 4]: RGB in [0, 1] and a depth in [2, 10]; target [h, w, 3]; depth target [h, w]), drawn as
    tests/test_gpu_training.py draws them."""
    g = torch.Generator().manual_seed(7 * h + w)
    frame = torch.rand(h, w, 4, generator=g)
    frame[:, :, 3] = 2.0 + 8.0 * frame[:, :, 3]
    tgt = (frame[:, :, :3] + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    dtgt = 2.0 + 8.0 * torch.rand(h, w, generator=g)
    return frame, tgt, dtgt


@functools.lru_cache(maxsize=None)
def masks(h, w):
    """name -> uint8 [h, w] tensor (host).  all255 / all0; random bytes of which a third are 255, a third 0 and a third
    soft; a single kept pixel in each corner and on the last row and the last column (the trailing ten rows and columns
    are counted by the last block only), one of them soft; a vertical edge at columns 63, 64 and 74 where the image is
    that wide (kept on the left); a horizontal edge at the first segment boundary (map row 8) and at the first of the
    ten trailing rows."""
    g = torch.Generator().manual_seed(1000 * h + w)
    out = {"all255": torch.full((h, w), 255, dtype=torch.uint8), "all0": torch.zeros((h, w), dtype=torch.uint8)}
    kind = torch.randint(0, 3, (h, w), generator=g)
    soft = torch.randint(1, 255, (h, w), generator=g).to(torch.uint8)
    out["random"] = torch.where(kind == 0, torch.full_like(soft, 255), torch.where(kind == 1, torch.zeros_like(soft), soft))
    pixels = torch.zeros((h, w), dtype=torch.uint8)
    for y, x, b in ((0, 0, 255), (0, w - 1, 255), (h - 1, 0, 255), (h - 1, w - 1, 255), (h - 1, w // 2, 200), (h // 2, w - 1, 255)):
        pixels[y, x] = b
    out["pixels"] = pixels
    for col in (63, 64, 74):
        if w > col:
            m = torch.zeros((h, w), dtype=torch.uint8)
            m[:, :col] = 255
            out[f"vedge{col}"] = m
    for name, row in (("hedge_segment", SEG_MIN), ("hedge_tail", h - 10)):
        if 0 < row < h:
            m = torch.zeros((h, w), dtype=torch.uint8)
            m[row:, :] = 255
            out[name] = m
    return out


def weights(mask) -> torch.Tensor:
    """float32 weights of a uint8 mask tensor: the correctly rounded quotients byte / 255 (numpy on the host)."""
    table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0))
    return table[mask.long()]


def is_binary(mask) -> bool:
    return bool(((mask == 0) | (mask == 255)).all())


def substituted64(x64, y64, mask):
    """The substituted image in float64: x where the byte is 255, y + m (x - y) otherwise (differentiable)."""
    m = weights(mask).double()[..., None]
    return torch.where((mask == 255)[..., None], x64, y64 + m * (x64 - y64))


@functools.lru_cache(maxsize=None)
def loss_reference(h, w, name, with_depth):
    """The float64 oracle of the masked loss on inputs(h, w) under masks(h, w)[name]: substitution in float64, then
    oracle.train_oracle.photometric_loss, the depth term mean(m |d - D|) written out, autograd for the gradients.
    -> dict(loss, l1, ssim, depth, grad_rgb [h, w, 3], grad_depth [h, w]) - shared by the three loss paths."""
    frame, tgt, dtgt = inputs(h, w)
    mask = masks(h, w)[name]
    x64 = frame[:, :, :3].double().requires_grad_(True)
    d64 = frame[:, :, 3].double().requires_grad_(True)
    ref, l1, s = TO.photometric_loss(substituted64(x64, tgt.double(), mask), tgt.double(), LAMBDA)
    depth = (weights(mask).double() * (d64 - dtgt.double())).abs().mean()
    total = ref + LAMBDA_DEPTH * depth if with_depth else ref
    total.backward()
    return dict(loss=float(total), l1=float(l1), ssim=float(s), depth=float(depth) if with_depth else 0.0,
                grad_rgb=x64.grad.clone(), grad_depth=d64.grad.clone() if with_depth else torch.zeros(h, w, dtype=torch.float64))


def ssim_map64(x64, y64):
    """The SSIM map [3, H - 10, W - 10] of two float64 [H, W, 3] images: oracle.train_oracle.ssim before its mean."""
    X, Y = x64.permute(2, 0, 1)[None], y64.permute(2, 0, 1)[None]
    win = TO.gauss_window(dtype=X.dtype)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = TO._filter(X, win), TO._filter(Y, win)
    s1 = TO._filter(X * X, win) - mu1 * mu1
    s2 = TO._filter(Y * Y, win) - mu2 * mu2
    s12 = TO._filter(X * Y, win) - mu1 * mu2
    return (((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * ((2 * s12 + c2) / (s1 + s2 + c2)))[0]


def metrics_reference(image, target, mask) -> np.ndarray:
    """Float64 restatement of the masked metrics' definitions -> {mse, l1, ssim, psnr}; NaN where
    the weights sum to zero.  image: float32 [H, W, 3]; target: float32 [H, W, 3]; mask: uint8 [H, W]."""
    x, y, m = image[:, :, :3].double(), target.double(), weights(mask).double()
    h, w = m.shape
    d = x - y
    with np.errstate(divide="ignore", invalid="ignore"):
        sm = float(m.sum())
        mse = np.float64((m[..., None] * d * d).sum()) / np.float64(3.0 * sm)
        l1 = np.float64((m[..., None] * d.abs()).sum()) / np.float64(3.0 * sm)
        mc = m[5:h - 5, 5:w - 5]
        smap = ssim_map64(substituted64(x, y, mask), y)
        ssim = np.float64((mc[None] * smap).sum()) / np.float64(3.0 * float(mc.sum()))
        psnr = np.float64(-10.0) * np.log10(mse)
    return np.array([mse, l1, ssim, psnr], dtype=np.float64)


def check_metrics(got, ref):
    """The four values against the restatement at the bars of tests/metrics_cases.py; NaN where the reference is NaN."""
    import metrics_cases as MC
    got = np.asarray(got, dtype=np.float64)
    for k, bar in ((0, MC.REL_MSE_L1 * abs(ref[0])), (1, MC.REL_MSE_L1 * abs(ref[1])), (2, MC.ABS_SSIM)):
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), (k, got, ref)
        elif k == 2:
            assert abs(got[k] - ref[k]) < bar, (k, got, ref)
        else:
            assert abs(got[k] - ref[k]) <= bar, (k, got, ref)
    if math.isnan(ref[3]):
        assert math.isnan(got[3]), (got, ref)
    elif ref[0] > 0:
        assert abs(got[3] - ref[3]) < MC.ABS_PSNR_DB, (got, ref)
    else:
        assert got[3] == math.inf


# ------------------------------------------------------------------------------------------------------- the host build
F32P, U8P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)


def build_host(directory):
    """g++ build of tests/hostmath/mask.cpp: csrc/mask_math.h compiled for the host."""
    so = Path(directory) / "_mask.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "mask.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.kh_weight.restype, lib.kh_weight.argtypes = ctypes.c_float, [ctypes.c_int]
    lib.kh_blend.restype, lib.kh_blend.argtypes = None, [ctypes.c_longlong, F32P, F32P, U8P, F32P]
    return lib


def host_blend(lib, image, target, mask) -> torch.Tensor:
    """image, target: float32 [H, W, 3] host tensors; mask: uint8 [H, W] -> the host build's substituted image."""
    x, y = np.ascontiguousarray(image.numpy(), dtype=np.float32), np.ascontiguousarray(target.numpy(), dtype=np.float32)
    m = np.ascontiguousarray(mask.numpy(), dtype=np.uint8)
    out = np.full_like(x, 7.0)
    lib.kh_blend(m.size, x.ctypes.data_as(F32P), y.ctypes.data_as(F32P), m.ctypes.data_as(U8P), out.ctypes.data_as(F32P))
    return torch.from_numpy(out)


def blend_restatement(image, target, mask) -> np.ndarray:
    """The definition restated in float64 numpy, rounded to float32: x where the byte is 255, else y + m d with d the
    FLOAT32 difference x - y, as the definition fmaf(m, x - y, y) has it (the product of two float32 values is exact in
    double, the sum is rounded to double and then to float32: at most one float32 ulp from the single rounding of the
    fused multiply-add)."""
    x, y = image.numpy().astype(np.float32), target.numpy().astype(np.float32)
    m = (np.arange(256, dtype=np.float32) / np.float32(255.0))[mask.numpy()][..., None].astype(np.float64)
    d = (x - y).astype(np.float64)
    return np.where((mask.numpy() == 255)[..., None], x.astype(np.float64), y.astype(np.float64) + m * d).astype(np.float32)
