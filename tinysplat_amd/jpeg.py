"""Baseline JPEG of an image that lives on the GPU (csrc/jpeg.hip).

The reference hands every viewer frame to cv2's encoder on the host (tinysplat/viewer.py:44-56).  Here the frame is
encoded where the compositing kernel left it and only the compressed bytes cross to the host: the file's size goes to a
device word that is mirrored to pinned memory, and exactly that many bytes follow.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _ptr, _stream

SUBSAMPLINGS = {"444": 0, "420": 1}          # ts_jpeg_*: subsampling
_U8, _F32 = 0, 1                              # ts_jpeg_encode: dtype


def _subsampling(name: str) -> int:
    if name not in SUBSAMPLINGS:
        raise ValueError(f"subsampling {name!r}: '420' or '444'")
    return SUBSAMPLINGS[name]


def jpeg_header(width: int, height: int, quality: int = 90, subsampling: str = "420",
                restart_interval: Optional[int] = None) -> bytes:
    """The file's bytes up to the entropy-coded data (no GPU is touched)."""
    buf = np.zeros(1024, np.uint8)
    n = _lib.load().ts_jpeg_header(width, height, quality, _subsampling(subsampling), restart_interval or 0,
                                   buf.ctypes.data, buf.size)
    if n < 0:
        _lib.check(int(n), "ts_jpeg_header")
    return buf[:n].tobytes()


def _as_image(image, device) -> Tensor:
    """-> a tensor the kernels read in place: uint8 [H, W, 3] contiguous, or float32 [H, W, 3] whose pixels lie 3 or 4
    floats apart (the one-node frame's RGB + depth tensor, sliced); anything else is made contiguous first."""
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image)).to(device)
    if not image.is_cuda:
        raise RuntimeError("encode_jpeg: the image must be on the GPU (tinysplat_amd has no CPU fallback)")
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype not in (torch.uint8, torch.float32):
        raise ValueError("encode_jpeg: uint8 or float32 [H, W, 3]")
    h, w, _ = image.shape
    if image.dtype == torch.float32 and image.stride(2) == 1 and image.stride(1) in (3, 4) \
            and image.stride(0) == w * image.stride(1):
        return image
    return image.contiguous()


class JpegEncoder:
    """Encoder of ``width`` x ``height`` frames: keeps the kernels' workspace, the device buffer of the file's worst case
    and a pinned (size word, bytes) pair, so a frame costs the launches, a 4-byte copy and a copy of the file itself."""

    def __init__(self, width: int, height: int, quality: int = 90, subsampling: str = "420",
                 restart_interval: Optional[int] = None, device="cuda:0"):
        self.width, self.height, self.quality = int(width), int(height), int(quality)
        self.subsampling, self.restart_interval = subsampling, int(restart_interval or 0)
        self.device = torch.device(device)
        if not 1 <= self.quality <= 100:
            raise ValueError("quality: 1..100")
        lib = _lib.load()
        code = _subsampling(subsampling)
        ws = int(lib.ts_jpeg_ws_bytes(self.width, self.height, code, self.restart_interval))
        self.capacity = int(lib.ts_jpeg_max_bytes(self.width, self.height, code, self.restart_interval))
        if ws < 0 or self.capacity < 0:
            raise ValueError(f"JpegEncoder: {width} x {height}, restart interval {restart_interval}: out of range")
        self._ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self._out = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self._size = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._size_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._bytes_host = torch.empty(max(4096, self.width * self.height // 2), dtype=torch.uint8).pin_memory()
        self.blocks = (self._mcus() * (6 if code else 3))

    def _mcus(self) -> int:
        m = 16 if self.subsampling == "420" else 8
        return -(-self.width // m) * -(-self.height // m)

    def launch(self, image, quality: Optional[int] = None, coefficients: Optional[Tensor] = None,
               out_capacity: Optional[int] = None) -> None:
        """Issues the encode of ``image`` on the current stream (no synchronisation)."""
        img = _as_image(image, self.device)
        if tuple(img.shape[:2]) != (self.height, self.width):
            raise ValueError(f"JpegEncoder: image {tuple(img.shape)} is not {self.height} x {self.width}")
        lib = _lib.load()
        self._image = img                       # stays alive until the launches that read it have been waited for
        _call("ts_jpeg_encode", lib.ts_jpeg_encode, _ptr(img), _F32 if img.dtype == torch.float32 else _U8,
              int(img.stride(1)), self.width, self.height, int(self.quality if quality is None else quality),
              SUBSAMPLINGS[self.subsampling], self.restart_interval, _ptr(self._ws), _ptr(self._out),
              self.capacity if out_capacity is None else int(out_capacity), _ptr(self._size), _ptr(coefficients),
              _stream(self.device))

    def collect(self) -> bytes:
        """Waits for the launched encode and brings the file to the host: the size word, then that many bytes."""
        stream = torch.cuda.current_stream(self.device)
        self._size_host.copy_(self._size, non_blocking=True)
        stream.synchronize()
        n = int(self._size_host[0])
        if not 0 < n <= self.capacity:
            raise RuntimeError(f"JpegEncoder: size word {n} outside the buffer of {self.capacity} bytes")
        if n > self._bytes_host.numel():
            self._bytes_host = torch.empty(2 * n, dtype=torch.uint8).pin_memory()
        self._bytes_host[:n].copy_(self._out[:n], non_blocking=True)
        stream.synchronize()
        self._image = None
        return self._bytes_host[:n].numpy().tobytes()

    def encode(self, image, quality: Optional[int] = None) -> bytes:
        self.launch(image, quality)
        return self.collect()


def encode_jpeg(image, quality: int = 90, subsampling: str = "420", restart_interval: Optional[int] = None) -> bytes:
    """``image`` (uint8 or float32 [H, W, 3] on the GPU; float samples are scaled by 255 and rounded) -> a baseline JPEG
    file.  ``restart_interval`` in MCUs; the default is one MCU row."""
    img = _as_image(image, torch.device("cuda:0") if isinstance(image, np.ndarray) else None)
    return JpegEncoder(img.shape[1], img.shape[0], quality, subsampling, restart_interval, img.device).encode(img)


def jpeg_coefficients(image, quality: int = 90, subsampling: str = "420") -> List[Tensor]:
    """The quantised coefficients the encoder codes: [Y, Cb, Cr], each int16 [block rows, block columns, 64] in zigzag
    order (for tests; the encoder writes them out only when asked)."""
    img = _as_image(image, torch.device("cuda:0") if isinstance(image, np.ndarray) else None)
    enc = JpegEncoder(img.shape[1], img.shape[0], quality, subsampling, None, img.device)
    coef = torch.empty((enc.blocks, 64), dtype=torch.int16, device=img.device)
    enc.launch(img, coefficients=coef)
    torch.cuda.current_stream(img.device).synchronize()
    return split_components(coef, img.shape[1], img.shape[0], subsampling)


def split_components(coef: Tensor, width: int, height: int, subsampling: str) -> List[Tensor]:
    """int16 [blocks, 64] in scan order -> [Y, Cb, Cr], each [block rows, block columns, 64]."""
    m = 16 if subsampling == "420" else 8
    mx, my = -(-width // m), -(-height // m)
    if subsampling == "420":
        c = coef.reshape(my, mx, 6, 64)
        y = c[:, :, :4].reshape(my, mx, 2, 2, 64).permute(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
        return [y.contiguous(), c[:, :, 4].contiguous(), c[:, :, 5].contiguous()]
    c = coef.reshape(my, mx, 3, 64)
    return [c[:, :, k].contiguous() for k in range(3)]
