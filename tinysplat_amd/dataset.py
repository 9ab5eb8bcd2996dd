"""COLMAP datasets: ``Dataset(colmap_path, images_path)`` of tinysplat/dataset.py:13-114.

The reference parses the sparse model with pycolmap, undistorts every image with OpenCV on the CPU and keeps float
targets.  Here ``colmap.read_reconstruction`` parses the model, the camera matrices are worked out on the host in
float64 (``camera_from_colmap``), and one HIP launch per image (csrc/undistort.hip) undistorts, recentres and
downscales it on the GPU, where the targets stay as ``uint8``.  There is no CPU path for the resampling.

Pixel conventions: a pixel INDEX counts pixel centres (the first pixel's centre is 0; OpenCV's and the kernel's
convention); COLMAP's pixel coordinates put that centre at 0.5.
"""
from __future__ import annotations

import ctypes
import math
import os
from collections.abc import Sequence
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .colmap import CAMERA_MODELS, read_reconstruction
from .init import PointCloud
from .ops import _call, _need_hip, _ptr, _stream
from .synthetic import PinholeCamera, quat_to_rot_matrix

# COLMAP model id -> (focal lengths, principal point, distortion coefficients kept): the models undistort_math.h covers
_MODELS = {0: (1, 2, 0), 1: (2, 2, 0), 2: (1, 2, 1), 3: (1, 2, 2), 4: (2, 2, 4), 6: (2, 2, 8)}
PRINCIPAL_POINT_MODES = ("reference", "center")
_GRID = 9                       # getOptimalNewCameraMatrix samples a 9 x 9 grid of source pixels
_IDENTITY_PX = 1e-6             # a map that moves no pixel further than this is the identity (see _is_identity)


class CameraSetup(NamedTuple):
    """What ``camera_from_colmap`` returns.  Intrinsics are float64 ``(fx, fy, cx, cy)`` in pixel indices."""
    src_k: np.ndarray           # of the image file
    dst_k: np.ndarray           # of the target
    dist: np.ndarray            # float64 [8]: k1 k2 p1 p2 k3 k4 k5 k6
    out_size: Tuple[int, int]   # (width, height) of the target
    resample: bool              # False: the file's pixels are the target
    camera: PinholeCamera


def distortion_coefficients(model_id: int, params) -> np.ndarray:
    """A COLMAP camera's parameters -> OpenCV's ``(k1, k2, p1, p2, k3, k4, k5, k6)``, as dataset.py:65-66 pads them."""
    if model_id not in _MODELS:
        name = CAMERA_MODELS.get(model_id, ("?",))[0]
        raise ValueError(f"camera model {name} (id {model_id}) is not supported: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, "
                         "RADIAL, OPENCV and FULL_OPENCV are")
    nf, nc, nd = _MODELS[model_id]
    d = np.zeros(8)
    d[:nd] = np.asarray(params, dtype=np.float64)[nf + nc:nf + nc + nd]
    return d


def distort_points(d, x, y):
    """undistort_math.h's forward distortion of normalised coordinates, in the dtype of the inputs."""
    r2 = x * x + y * y
    rad = (1 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))) / (1 + r2 * (d[5] + r2 * (d[6] + r2 * d[7])))
    xy2 = 2 * (x * y)
    return x * rad + d[2] * xy2 + d[3] * (r2 + 2 * x * x), y * rad + d[2] * (r2 + 2 * y * y) + d[3] * xy2


def undistort_points(d, xd, yd, max_iter: int = 200, tol: float = 1e-15):
    """The inverse of ``distort_points`` by OpenCV's fixed-point iteration (undistortPoints), float64:
    ``x <- (xd - tangential(x, y)) / rad(x, y)`` until no coordinate moves by ``tol`` or more."""
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    x, y = xd.copy(), yd.copy()
    for _ in range(max_iter):
        r2 = x * x + y * y
        inv = (1 + r2 * (d[5] + r2 * (d[6] + r2 * d[7]))) / (1 + r2 * (d[0] + r2 * (d[1] + r2 * d[4])))
        dx = 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
        dy = d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
        nx, ny = (xd - dx) * inv, (yd - dy) * inv
        step = max(float(np.max(np.abs(nx - x))), float(np.max(np.abs(ny - y))))
        x, y = nx, ny
        if step < tol:
            break
    return x, y


def inner_rectangle(src_k, d, width: int, height: int):
    """``(x0, x1, y0, y1)`` in undistorted normalised coordinates: the largest axis-parallel rectangle inside the image
    of the 9 x 9 grid of source pixels ``(i (W-1)/8, j (H-1)/8)`` (OpenCV's icvGetRectangles, the inner one)."""
    fx, fy, cx, cy = src_k
    gx, gy = np.meshgrid(np.arange(_GRID) * (width - 1) / (_GRID - 1), np.arange(_GRID) * (height - 1) / (_GRID - 1))
    xd, yd = (gx - cx) / fx, (gy - cy) / fy
    x, y = undistort_points(d, xd, yd)
    bx, by = distort_points(d, x, y)
    x0, x1, y0, y1 = float(x[:, 0].max()), float(x[:, -1].min()), float(y[0, :].max()), float(y[-1, :].min())
    # coefficients as strong as these are not a lens: the iteration wanders, and its output would pass for a matrix
    if not (max(np.abs(bx - xd).max(), np.abs(by - yd).max()) < 1e-9 and x0 < x1 and y0 < y1):
        raise ValueError("the inverse distortion does not converge on this frame: the coefficients fold it over")
    return x0, x1, y0, y1


def optimal_new_camera_matrix(src_k, d, width: int, height: int) -> np.ndarray:
    """OpenCV's ``getOptimalNewCameraMatrix(alpha=0)``: the inner rectangle stretched over the whole frame."""
    x0, x1, y0, y1 = inner_rectangle(src_k, d, width, height)
    fx, fy = (width - 1) / (x1 - x0), (height - 1) / (y1 - y0)
    return np.array([fx, fy, -fx * x0, -fy * y0])


def centered_camera_matrix(src_k, d, width: int, height: int) -> np.ndarray:
    """The principal point at the frame's centre, where the rasteriser's optical axis is, and the largest focal lengths
    at which the inner rectangle still covers the frame."""
    x0, x1, y0, y1 = inner_rectangle(src_k, d, width, height)
    ax, ay = (width - 1) / 2, (height - 1) / 2
    return np.array([ax / min(-x0, x1), ay / min(-y0, y1), ax, ay])


def _is_identity(src_k, dst_k, d, size, out_size) -> bool:
    """No distortion, equal sizes and intrinsics that agree to ``_IDENTITY_PX`` of a pixel at the frame's corners: the
    source's integer levels then come back unchanged (a shift of 1e-6 px moves a value by 3e-4 levels at most)."""
    if np.any(d != 0) or tuple(size) != tuple(out_size):
        return False
    w, h = size
    corners = np.array([[0.0, 0.0], [w - 1.0, h - 1.0]])
    moved = (corners - dst_k[2:]) / dst_k[:2] * src_k[:2] + src_k[2:] - corners
    return bool(np.max(np.abs(moved)) < _IDENTITY_PX)


def camera_from_colmap(cam, image, image_size, principal_point: str = "reference",
                       max_image_dimension: Optional[int] = None) -> CameraSetup:
    """A ``colmap.Camera`` and ``colmap.Image`` with the ``(width, height)`` of the image file -> ``CameraSetup``.

    ``principal_point="reference"`` follows dataset.py:38-79: the focal lengths are multiplied by ``size / 2 / c``,
    COLMAP's ``cx, cy`` enter the camera matrix as they are, the new matrix is OpenCV's ``getOptimalNewCameraMatrix``
    at alpha 0, and only a model with distortion parameters is undistorted.  ``"center"``: the source intrinsics are
    COLMAP's, moved to pixel indices (``c - 0.5``) and scaled to the file's size; the target's principal point is the
    frame's centre, which is where the rasteriser's optical axis is.  ``max_image_dimension`` scales the target so
    that its longer side is at most that many pixels."""
    if principal_point not in PRINCIPAL_POINT_MODES:
        raise ValueError(f"principal_point must be one of {PRINCIPAL_POINT_MODES}")
    d = distortion_coefficients(cam.model_id, cam.params)
    nf = _MODELS[cam.model_id][0]
    params = np.asarray(cam.params, dtype=np.float64)
    fx, fy = params[0], params[nf - 1]
    cx, cy = params[nf], params[nf + 1]
    width, height = int(image_size[0]), int(image_size[1])
    if width < 1 or height < 1:
        raise ValueError("image_size must be (width, height), both at least 1")
    if not (np.isfinite(params).all() and min(fx, fy, cx, cy) > 0 and cam.width >= 1 and cam.height >= 1):
        raise ValueError(f"camera {cam.camera_id}: finite parameters, positive focal lengths, principal point and size "
                         "expected")
    if principal_point == "reference":
        src_k = np.array([fx * (width / 2 / cx), fy * (height / 2 / cy), cx, cy])
        dst_k = optimal_new_camera_matrix(src_k, d, width, height) if _MODELS[cam.model_id][2] else src_k.copy()
    else:
        sx, sy = width / cam.width, height / cam.height
        src_k = np.array([fx * sx, fy * sy, cx * sx - 0.5, cy * sy - 0.5])
        dst_k = centered_camera_matrix(src_k, d, width, height)
    out_w, out_h = width, height
    if max_image_dimension is not None:
        s = min(1.0, max_image_dimension / max(width, height))
        out_w, out_h = max(1, int(width * s + 0.5)), max(1, int(height * s + 0.5))
        kx, ky = out_w / width, out_h / height
        dst_k = np.array([dst_k[0] * kx, dst_k[1] * ky, (dst_k[2] + 0.5) * kx - 0.5, (dst_k[3] + 0.5) * ky - 0.5])
    resample = not _is_identity(src_k, dst_k, d, (width, height), (out_w, out_h))

    f_x, f_y = float(dst_k[0]), float(dst_k[1])
    rot = quat_to_rot_matrix(np.asarray(image.qvec, dtype=np.float64))
    position = -rot.T @ np.asarray(image.tvec, dtype=np.float64)
    camera = PinholeCamera(None, None, f_x, f_y, out_w, out_h)
    camera.update_view_matrix(position, np.asarray(image.qvec, dtype=np.float64))
    camera.update_proj_matrix(2 * math.atan(out_w / (2 * f_x)), 2 * math.atan(out_h / (2 * f_y)), 0.001, 1000)
    camera.position = position
    camera.name = os.path.basename(image.name)
    ids = np.asarray(image.point3D_ids, dtype=np.int64)
    camera.visible_point_ids = torch.from_numpy(ids[ids != -1].copy())
    return CameraSetup(src_k, dst_k, d, (out_w, out_h), resample, camera)


def undistort_image(src_u8: Tensor, src_K, dst_K, dist, out_size, dtype=torch.uint8) -> Tensor:
    """``src_u8`` uint8 [H, W, 3] on the GPU -> the image of ``out_size = (width, height)`` seen by a pinhole camera
    with intrinsics ``dst_K`` (``fx, fy, cx, cy`` in pixel indices), resampled from the source with intrinsics ``src_K``
    and distortion ``dist`` (up to 8 coefficients, OpenCV's order); all three are rounded to float32.  ``dtype``:
    ``torch.uint8`` (the mean rounded half to even) or ``torch.float32`` (the unrounded mean / 255).  Downscaling
    averages n x n sub-samples per pixel (csrc/undistort_math.h)."""
    dev = _need_hip(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 3 or src_u8.shape[2] != 3:
        raise ValueError("a uint8 [H, W, 3] image expected")
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError("dtype must be torch.uint8 or torch.float32")
    src_u8 = src_u8.contiguous()
    h, w = int(src_u8.shape[0]), int(src_u8.shape[1])
    out_w, out_h = int(out_size[0]), int(out_size[1])
    if min(h, w, out_h, out_w) < 1 or h * w >= 1 << 31 or out_h * out_w >= 1 << 31:
        raise ValueError("image sizes must be at least 1 x 1 and below 2^31 pixels")
    coeff = [float(v) for v in dist]
    if len(coeff) > 8:
        raise ValueError("at most 8 distortion coefficients")
    k4, d8 = ctypes.c_float * 4, ctypes.c_float * 8
    src_k, dst_k = k4(*[float(v) for v in src_K]), k4(*[float(v) for v in dst_K])
    out = torch.empty((out_h, out_w, 3), dtype=dtype, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_undistort_image", lib.ts_undistort_image, _ptr(src_u8), h, w, src_k, dst_k,
              d8(*(coeff + [0.0] * (8 - len(coeff)))), out_h, out_w, int(dtype == torch.float32), _ptr(out), _stream(dev))
    return out


class Targets(Sequence):
    """The training targets: ``uint8`` [H, W, 3] on the device, a quarter of float targets' memory; ``targets[i]`` is
    the float32 image in [0, 1] (the byte / 255, what the reference's ``Camera`` keeps)."""

    def __init__(self, images_u8):
        self.images_u8 = list(images_u8)

    def __len__(self) -> int:
        return len(self.images_u8)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [t.to(torch.float32) / 255.0 for t in self.images_u8[i]]
        return self.images_u8[i].to(torch.float32) / 255.0


class Dataset:
    """tinysplat/dataset.py:13-114 on COLMAP's binary model.  ``cameras``: one ``PinholeCamera`` per image, in the order
    of images.bin; ``targets``: a ``Targets``; ``pcd``: an ``init.PointCloud`` for ``from_pcd``; ``resampled[i]``:
    whether image i went through the kernel; ``spatial_extent``: 1.1 x the largest distance of a camera centre from the
    mean centre (the reference's lines 100-102 flatten the positions first, which gives no distance; nothing reads
    it there)."""

    def __init__(self, colmap_path, images_path, max_image_dimension: Optional[int] = None, device="cuda:0",
                 principal_point: str = "reference"):
        from PIL import Image as PILImage
        dev = torch.device(device)
        rec = read_reconstruction(colmap_path)
        self.cameras, images_u8, self.resampled = [], [], []
        # each image's CameraSetup and the (width, height) of its file: what warps a source-sized mask exactly as its
        # photo was warped (masks.TrainingMasks)
        self.setups, self.source_sizes = [], []
        for img in rec.images.values():
            if img.camera_id not in rec.cameras:
                raise ValueError(f"image {img.name} names camera {img.camera_id}, which cameras.bin does not hold")
            with PILImage.open(os.path.join(images_path, img.name)) as f:
                pixels = np.array(f.convert("RGB"))            # a copy: torch wants writable memory
            setup = camera_from_colmap(rec.cameras[img.camera_id], img, (pixels.shape[1], pixels.shape[0]),
                                       principal_point, max_image_dimension)
            src = torch.from_numpy(np.ascontiguousarray(pixels)).to(dev)
            _need_hip(src)
            if setup.resample:
                src = undistort_image(src, setup.src_k, setup.dst_k, setup.dist, setup.out_size)
            setup.camera.visible_point_ids = setup.camera.visible_point_ids.to(dev)
            self.cameras.append(setup.camera)
            images_u8.append(src)
            self.resampled.append(setup.resample)
            self.setups.append(setup)
            self.source_sizes.append((int(pixels.shape[1]), int(pixels.shape[0])))
        self.targets = Targets(images_u8)

        positions = np.stack([c.position for c in self.cameras]) if self.cameras else np.zeros((0, 3))
        self.spatial_extent = float(np.max(np.linalg.norm(positions - positions.mean(axis=0), axis=1)) * 1.1) \
            if len(positions) else 0.0

        pts = list(rec.points3D.values())
        ids = np.array([p.point3D_id for p in pts], dtype=np.uint64)
        if ids.size and int(ids.max()) >= 1 << 63:
            raise ValueError("a point3D_id does not fit int64")
        self.pcd = PointCloud(
            point_ids=torch.from_numpy(ids.astype(np.int64)).to(dev),
            xyz=torch.from_numpy(np.array([p.xyz for p in pts], dtype=np.float64).reshape(-1, 3)).to(dev),
            colors=torch.from_numpy(np.array([p.rgb for p in pts], dtype=np.uint8).reshape(-1, 3)).to(dev),
            errors=torch.from_numpy(np.array([p.error for p in pts], dtype=np.float64)).to(dev))
