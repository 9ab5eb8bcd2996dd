"""Depth priors: stored dense depth maps scale-matched to the SfM points, the second half of
tinysplat/depth.py.

The reference runs a monocular network per image, caches its output as ``depths/<image name>.npy`` and reads the file
back when it exists (depth.py:16-40).  ``_estimate_sparse`` projects the camera's visible SfM points to pixels and
``_match_scale`` fits ``s, t`` so that ``s D + t`` agrees with them under an error-weighted L1; the result is the depth
target of the training step (train.py:65-69).  The networks stay out of scope; this module reads ``.npy`` maps made with
any monocular model and does the rest for all cameras in one batch on the GPU (csrc/depth_prior.hip): projection,
last-wins de-duplication, sampling, an exact minimiser in place of the reference's Nelder-Mead run, and the targets.

Deviations from the reference, both on inputs a valid reconstruction does not hold: a point with ``z <= 0`` or a
non-finite ``z`` is dropped (the reference has no such test), and so is a point whose reprojection error is not finite or
``<= 0`` (scipy's ``lil_matrix`` silently drops a stored zero, which misaligns the reference's depth and error arrays), as
is a visible id that the point cloud does not hold.  Maps are taken to be in the undistorted camera's frame, as the
reference's are; a map of another size than the camera (``max_image_dimension``) is sampled bilinearly.
"""
from __future__ import annotations

import csv
import os
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _need_hip, _ptr, _stream

SPACES = ("depth", "disparity")
COLUMNS = ("s", "t", "objective", "m", "evaluations", "status")      # a row of ts_depth_prior_fit, in its order
STATUS = ("ok", "adjacent", "equal_x", "no_points", "bracket_cap", "not_finite")       # TS_DEPTH_FIT_*
MAX_CAMERAS, MAX_VISIBLE, MAX_PIXELS = 1 << 15, 1 << 20, (1 << 28) - 1


@dataclass
class SparseDepth:
    """Per-camera lists in CSR form on the device: camera c owns ``[offsets[c], offsets[c + 1])`` of ``pixel`` (int32,
    ``py W + px``, ascending: the order of the reference's ``tocoo()``), ``z`` (float32) and ``weight`` (float64,
    ``1 / error``); ``x`` (float32): the dense map at the pixel, when maps were given."""
    offsets: Tensor
    pixel: Tensor
    z: Tensor
    weight: Tensor
    x: Optional[Tensor] = None

    def camera(self, c: int):
        a, b = int(self.offsets[c]), int(self.offsets[c + 1])
        return self.pixel[a:b], self.z[a:b], self.weight[a:b]


def _space(space: str) -> int:
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}")
    return SPACES.index(space)


def _maps_on(dense_maps, cameras, dev) -> List[Tensor]:
    if len(dense_maps) != len(cameras):
        raise ValueError(f"{len(cameras)} cameras, {len(dense_maps)} dense maps")
    maps = []
    for d in dense_maps:
        d = torch.as_tensor(d)
        if d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1 or d.numel() >= 1 << 31:
            raise ValueError(f"a dense map must be [rows, columns], got {tuple(d.shape)}")
        maps.append(d.to(device=dev, dtype=torch.float32).contiguous())
    return maps


def _sparse(cameras: Sequence, pcd, maps: Optional[List[Tensor]]) -> SparseDepth:
    dev = _need_hip(pcd.xyz, pcd.errors, pcd.point_ids)
    cameras = list(cameras)
    n_cam = len(cameras)
    if n_cam > MAX_CAMERAS:
        raise ValueError(f"at most {MAX_CAMERAS} cameras per batch")
    lists = [torch.as_tensor(c.visible_point_ids).to(device=dev, dtype=torch.int64).reshape(-1) for c in cameras]
    counts = [int(v.numel()) for v in lists]
    if counts and max(counts) > MAX_VISIBLE:
        raise ValueError(f"at most {MAX_VISIBLE} visible points per camera")
    for c in cameras:
        if not (int(c.width) >= 1 and int(c.height) >= 1 and int(c.width) * int(c.height) < MAX_PIXELS):
            raise ValueError(f"camera sizes must be at least 1 x 1 and below {MAX_PIXELS} pixels")
    offsets_host = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    n, points = int(offsets_host[-1]), int(pcd.point_ids.shape[0])
    offsets = torch.from_numpy(offsets_host).to(dev)
    empty = SparseDepth(torch.zeros(n_cam + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                        torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.float64, device=dev),
                        None if maps is None else torch.empty(0, dtype=torch.float32, device=dev))
    if n == 0:
        return empty
    ids = torch.cat(lists)
    if points:
        indices = torch.searchsorted(pcd.point_ids, ids)              # PointCloud.get_points
        found = pcd.point_ids[indices.clamp(max=points - 1)] == ids
        indices = torch.where(found, indices, torch.full_like(indices, -1))
    else:
        indices = torch.full_like(ids, -1)
    xyz = pcd.xyz.to(torch.float32).contiguous()                      # depth.py:83: xyz_world.t().float()
    errors = pcd.errors.to(torch.float64).contiguous()
    cam_f = np.zeros((n_cam, 14), dtype=np.float32)
    cam_size = np.zeros((n_cam, 2), dtype=np.int32)
    for i, c in enumerate(cameras):
        cam_f[i, :12] = torch.as_tensor(c.view_matrix).detach().cpu().to(torch.float32).numpy()[:3, :4].reshape(-1)
        cam_f[i, 12], cam_f[i, 13] = c.f_x, c.f_y
        cam_size[i] = int(c.width), int(c.height)
    cam_f, cam_size = torch.from_numpy(cam_f).to(dev), torch.from_numpy(cam_size).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    z = torch.empty(n, dtype=torch.float32, device=dev)
    w = torch.empty(n, dtype=torch.float64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_depth_prior_project", lib.ts_depth_prior_project, n_cam, n, points, _ptr(offsets), _ptr(indices.contiguous()),
              _ptr(xyz), _ptr(errors), _ptr(cam_f), _ptr(cam_size), _ptr(keys), _ptr(z), _ptr(w), _stream(dev))
        sorted_keys, order = torch.sort(keys)
        flags = torch.empty(n, dtype=torch.int64, device=dev)
        _call("ts_depth_prior_mark", lib.ts_depth_prior_mark, n, _ptr(sorted_keys), _ptr(flags), _stream(dev))
        running = torch.cumsum(flags, 0)
        # a camera's entries stay in its span of the sorted list, so the survivors before a span are those before its start
        survivors = torch.cat([running.new_zeros(1), running])[offsets]
        pixel = torch.empty(n, dtype=torch.int32, device=dev)
        z_out, w_out = torch.empty_like(z), torch.empty_like(w)
        x_out = map_ptrs = map_size = None
        if maps is not None:
            for d, c in zip(maps, cameras):
                if d.device != dev:
                    raise ValueError("the dense maps and the point cloud must live on the same device")
            x_out = torch.empty(n, dtype=torch.float32, device=dev)
            map_ptrs = torch.tensor([d.data_ptr() for d in maps], dtype=torch.int64).to(dev)
            map_size = torch.tensor([[d.shape[0], d.shape[1]] for d in maps], dtype=torch.int32).to(dev)
        _call("ts_depth_prior_gather", lib.ts_depth_prior_gather, n, _ptr(sorted_keys), _ptr(order), _ptr(flags),
              _ptr(running), _ptr(z), _ptr(w), _ptr(map_ptrs), _ptr(map_size), _ptr(cam_size), _ptr(pixel), _ptr(z_out),
              _ptr(w_out), _ptr(x_out), _stream(dev))
        m = int(survivors[-1])
    return SparseDepth(survivors, pixel[:m], z_out[:m], w_out[:m], None if x_out is None else x_out[:m])


def sparse_depth(cameras: Sequence, pcd) -> SparseDepth:
    """``DepthEstimator._estimate_sparse`` (depth.py:73-111) for all cameras at once: every camera's
    ``visible_point_ids`` looked up in ``pcd`` (an ``init.PointCloud`` on the GPU), projected in float32 with the
    reference's arithmetic, and de-duplicated per pixel as its ``lil_matrix`` does - the point latest in the camera's list
    wins.  See the module's docstring for the points dropped beyond those that land outside the image."""
    return _sparse(cameras, pcd, None)


def fit_scale(x: Tensor, z: Tensor, weight: Tensor, offsets: Tensor, space: str = "depth") -> Tensor:
    """One exact fit per span of ``offsets`` (int64 [C + 1]): minimises ``(1/m) sum w_i |y_i - s x_i - t|`` with
    ``y = z`` (``space="depth"``) or ``y = 1 / z`` (``"disparity"``) over ``x``, ``z`` (float32) and ``weight``
    (float64) -> float64 [C, 6] on the device, a row of ``COLUMNS`` per span; ``STATUS[int(row[5])]`` names how the
    search ended.  One launch, one workgroup per span."""
    dev = _need_hip(x, z, weight, offsets)
    if x.dtype != torch.float32 or z.dtype != torch.float32 or weight.dtype != torch.float64 or offsets.dtype != torch.int64:
        raise ValueError("x and z must be float32, weight float64 and offsets int64")
    x, z, weight, offsets = x.contiguous(), z.contiguous(), weight.contiguous(), offsets.contiguous()
    spans = int(offsets.numel()) - 1
    bounds = offsets.cpu()
    if spans < 0 or x.dim() != 1 or x.shape != z.shape or x.shape != weight.shape or int(bounds[0]) != 0 or \
            int(bounds[-1]) != x.numel() or bool((bounds[1:] < bounds[:-1]).any()):
        raise ValueError("offsets must ascend from 0 to the common length of x, z and weight")
    fits = torch.empty((spans, len(COLUMNS)), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _call("ts_depth_prior_fit", _lib.load().ts_depth_prior_fit, spans, _ptr(offsets), _ptr(x), _ptr(z), _ptr(weight),
              _space(space), _ptr(fits), _stream(dev))
    return fits


def apply_scale(dense_map: Tensor, fit: Tensor, height: int, width: int, space: str = "depth") -> Tensor:
    """The float32 [height, width] target of one camera: ``float32(float64(s) D + t)`` (train.py:66: numpy float64
    scalars times the map, then ``.float()``), or its reciprocal in disparity space, ``D`` being ``dense_map`` sampled at
    the camera's pixels; ``fit``: a row of ``fit_scale``'s table on the device - it is read there, without a
    synchronisation."""
    dev = _need_hip(dense_map, fit)
    if dense_map.dtype != torch.float32 or dense_map.dim() != 2 or not dense_map.is_contiguous():
        raise ValueError("dense_map must be a contiguous float32 [rows, columns] tensor")
    if fit.dtype != torch.float64 or fit.numel() < 2 or not fit.is_contiguous():
        raise ValueError("fit must be a contiguous float64 row {s, t, ...}")
    if not (height >= 1 and width >= 1 and height * width < MAX_PIXELS):
        raise ValueError(f"the target must be at least 1 x 1 and below {MAX_PIXELS} pixels")
    out = torch.empty((int(height), int(width)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_depth_prior_apply", _lib.load().ts_depth_prior_apply, _ptr(dense_map), int(dense_map.shape[0]),
              int(dense_map.shape[1]), int(height), int(width), _ptr(fit), _space(space), _ptr(out), _stream(dev))
    return out


def match_scale(dense_maps: Sequence, cameras: Sequence, pcd, space: str = "depth"):
    """``_match_scale`` (``space="depth"``) or ``_match_scale_disparity`` (``"disparity"``, whose call site in the
    reference is dead code) for all cameras at once -> ``(fits, targets)``: a float64 [C, 6] numpy table, a row of
    ``COLUMNS`` per camera, and the float32 [H, W] device targets ``s D + t`` (``1 / (s D + t)`` in disparity space).
    ``dense_maps[i]``: camera i's [rows, columns] map, of any size.  A camera without a fit (status ``no_points`` or
    ``not_finite``) gets a target of NaNs: ``DepthPriors`` is the policy on top."""
    _space(space)
    cameras = list(cameras)
    dev = _need_hip(pcd.xyz)
    maps = _maps_on(dense_maps, cameras, dev)
    sparse = _sparse(cameras, pcd, maps)
    fits = fit_scale(sparse.x, sparse.z, sparse.weight, sparse.offsets, space)
    targets = [apply_scale(d, fits[i], int(c.height), int(c.width), space) for i, (d, c) in enumerate(zip(maps, cameras))]
    return fits.cpu().numpy(), targets


class DepthPriors:
    """The depth targets of a dataset: reads ``<depths_path>/<camera.name>.npy`` (the reference's naming, depth.py:40)
    for every camera of ``dataset_or_cameras`` (a ``Dataset`` or a sequence of cameras), scale-matches the maps to
    ``pcd`` in one batch and keeps ``targets``, a list aligned with the cameras for ``fit(..., depth_targets=)``, and
    ``fits``, the float64 [C, 6] table (``COLUMNS``; NaN rows for cameras without a file).  A camera with no file, fewer
    than ``min_points`` surviving points or a fitted ``s <= 0`` gets ``None`` - ``fit`` reads that as "no depth term this
    step" - and one warning line.  A float32 target is 4 bytes per pixel beside the 3 of the ``uint8`` image."""

    def __init__(self, dataset_or_cameras, pcd, depths_path, space: str = "depth", min_points: int = 2):
        _space(space)
        self.cameras = list(getattr(dataset_or_cameras, "cameras", dataset_or_cameras))
        self.space, self.min_points = space, int(min_points)
        self.names = [str(getattr(c, "name", i)) for i, c in enumerate(self.cameras)]
        self.fits = np.full((len(self.cameras), len(COLUMNS)), np.nan)
        self.targets: List[Optional[Tensor]] = [None] * len(self.cameras)
        self.reasons: List[Optional[str]] = [None] * len(self.cameras)
        have, maps = [], []
        for i, name in enumerate(self.names):
            path = os.path.join(str(depths_path), name + ".npy")
            if not os.path.exists(path):
                self.reasons[i] = f"no file {path}"
                continue
            d = np.load(path, allow_pickle=False)
            have.append(i)
            maps.append(torch.from_numpy(np.ascontiguousarray(np.squeeze(d), dtype=np.float32)))
        if have:
            fits, targets = match_scale(maps, [self.cameras[i] for i in have], pcd, space)
            for row, target, i in zip(fits, targets, have):
                self.fits[i] = row
                if row[3] < self.min_points:
                    self.reasons[i] = f"{int(row[3])} SfM points survive, fewer than {self.min_points}"
                elif not (np.isfinite(row[0]) and np.isfinite(row[1])):
                    self.reasons[i] = f"no finite fit ({STATUS[int(row[5])]})"
                elif row[0] <= 0:
                    self.reasons[i] = f"the fitted scale {row[0]:.6g} is not positive"
                else:
                    self.targets[i] = target
        for name, reason in zip(self.names, self.reasons):
            if reason is not None:
                warnings.warn(f"depth prior: camera {name} trains without a depth term: {reason}", stacklevel=2)

    def __len__(self) -> int:
        return len(self.targets)

    def write_csv(self, path) -> None:
        """One line per camera: its name, the fit's row (doubles by ``repr``, which round-trips) and whether it is used."""
        with open(path, "w", newline="") as f:
            writer = csv.writer(f)
            writer.writerow(["name", *COLUMNS, "used"])
            for name, row, target in zip(self.names, self.fits, self.targets):
                status = "" if np.isnan(row[5]) else STATUS[int(row[5])]
                writer.writerow([name, repr(float(row[0])), repr(float(row[1])), repr(float(row[2])),
                                 "" if np.isnan(row[3]) else int(row[3]), "" if np.isnan(row[4]) else int(row[4]), status,
                                 int(target is not None)])
