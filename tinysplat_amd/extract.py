"""SuGaR level-set surface points from depth renders: the tensor half of ``GaussianModel.extract_mesh_poisson``
(tinysplat/splatting/model_gaussian.py:401-460), DESIGN.md section 6f.

Per camera: render the depth plane, back-project random pixels (scene.py:165-192), find each point's nearest Gaussian,
march 21 samples over +-3 sigma along the pixel's ray, evaluate the 16-neighbour density of §6e at every sample, and
interpolate the first crossing of the level 0.3.  The result is an oriented point cloud (the normals are an addition:
``-grad d / |grad d|`` at each point), the input every Poisson tool takes; ``formats.export_points_ply`` writes it.
Poisson reconstruction, decimation and the outlier filter are not part of this package.

The hot path is csrc/extract.hip on top of ``ts_knn``; there is no CPU fallback: tensors must be on the GPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._field import EXTRACT_K, PackedModel, Workspace, cat, knn, largest, normals_at, pack_model
from .ops import _call, _f32c, _need_hip, _ptr, _stream

MAX_STEPS = 64                  # TS_EXTRACT_MAX_STEPS
_CONVENTIONS = {"reference": 0, "screen": 1}


@dataclass
class ExtractConfig:
    """The literals of model_gaussian.py:402-403, :429: ``surface_level`` 0.3, ``num_total_points`` 2_000_000 (split
    ``// len(cameras)``), ``num_steps`` 21 samples over ``extent_sigmas`` = +-3 ``|exp(scales)|`` of the nearest
    Gaussian.  ``pixel_convention``: ``"reference"`` pairs pixel and depth as the reference does (x = f % H, y = f // H
    with the depth of row f // W, column f % W; x divided by the height, y by the width, integer image centres:
    right only for square images of even size) or ``"screen"`` (column f % W, row f // W, the inverse of where the
    rasterizer puts a Gaussian's centre).  ``normals``: also compute ``-grad d / |grad d|``.  ``max_workspace_bytes``
    bounds every transient buffer of the march (samples, neighbour lists, the k-NN workspace); the packed records
    (44 B per Gaussian) and the returned tensors come on top."""
    surface_level: float = 0.3
    num_total_points: int = 2_000_000
    num_steps: int = 21
    extent_sigmas: float = 3.0
    pixel_convention: str = "reference"
    normals: bool = True
    max_workspace_bytes: int = 256 << 20

    def __post_init__(self):
        if self.pixel_convention not in _CONVENTIONS:
            raise ValueError(f"pixel_convention must be one of {sorted(_CONVENTIONS)}")
        if not 2 <= int(self.num_steps) <= MAX_STEPS:
            raise ValueError(f"num_steps must be in 2..{MAX_STEPS}")
        if not self.extent_sigmas > 0:
            raise ValueError("extent_sigmas must be positive")
        if int(self.num_total_points) < 1 or int(self.max_workspace_bytes) < 1:
            raise ValueError("num_total_points and max_workspace_bytes must be positive")


@dataclass
class SurfacePoints:
    """``points`` float32 [P,3] (model_gaussian.py:459), ``normals`` float32 [P,3] unit or zero (None without),
    ``camera`` int32 [P] (index into the cameras), ``pixel`` int64 [P] (the flat pixel index of the ray: the
    reference's ``idxs`` entry), ``t`` float32 [P] (``t_intersect`` along the ray, world units).  Cameras in order,
    rays in the order of their pixel indices."""
    points: Tensor
    normals: Optional[Tensor]
    camera: Tensor
    pixel: Tensor
    t: Tensor


def camera_position(camera) -> np.ndarray:
    """``camera.position`` when the camera carries one (the reference's ``Camera`` does), else ``-R^T t`` of its view
    matrix in double."""
    pos = getattr(camera, "position", None)
    if pos is not None:
        return np.asarray(torch.as_tensor(pos).detach().cpu().numpy(), dtype=np.float64).reshape(3)
    v = camera.view_matrix.detach().cpu().double().numpy()
    return -(v[:3, :3].T @ v[:3, 3])


def pixel_ndc(pixel_ids: Tensor, height: int, width: int, convention: str = "reference"):
    """The NDC x, y (float64) that ``ts_extract_rays`` pairs with the depth ``depth.reshape(-1)[f]`` of a flat pixel
    index ``f`` (the kernel evaluates the same expressions in float32).  ``"reference"``: x = f % H, y = f // H,
    ``(x + 0.5 - W // 2) / H * 2`` and ``(y + 0.5 - H // 2) / W * 2`` (model_gaussian.py:417-419, scene.py:183-186 as
    they stand).  ``"screen"``: column f % W, row f // W, ``(col + 0.5 - W / 2) * 2 / W`` and likewise with H."""
    if convention not in _CONVENTIONS:
        raise ValueError(f"convention must be one of {sorted(_CONVENTIONS)}")
    f = torch.as_tensor(pixel_ids).long()
    h, w = int(height), int(width)
    if convention == "reference":
        return ((f % h).double() + 0.5 - w // 2) / h * 2, ((f // h).double() + 0.5 - h // 2) / w * 2
    return ((f % w).double() + 0.5 - w / 2) * 2 / w, ((f // w).double() + 0.5 - h / 2) * 2 / h


def _camera_host(camera):
    """{inverse(P V), position, P22, P23} as 21 floats.  The inverse is taken in double of the float32 matrices'
    double product and rounded once; the reference inverts the float32 product in float32 (scene.py:170)."""
    v = camera.view_matrix.detach().cpu().double().numpy()
    p = camera.proj_matrix.detach().cpu().double().numpy()
    inv = np.linalg.inv(p @ v)
    vals = [*inv.reshape(-1).tolist(), *camera_position(camera).tolist(), float(p[2, 2]), float(p[2, 3])]
    return (ctypes.c_float * 21)(*vals)


def _chunk_rays(lib, n: int, m: int, steps: int, cap: int) -> int:
    """The largest number of rays (at most ``m``) whose chunk fits ``cap`` bytes."""
    rays = largest(lambda r: int(lib.ts_extract_chunk_bytes(n, r, steps)) <= cap, min(m, (2 ** 31 - 2) // steps))
    if rays < 1:
        need = int(lib.ts_extract_chunk_bytes(n, 1, steps))
        raise ValueError(f"max_workspace_bytes = {cap} is below the {need} bytes one ray over {n} Gaussians needs")
    return rays


class _Chunk:
    """The buffers of one chunk of rays, carved in the order of ``ts_extract_chunk_bytes``."""

    def __init__(self, lib, n: int, rays: int, steps: int, dev):
        ws = Workspace(int(lib.ts_extract_chunk_bytes(n, rays, steps)), dev)
        e = rays * steps
        f32, i32 = torch.float32, torch.int32
        self.knn_ws = ws.take(torch.uint8, int(lib.ts_knn_ws_bytes(n, e, EXTRACT_K)))
        self.p_world, self.dirs, self.points = (ws.take(f32, rays, 3) for _ in range(3))
        self.valid, self.keep, self.first, self.nearest = (ws.take(i32, rays) for _ in range(4))
        self.p_std, self.t, self.nearest_dist = (ws.take(f32, rays) for _ in range(3))
        self.samples = ws.take(f32, e, 3)
        self.knn_dist = ws.take(f32, e, EXTRACT_K)
        self.knn_idx = ws.take(i32, e, EXTRACT_K)
        ws.done()


@torch.no_grad()
def level_set_points(model, camera, depth: Tensor, pixel_ids: Tensor, config: Optional[ExtractConfig] = None,
                     return_debug: bool = False, camera_index: int = 0, packed: Optional[PackedModel] = None):
    """The per-camera core (model_gaussian.py:416-459) on a given depth map [H,W] and given flat pixel indices
    (int [M], each in [0, H*W)) -> ``SurfacePoints``, rays in ``pixel_ids`` order.

    A pixel with depth <= 0 or a non-finite back-projection yields no point (in the reference it turns into NaN and
    falls out at the crossing test); its debug ``p_world`` is the first mean, its direction zero.  ``inverse(P V)``
    is taken on the host in double; the reference inverts in float32.  The rays are processed in chunks sized so that every transient buffer stays under
    ``config.max_workspace_bytes``; the result does not depend on the chunk size.  ``return_debug``: also a dict of
    ``samples`` float32 [M,S,3], ``knn`` int32 [M,S,16], ``density`` float32 [M,S], ``p_world`` / ``dirs`` [M,3],
    ``p_std`` [M], ``nearest`` int32 [M], ``valid`` / ``keep`` bool [M], ``first`` int32 [M] and ``chunks`` (how many
    the run took).  ``packed``: a ``pack_model`` result to reuse across cameras."""
    cfg = config if config is not None else ExtractConfig()
    pk = packed if packed is not None else pack_model(model)
    depth = _f32c(depth.detach())
    dev = _need_hip(pk.means, depth)
    if depth.dim() != 2:
        raise ValueError("depth must be [H, W]")
    h, w = depth.shape
    if (h, w) != (int(camera.height), int(camera.width)):
        raise ValueError(f"depth is {h}x{w}, the camera {camera.height}x{camera.width}")
    ids = torch.as_tensor(pixel_ids).to(device=dev, dtype=torch.int64).contiguous()
    if ids.dim() != 1:
        raise ValueError("pixel_ids must be [M]")
    m, n, steps = ids.shape[0], pk.means.shape[0], int(cfg.num_steps)
    f32 = dict(dtype=torch.float32, device=dev)
    if m and bool(((ids < 0) | (ids >= h * w)).any()):
        raise ValueError(f"pixel_ids must lie in [0, {h * w})")
    lib = _lib.load()
    out_pts, out_nrm, out_pix, out_t = [], [], [], []
    dbg = {k: [] for k in ("samples", "knn", "density", "p_world", "dirs", "p_std", "nearest", "valid", "keep",
                           "first")} if return_debug else None
    chunks = 0
    if m:
        rays = _chunk_rays(lib, n, m, steps, int(cfg.max_workspace_bytes))
        ck = _Chunk(lib, n, rays, steps, dev)
        cam_host = _camera_host(camera)
        conv = _CONVENTIONS[cfg.pixel_convention]
        with torch.cuda.device(dev):
            s = _stream(dev)
            for r0 in range(0, m, rays):
                r = min(rays, m - r0)
                chunks += 1
                cid = ids[r0:r0 + r]
                _call("ts_extract_rays", lib.ts_extract_rays, r, _ptr(cid), h, w, _ptr(depth), conv, cam_host,
                      _ptr(pk.means), _ptr(ck.p_world), _ptr(ck.dirs), _ptr(ck.valid), s)
                knn(lib, pk, ck.p_world, r, 1, ck.nearest_dist, ck.nearest, ck.knn_ws, None, s)
                _call("ts_extract_samples", lib.ts_extract_samples, n, r, steps, float(cfg.extent_sigmas),
                      _ptr(ck.p_world), _ptr(ck.dirs), _ptr(ck.nearest), _ptr(pk.p_std), _ptr(ck.p_std),
                      _ptr(ck.samples), s)
                knn(lib, pk, ck.samples, r * steps, EXTRACT_K, ck.knn_dist, ck.knn_idx, ck.knn_ws, None, s)
                dens = torch.empty((r, steps), **f32) if return_debug else None
                _call("ts_extract_march", lib.ts_extract_march, n, r, steps, float(cfg.extent_sigmas),
                      float(cfg.surface_level), _ptr(ck.samples), _ptr(ck.knn_idx), _ptr(pk.records), _ptr(ck.p_world),
                      _ptr(ck.dirs), _ptr(ck.p_std), _ptr(ck.valid), _ptr(ck.keep), _ptr(ck.first), _ptr(ck.t),
                      _ptr(ck.points), _ptr(dens), s)
                if return_debug:
                    e = r * steps
                    dbg["samples"].append(ck.samples[:e].view(r, steps, 3).clone())
                    dbg["knn"].append(ck.knn_idx[:e].view(r, steps, EXTRACT_K).clone())
                    dbg["density"].append(dens)
                    for k in ("p_world", "dirs", "p_std", "nearest", "valid", "keep", "first"):
                        dbg[k].append(getattr(ck, k)[:r].clone())
                # survivors in ray order: the indices of the set flags, ascending
                sel = torch.nonzero(ck.keep[:r]).view(-1)
                p = int(sel.shape[0])
                if p == 0:
                    continue
                pts = ck.points[:r].index_select(0, sel)
                out_pts.append(pts)
                out_t.append(ck.t[:r].index_select(0, sel))
                out_pix.append(cid.index_select(0, sel))
                if cfg.normals:
                    nrm = torch.empty((p, 3), **f32)
                    normals_at(lib, pk, pts, p, nrm, ck.knn_dist, ck.knn_idx, ck.knn_ws, s)
                    out_nrm.append(nrm)
    points = cat(out_pts, (0, 3), torch.float32, dev)
    res = SurfacePoints(points, cat(out_nrm, (0, 3), torch.float32, dev) if cfg.normals else None,
                        torch.full((points.shape[0],), int(camera_index), dtype=torch.int32, device=dev),
                        cat(out_pix, (0,), torch.int64, dev), cat(out_t, (0,), torch.float32, dev))
    if not return_debug:
        return res
    shapes = {"samples": ((0, steps, 3), torch.float32), "knn": ((0, steps, EXTRACT_K), torch.int32),
              "density": ((0, steps), torch.float32), "p_world": ((0, 3), torch.float32),
              "dirs": ((0, 3), torch.float32), "p_std": ((0,), torch.float32), "nearest": ((0,), torch.int32),
              "valid": ((0,), torch.int32), "keep": ((0,), torch.int32), "first": ((0,), torch.int32)}
    debug = {k: cat(v, *shapes[k], dev) for k, v in dbg.items()}
    debug["valid"], debug["keep"] = debug["valid"].bool(), debug["keep"].bool()
    debug["chunks"] = chunks
    return res, debug


@torch.no_grad()
def extract_surface_points(model, cameras: Sequence, config: Optional[ExtractConfig] = None, device="cuda:0",
                           generator: Optional[torch.Generator] = None) -> SurfacePoints:
    """model_gaussian.py:401-460 over all ``cameras``: per camera, render the depth plane through the forward-only
    frame with a zero background, draw ``num_total_points // len(cameras)`` pixels with
    ``torch.randperm(H * W, generator=generator)`` on the CPU (the same seed gives the reference's pixels), run
    ``level_set_points`` and concatenate in camera order.

    The reference sets ``model.background = 0`` and leaves it; here the model's background is restored afterwards.
    ``model`` must live on ``device``."""
    from .rasterizer import GaussianRasterizer
    cfg = config if config is not None else ExtractConfig()
    cameras = list(cameras)
    if not cameras:
        raise ValueError("extract_surface_points needs at least one camera")
    dev = torch.device(device)
    per_camera = int(cfg.num_total_points) // len(cameras)
    pk = pack_model(model)
    if pk.means.device != dev:
        raise ValueError(f"the model lives on {pk.means.device}, not on {dev}")
    background = model.background
    model.background = torch.zeros(3, device=dev)
    parts = []
    try:
        render = GaussianRasterizer(model, cameras, device=dev)
        for ci, cam in enumerate(cameras):
            _, extras = render(cam)
            depth = extras["depth"]
            ids = torch.randperm(depth.numel(), generator=generator)[:per_camera]
            parts.append(level_set_points(model, cam, depth, ids, cfg, camera_index=ci, packed=pk))
    finally:
        model.background = background
    return SurfacePoints(torch.cat([p.points for p in parts]),
                         torch.cat([p.normals for p in parts]) if cfg.normals else None,
                         torch.cat([p.camera for p in parts]), torch.cat([p.pixel for p in parts]),
                         torch.cat([p.t for p in parts]))
