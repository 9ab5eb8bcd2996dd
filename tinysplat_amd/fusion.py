"""Truncated signed distance fusion of depth maps: ``cameras + depth maps -> mesh``, DESIGN.md section 6p.

The second mesh extractor, for the scenes whose density is no surface (a plain ``fit``, a loaded ``.ply`` or ``.splat``:
anything not trained through the density regulariser's window) but which render good depth.  Every corner of the mesher's
brick grid (``_bricks.BrickGrid``, csrc/mesh_cells.h) is projected into every camera as ``project_gaussians`` places a
Gaussian's centre, reads the depth ``d`` of the pixel it rounds to and, unless it lies more than ``trunc`` behind it,
observes ``min(1, (d - z) / trunc)``; the field is minus the mean observation (positive inside), NaN where fewer than
``min_observations`` cameras observed the corner, and the mesh is its zero set by the marching tetrahedra of section 6g,
with one added rule: a cell with a NaN corner emits nothing.

Only the bricks near a depth sample are evaluated.  **The sparsity condition**: a cell emits only if one of its corners
has a positive field value, which takes a negative observation, ``-trunc <= d - z < 0`` at the pixel the corner rounds to:
the corner lies in that pixel's frustum piece between the depths ``d`` and ``d + trunc``, and the cell in that piece's box
widened by one cell edge.  ``ts_tsdf_mark`` flags the bricks such a box touches; ``sparse=False`` evaluates every brick
and gives the same mesh bit for bit.

The grid, the list of active bricks, the march over chunks of them, the weld and the simplify and clean tail are
``_bricks.py``'s, the code ``mesh.extract_mesh`` runs; what is here is how the depth maps flag bricks and fill a chunk's
field.

The hot path is csrc/tsdf.hip and the observed variant of csrc/mesh.hip's cell kernel; there is no CPU fallback: tensors
must be on the GPU.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._bricks import BRICK_CORNERS, BrickGrid, _check_bounds, check_config, march, mesh_tail, weld
from ._field import Workspace, cat
from .mesh import TriangleMesh
from .ops import _call, _f32c, _need_hip, _ptr, _stream

_MAX_BRICKS = (2 ** 31 - 1) // BRICK_CORNERS
_MAX_CAMERAS = 65535
# the marking's containment argument (section 6p) leaves h / 16 for the float32 rounding of a pair's own arithmetic:
# enough while a camera sees the grid's coordinates below this many cell edges
_MAX_COORD_CELLS = 2.0 ** 16


@dataclass
class FusionConfig:
    """``resolution``: cells along the longest axis of the bounds; ``bounds``: ``(lo, hi)``, or None for the box of all
    back-projected valid pixels, widened by the truncation distance; ``trunc_voxels``: the truncation distance in cell
    edges (``trunc = trunc_voxels * h``); ``znear``: a corner at or nearer than this to a camera's plane is not seen by it
    (the rasteriser's 0.001); ``depth_max``: a depth beyond it counts as no depth; ``min_alpha``: ``render_depth_alpha``'s
    pixels below this opacity carry no depth (``extract_mesh_tsdf`` only); ``min_observations``: a corner that fewer
    cameras observed is unknown, and no cell with such a corner emits; ``sparse=False`` evaluates every brick (a test and
    timing yardstick); ``max_workspace_bytes`` bounds the brick flags and the transient buffers of a chunk of bricks (the
    emitted triangles and the returned tensors come on top); ``camera_batch``: cameras per ``ts_tsdf_integrate`` launch
    (None: all; the result does not depend on it); ``target_faces`` and ``clean`` as ``MeshConfig``'s."""
    resolution: int = 256
    bounds: Optional[Tuple[Sequence[float], Sequence[float]]] = None
    trunc_voxels: float = 4.0
    znear: float = 0.001
    depth_max: float = math.inf
    min_alpha: float = 0.5
    min_observations: int = 1
    sparse: bool = True
    max_workspace_bytes: int = 256 << 20
    camera_batch: Optional[int] = None
    target_faces: Optional[int] = None
    clean: Optional["CleanConfig"] = None

    def __post_init__(self):
        check_config(self)
        tv = self.trunc_voxels
        if not (isinstance(tv, (int, float)) and math.isfinite(tv) and tv > 0):
            raise ValueError("trunc_voxels must be positive and finite")
        if self.bounds is None and not 2.0 * float(tv) < int(self.resolution):
            raise ValueError("without bounds the grid is the depth samples' box widened by trunc_voxels cells on each side: "
                             "resolution must exceed 2 trunc_voxels")
        if not math.isfinite(float(self.znear)):
            raise ValueError("znear must be finite")
        if not float(self.depth_max) > 0:
            raise ValueError("depth_max must be positive (inf: no limit)")
        if not 0.0 < float(self.min_alpha) <= 1.0:
            raise ValueError("min_alpha must be in (0, 1]")
        if int(self.min_observations) < 1:
            raise ValueError("min_observations must be at least 1")
        if self.camera_batch is not None and int(self.camera_batch) < 1:
            raise ValueError("camera_batch must be at least 1")


def projview(camera) -> np.ndarray:
    """``proj_matrix @ view_matrix`` of the float32 matrices: the double product rounded once to float32 (float32 [4,4])."""
    v = camera.view_matrix.detach().cpu().numpy().astype(np.float32).astype(np.float64)
    p = camera.proj_matrix.detach().cpu().numpy().astype(np.float32).astype(np.float64)
    return (p @ v).astype(np.float32)


def cull_planes(view: np.ndarray, pv: np.ndarray) -> np.ndarray:
    """The six planes ``{n, d, |n|}`` of csrc/tsdf_math.h's sphere test, float32 [6,5], from the float32 ``view`` [4,4]
    and ``pv`` [4,4]: z; hw; ``k (hw + 1e-6) +- hx`` and ``+- hy`` with ``k = 1.125`` (an eighth of the image to spare on
    each side, which covers the float32 rounding of a pixel near the camera's plane)."""
    v, q = view.astype(np.float64), pv.astype(np.float64)
    eps = float(np.float32(1e-6))
    k = 1.125
    rows = [v[2], q[3]]
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            r = k * q[3] + sign * q[axis]
            r[3] += k * eps
            rows.append(r)
    out = np.zeros((_lib.TSDF_PLANES, 5), dtype=np.float64)
    for i, r in enumerate(rows):
        out[i, :4] = r
        out[i, 4] = np.linalg.norm(r[:3]) * (1.0 + 1e-6)
    return out.astype(np.float32)


def camera_table(cameras, depths) -> np.ndarray:
    """The host image of the device table: one ``_lib.TsTsdfCamera`` per camera, as bytes (uint8 [C * record])."""
    table = (_lib.TsTsdfCamera * len(cameras))()
    for rec, cam, depth in zip(table, cameras, depths):
        view = cam.view_matrix.detach().cpu().numpy().astype(np.float32)
        pv = projview(cam)
        h, w = int(depth.shape[0]), int(depth.shape[1])
        rec.view[:] = view[:3].reshape(-1).tolist()
        rec.proj[:] = pv[[0, 1, 3]].reshape(-1).tolist()
        rec.planes[:] = cull_planes(view, pv).reshape(-1).tolist()
        rec.width, rec.height, rec.depth = w, h, depth.data_ptr()
    return np.frombuffer(bytes(table), dtype=np.uint8).copy()


def _back_projected_box(cameras, depths, pvs, depth_max: float):
    """``(lo, hi)`` of the world points of all pixels with a depth, in double: per camera the extremes of the rays through
    the pixel centres at their depths (the three-plane solve of csrc/tsdf_math.h's unprojection, vectorised)."""
    lo = [math.inf] * 3
    hi = [-math.inf] * 3
    eps = float(np.float32(1e-6))
    for cam, depth, pv in zip(cameras, depths, pvs):
        dev = depth.device
        h, w = int(depth.shape[0]), int(depth.shape[1])
        d = depth.double()
        ok = torch.isfinite(depth) & (depth > 0) & (depth <= depth_max)
        if not bool(ok.any()):
            continue
        view = torch.from_numpy(cam.view_matrix.detach().cpu().numpy().astype(np.float64)).to(dev)
        q = torch.from_numpy(pv.astype(np.float64)).to(dev)
        nx = ((torch.arange(w, device=dev, dtype=torch.float64) + 0.5 - 0.5 * w) * 2.0 / w)[None, :, None]
        ny = ((torch.arange(h, device=dev, dtype=torch.float64) + 0.5 - 0.5 * h) * 2.0 / h)[:, None, None]
        a0 = (q[0, :3] - nx * q[3, :3]).expand(h, w, 3)
        a1 = (q[1, :3] - ny * q[3, :3]).expand(h, w, 3)
        a2 = view[2, :3].expand(h, w, 3)
        b0 = (nx[..., 0] * (eps + q[3, 3]) - q[0, 3]).expand(h, w)
        b1 = (ny[..., 0] * (eps + q[3, 3]) - q[1, 3]).expand(h, w)
        b2 = d - view[2, 3]
        c0, c1, c2 = torch.cross(a1, a2, dim=-1), torch.cross(a2, a0, dim=-1), torch.cross(a0, a1, dim=-1)
        det = (a0 * c0).sum(-1)
        x = (b0[..., None] * c0 + b1[..., None] * c1 + b2[..., None] * c2) / det[..., None]
        x = x[ok & (det != 0)]
        x = x[torch.isfinite(x).all(-1)]
        if x.shape[0]:
            lo = [min(a, b) for a, b in zip(lo, x.amin(0).tolist())]
            hi = [max(a, b) for a, b in zip(hi, x.amax(0).tolist())]
    return lo, hi


class _Chunk:
    """The buffers of one chunk of bricks, carved in the order of ``ts_tsdf_chunk_bytes``."""

    def __init__(self, lib, bricks: int, dev):
        ws = Workspace(int(lib.ts_tsdf_chunk_bytes(bricks)), dev)
        q = bricks * BRICK_CORNERS
        self.sum = ws.take(torch.float64, q)
        self.count = ws.take(torch.int32, q)
        self.field = ws.take(torch.float32, q)
        self.counts = ws.take(torch.int32, bricks)
        self.offsets = ws.take(torch.int64, bricks)
        ws.done()


@torch.no_grad()
def fuse_depth_maps(cameras, depths, config: Optional[FusionConfig] = None, return_debug: bool = False,
                    frustum_cull: bool = True):
    """The zero set of the fused field of ``depths`` (float32 [H_c, W_c] tensors of view-space z on one GPU; an entry that
    is not finite or is <= 0 is no depth) seen by ``cameras`` (``view_matrix``, ``proj_matrix``; the map's shape is the
    camera's size) as a ``TriangleMesh`` with ``normals=None`` and ``colors=None``.

    Stages: the camera table; the grid (by default over the back-projected depth samples); the flags of the bricks near a
    depth sample and their ascending list; per chunk of listed bricks (sized so that one chunk's buffers fit
    ``config.max_workspace_bytes``) the double sums and the counts over the cameras in list order, ``camera_batch`` at a
    time, the field, the triangle counts and the triangles as edge keys and positions; then the vertices are welded by
    key (``_bricks.weld``, as ``extract_mesh``'s), and the mesh is simplified and cleaned when configured.  The mesh is a fixed
    function of (cameras, depths, config): the same for any chunk size, any camera batch, ``sparse`` on or off and
    ``frustum_cull`` on or off (a debug switch: off, every corner is projected into every camera).

    ``return_debug``: also a dict of ``active_bricks`` int64 [A], ``field`` float32 [A,729], ``count`` int32 [A,729],
    ``keys`` int64 [T,3] and ``cell`` int64 [T] per triangle before welding, ``chunks``, ``total_bricks``, ``trunc`` and
    ``grid`` (``lo``, ``h``, ``cells``)."""
    cfg = config if config is not None else FusionConfig()
    cameras, depths = list(cameras), [_f32c(d.detach()) for d in depths]
    if not cameras or len(cameras) != len(depths):
        raise ValueError("one depth map per camera expected, and at least one camera")
    if len(cameras) > _MAX_CAMERAS:
        raise ValueError(f"at most {_MAX_CAMERAS} cameras")
    dev = _need_hip(*depths)
    for d in depths:
        if d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1 or d.numel() >= 2 ** 31:
            raise ValueError("a depth map is a float32 [H, W] tensor")
    lib = _lib.load()
    depth_max, znear = float(cfg.depth_max), float(cfg.znear)
    pvs = [projview(c) for c in cameras]
    res, tv = int(cfg.resolution), float(cfg.trunc_voxels)
    if cfg.bounds is None:
        lo_t, hi_t = _back_projected_box(cameras, depths, pvs, depth_max)
        try:
            lo_t, hi_t = _check_bounds(lo_t, hi_t)
        except ValueError as e:
            raise ValueError(f"the depth samples' box is no usable bound ({e}); give bounds") from None
        # widened by trunc = tv h on each side, with h = (longest + 2 trunc) / resolution
        longest = max(b - a for a, b in zip(lo_t, hi_t))
        trunc_w = tv * longest / (res - 2.0 * tv)
        lo_hi = ([a - trunc_w for a in lo_t], [b + trunc_w for b in hi_t])
    else:
        lo_hi = _check_bounds(*cfg.bounds)
    grid = BrickGrid(*lo_hi, res, cfg.max_workspace_bytes)
    glo, h, cells = grid.lo, grid.h, grid.cells
    trunc = ctypes.c_float(tv * h).value
    if not (trunc > 0 and math.isfinite(trunc)):
        raise ValueError("the truncation distance trunc_voxels * h is not a positive float32")
    reach = max(abs(v) for v in (*glo, *(a + h * c for a, c in zip(glo, cells))))
    for cam in cameras:
        view = cam.view_matrix.detach().cpu().numpy().astype(np.float64)
        if float((np.abs(view[:3, :3]).sum(1) * reach + np.abs(view[:3, 3])).max()) > _MAX_COORD_CELLS * h:
            raise ValueError("the grid's coordinates in a camera's frame exceed 2^16 cell edges: float32 cannot place a "
                             "corner in a pixel to a sixteenth of a cell there; move the scene or lower the resolution")
    grid.check_fits(int(lib.ts_tsdf_chunk_bytes(1)), "one brick")
    n_cam = len(cameras)
    batch = n_cam if cfg.camera_batch is None else min(int(cfg.camera_batch), n_cam)
    flags_arg = 0 if frustum_cull else _lib.TSDF_NO_CULL
    dbg = {"field": [], "count": []} if return_debug else None
    tail = {}
    with torch.cuda.device(dev):
        s = _stream(dev)
        table = torch.from_numpy(camera_table(cameras, depths)).to(dev)

        def mark(flags):
            _call("ts_tsdf_mark", lib.ts_tsdf_mark, n_cam, _ptr(table), max(int(d.numel()) for d in depths),
                  grid.grid_host, grid.cells_host, trunc, depth_max, _ptr(flags), s)

        def fill(ck, ids, b):
            q = b * BRICK_CORNERS
            ck.sum[:q].zero_()
            ck.count[:q].zero_()
            for c0 in range(0, n_cam, batch):
                _call("ts_tsdf_integrate", lib.ts_tsdf_integrate, b, _ptr(ids), grid.grid_host, grid.cells_host,
                      _ptr(table), c0, min(c0 + batch, n_cam), trunc, znear, depth_max, flags_arg, _ptr(ck.sum),
                      _ptr(ck.count), s)
            _call("ts_tsdf_field", lib.ts_tsdf_field, b, _ptr(ck.sum), _ptr(ck.count), int(cfg.min_observations),
                  _ptr(ck.field), s)
            if return_debug:
                dbg["field"].append(ck.field[:q].view(b, BRICK_CORNERS).clone())
                dbg["count"].append(ck.count[:q].view(b, BRICK_CORNERS).clone())
            return ck.field

        active = grid.active_bricks(cfg.sparse, mark, dev)
        # level 0, observed: a corner is inside where the field is positive, and a cell with a NaN corner emits nothing
        keys, pos, cell, chunks = march(lib, grid, active, lib.ts_tsdf_chunk_bytes, _MAX_BRICKS,
                                        lambda b: _Chunk(lib, b, dev), fill, 0.0, True, return_debug, s)
        vertices, faces = weld(keys, pos)
        del pos
        vertices, faces = mesh_tail(lib, vertices, faces, cfg, s, tail)
        torch.cuda.current_stream(dev).synchronize()        # the table and the maps it points to stay alive until here
    mesh = TriangleMesh(vertices, faces, None, None)
    if not return_debug:
        return mesh
    debug = {"active_bricks": active, "field": cat(dbg["field"], (0, BRICK_CORNERS), torch.float32, dev),
             "count": cat(dbg["count"], (0, BRICK_CORNERS), torch.int32, dev), "keys": keys, "cell": cell,
             "chunks": chunks, "total_bricks": grid.total_bricks, "trunc": trunc, "grid": grid.debug, **tail}
    return mesh, debug


@torch.no_grad()
def render_depth_alpha(model, camera, device=None):
    """``(depth, alpha)`` float32 [H,W] of ``model`` seen by ``camera``, forward only: one op-level compositing pass with
    the colour triple ``(z, 1, 0)`` over a zero background (the route ``rasterizer.py`` takes for its non-fused depth
    image) gives ``sum w z`` and ``alpha = sum w``; ``depth`` is their quotient, the expected depth of what the pixel sees.
    Thresholding by alpha is the caller's (``extract_mesh_tsdf``: ``min_alpha``)."""
    from . import ops
    from .rasterizer import camera_on_device, tile_bounds
    dev = torch.device(device) if device is not None else model.means.device
    w, h = int(camera.width), int(camera.height)
    view, pv, _ = camera_on_device(camera, dev)
    xys, z, radii, conics, num_tiles, _ = ops.project_gaussians(
        model.means, model.scales, 1., model.quats, view[:3, :], pv, camera.f_x, camera.f_y, w / 2, h / 2, h, w,
        tile_bounds((w, h)), log_scales=True, raw_quats=True)
    colors = torch.stack((z, torch.ones_like(z), torch.zeros_like(z)), dim=1)
    antialiased = ops.rasterize_mode(model) == "antialiased"        # compensated plain opacities
    opacity = ops.compensated_opacity(model, view[:3, :], camera.f_x, camera.f_y, w, h) if antialiased else model.opacities
    out, _ = ops.rasterize_gaussians(xys, z, radii, conics, num_tiles, colors, opacity, h, w,
                                     torch.zeros(3, dtype=torch.float32, device=dev), logit_opacity=not antialiased)
    alpha = out[:, :, 1].contiguous()
    depth = torch.where(alpha > 0, out[:, :, 0] / alpha, torch.zeros_like(alpha))
    return depth, alpha


@torch.no_grad()
def extract_mesh_tsdf(model, cameras, config: Optional[FusionConfig] = None, device="cuda:0",
                      return_debug: bool = False):
    """Renders the depth of every camera (``render_depth_alpha``; a pixel below ``config.min_alpha`` carries no depth)
    and fuses the maps (``fuse_depth_maps``).  Works for any model the rasteriser renders, a ``load_splat`` one
    included."""
    cfg = config if config is not None else FusionConfig()
    cameras = list(cameras)
    depths = []
    for cam in cameras:
        depth, alpha = render_depth_alpha(model, cam, device)
        depths.append(torch.where(alpha >= float(cfg.min_alpha), depth, torch.zeros_like(depth)).contiguous())
    return fuse_depth_maps(cameras, depths, cfg, return_debug=return_debug)
