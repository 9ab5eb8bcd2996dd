"""Iso-surface triangle mesh of the SuGaR density: ``model -> mesh``, DESIGN.md section 6g.

The surface is the level set ``density_function = surface_level`` (model_gaussian.py:257-274, level 0.3) that the
density regulariser trains towards and ``extract.level_set_points`` samples, meshed by marching tetrahedra (the
Freudenthal split of every cell, csrc/mesh_cells.h) on a regular grid of cubes.  It stands in for the reference's
``export_mesh(..., 'marching_cubes')`` (model_gaussian.py:482-531), which cannot run as written; parity with mcubes is
not a goal.

Only the bricks (8^3 cells) near a Gaussian are evaluated.  **The sparsity condition**: a point outside every
Gaussian's axis-aligned box of half-size ``extent_sigmas * sqrt(Sigma_aa)`` has Mahalanobis ``q > extent_sigmas^2`` to
every Gaussian, so its 16-neighbour density is at most ``16 exp(-extent_sigmas^2 / 2)`` (0.178 at 3 sigma).
``MeshConfig`` refuses a ``surface_level`` at or below that bound; above it no corner outside all boxes is above the
level, every cell the surface crosses has a corner inside some box, and the bricks holding such cells give the mesh of
the dense grid bit for bit (``sparse=False`` evaluates every brick, to show it).  This is a condition, not a tuning knob.

``MeshConfig(colors=True)`` also colours the vertices from the Gaussians' spherical harmonics, seen head-on along the
normal (section 6h, csrc/field_color.hip); ``vertex_colors`` does the same for any points.

The grid, the list of active bricks, the march over chunks of them, the weld and the simplify and clean tail are
``_bricks.py``'s, shared with the depth-map fusion (``fusion.py``); what is here is the density's own: the boxes that flag
bricks and the corners, neighbours and densities that fill a chunk.

The hot path is csrc/mesh.hip on top of ``ts_knn``, ``ts_extract_pack`` and ``ts_extract_normals``; there is no CPU
fallback: tensors must be on the GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from ._bricks import BRICK, make_grid  # noqa: F401  (tests and tools import them from here)
from ._bricks import BRICK_CORNERS, BrickGrid, _check_bounds, check_config, march, mesh_tail, weld
from ._field import (EXTRACT_K, PackedModel, Workspace, align256, cat, colors_at, knn, largest, normals_at,
                     pack_model)
from .ops import _call, _f32c, _need_hip, _ptr, _stream

_MAX_BRICKS = (2 ** 31 - 1) // (BRICK_CORNERS * EXTRACT_K)
MAX_COLOR_DEGREE = 3            # ts_field_colors evaluates the bands 0..3


def level_floor(extent_sigmas: float) -> float:
    """``16 exp(-extent_sigmas^2 / 2)``: the most the density reaches outside every Gaussian's box."""
    return EXTRACT_K * math.exp(-0.5 * float(extent_sigmas) ** 2)


@dataclass
class MeshConfig:
    """``surface_level`` as ``ExtractConfig``; ``resolution``: cells along the longest axis of the bounds (256, the
    reference's literal); ``bounds``: ``(lo, hi)``, or None for the union of the Gaussians' boxes; ``extent_sigmas``:
    the half-size of a Gaussian's box in standard deviations per world axis; ``sparse=False`` evaluates every brick (a
    test and timing yardstick); ``max_workspace_bytes`` bounds the brick flags and every transient buffer of a chunk
    of bricks (the emitted triangles, the packed records and the returned tensors come on top); ``colors``: also the
    vertices' colours (section 6h), with the bands up to ``color_sh_degree`` (None: the model's ``active_sh_degree``;
    it may not exceed what the model stores); ``target_faces``: simplify the mesh to at most this many faces before the
    normals and colours are evaluated (section 6i, ``simplify.simplify_mesh``; None: the mesh as the grid gives it);
    ``clean``: a ``clean.CleanConfig``: remove the faces at non-manifold edges and the small components (section 6j,
    ``clean.clean_mesh``) after the simplification and before the normals and colours (None: no clean-up)."""
    surface_level: float = 0.3
    resolution: int = 256
    bounds: Optional[Tuple[Sequence[float], Sequence[float]]] = None
    extent_sigmas: float = 3.0
    sparse: bool = True
    normals: bool = True
    max_workspace_bytes: int = 256 << 20
    colors: bool = False
    color_sh_degree: Optional[int] = None
    target_faces: Optional[int] = None
    clean: Optional["CleanConfig"] = None

    def __post_init__(self):
        if not (isinstance(self.extent_sigmas, (int, float)) and math.isfinite(self.extent_sigmas)
                and self.extent_sigmas > 0):
            raise ValueError("extent_sigmas must be positive and finite")
        if not math.isfinite(float(self.surface_level)):
            raise ValueError("surface_level must be finite")
        if not float(self.surface_level) > level_floor(self.extent_sigmas):
            raise ValueError(f"surface_level = {self.surface_level} is not above 16 exp(-extent_sigmas^2 / 2) = "
                             f"{level_floor(self.extent_sigmas):.4f}: the density may reach it outside every Gaussian's "
                             "box and the sparse grid would miss surface")
        check_config(self)
        if self.color_sh_degree is not None and not 0 <= int(self.color_sh_degree) <= MAX_COLOR_DEGREE:
            raise ValueError(f"color_sh_degree must be in 0..{MAX_COLOR_DEGREE}")


@dataclass
class TriangleMesh:
    """``vertices`` float32 [V,3] in ascending order of their edge keys; ``faces`` int32 [F,3], wound so that the
    geometric normal points towards falling density; ``normals`` float32 [V,3], ``-grad d / |grad d|`` at the vertices
    (zero where undefined), or None; ``colors`` float32 [V,3] in [0, 1] (section 6h), or None."""
    vertices: Tensor
    faces: Tensor
    normals: Optional[Tensor]
    colors: Optional[Tensor] = None


class _Chunk:
    """The buffers of one chunk of bricks, carved in the order of ``ts_mesh_chunk_bytes``."""

    def __init__(self, lib, n: int, bricks: int, dev):
        ws = Workspace(int(lib.ts_mesh_chunk_bytes(n, bricks)), dev)
        q = bricks * BRICK_CORNERS
        self.knn_ws = ws.take(torch.uint8, int(lib.ts_knn_ws_bytes(n, q, EXTRACT_K)))
        self.corners = ws.take(torch.float32, q, 3)
        self.knn_dist = ws.take(torch.float32, q, EXTRACT_K)
        self.knn_idx = ws.take(torch.int32, q, EXTRACT_K)
        self.density = ws.take(torch.float32, q)
        self.counts = ws.take(torch.int32, bricks)
        self.offsets = ws.take(torch.int64, bricks)
        self.stats = ws.take(torch.int32, bricks, 2)
        ws.done()


@torch.no_grad()
def gaussian_boxes(model, extent_sigmas: float = 3.0) -> Tensor:
    """``ts_mesh_boxes``: float32 [N,6], ``{lo, hi}`` of every Gaussian's axis-aligned box of half-size
    ``extent_sigmas * sqrt(Sigma_aa)``."""
    means, scales, quats = (_f32c(t.detach()) for t in (model.means, model.scales, model.quats))
    dev = _need_hip(means, scales, quats)
    n = means.shape[0]
    boxes = torch.empty((n, 6), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_mesh_boxes", _lib.load().ts_mesh_boxes, n, _ptr(means), _ptr(scales), _ptr(quats),
              float(extent_sigmas), _ptr(boxes), _stream(dev))
    return boxes


def _color_coeffs(model, n: int, sh_degree: Optional[int]):
    """-> ``(colors_dc [N,3], colors_rest [N,K,3], degree)`` of ``model`` for ``ts_field_colors``: ``sh_degree``, or the
    model's ``active_sh_degree``; refused when the model does not store its bands."""
    dc, rest = _f32c(model.colors_dc.detach()), _f32c(model.colors_rest.detach())
    _need_hip(dc, rest)
    if dc.shape != (n, 3) or rest.dim() != 3 or rest.shape[0] != n or rest.shape[2] != 3:
        raise ValueError(f"colors_dc [{n},3] and colors_rest [{n},K,3] expected")
    degree = int(model.active_sh_degree if sh_degree is None else sh_degree)
    if not 0 <= degree <= MAX_COLOR_DEGREE:
        raise ValueError(f"the colours take an SH degree in 0..{MAX_COLOR_DEGREE}, got {degree}")
    if (degree + 1) ** 2 > rest.shape[1] + 1:
        raise ValueError(f"SH degree {degree} needs {(degree + 1) ** 2} coefficients, the model stores {rest.shape[1] + 1}")
    return dc, rest, degree


_OWN = "own"


def _at_points(lib, pk: PackedModel, points: Tensor, cap: int, s, want_normals: bool, coeffs, along=_OWN):
    """The normals and / or the colours of ``points`` [P,3] in chunks whose buffers fit ``cap`` bytes, one neighbour
    search per chunk -> ``(normals or None, colors or None)``.  ``coeffs``: ``_color_coeffs``'s, or None for no colours.
    The colours look along the normals evaluated here (``along=_OWN``), or along the caller's [P,3] (None: band 0)."""
    dev = points.device
    n, v = pk.means.shape[0], int(points.shape[0])
    f32 = dict(dtype=torch.float32, device=dev)
    evaluate = want_normals or (coeffs is not None and along is _OWN)
    normals = torch.empty((v, 3), **f32) if want_normals else None
    colors = torch.empty((v, 3), **f32) if coeffs is not None else None
    if not v or not (evaluate or coeffs is not None):
        return normals, colors
    scratch = evaluate and not want_normals            # normals the colours need and the caller does not get

    def fits(p):
        return int(lib.ts_knn_ws_bytes(n, p, EXTRACT_K)) + 2 * align256(p * EXTRACT_K * 4) \
            + (align256(p * 12) if scratch else 0) <= cap
    per = largest(fits, min(v, (2 ** 31 - 2) // EXTRACT_K))
    if per < 1:
        raise ValueError(f"max_workspace_bytes = {cap} is too small for the normals of one vertex")
    ws = torch.empty((int(lib.ts_knn_ws_bytes(n, per, EXTRACT_K)),), dtype=torch.uint8, device=dev)
    dist = torch.empty((per, EXTRACT_K), **f32)
    idx = torch.empty((per, EXTRACT_K), dtype=torch.int32, device=dev)
    own = torch.empty((per, 3), **f32) if scratch else None
    for v0 in range(0, v, per):
        p = min(per, v - v0)
        pts = points[v0:v0 + p]
        nrm = None if along is _OWN or along is None else along[v0:v0 + p]
        if evaluate:
            nrm = normals[v0:v0 + p] if want_normals else own
            normals_at(lib, pk, pts, p, nrm, dist, idx, ws, s)
        if coeffs is not None:
            colors_at(lib, pk, coeffs[0], coeffs[1], pts, nrm, p, coeffs[2], colors[v0:v0 + p], dist, idx, ws, s,
                      search=not evaluate)
    return normals, colors


@torch.no_grad()
def vertex_colors(model, points: Tensor, normals: Optional[Tensor] = None, sh_degree: Optional[int] = None,
                  max_workspace_bytes: int = 256 << 20, packed: Optional[PackedModel] = None) -> Tensor:
    """The colours (float32 [P,3] in [0, 1], section 6h) of any ``points`` float32 [P,3] on the model's device, e.g. an
    ``extract.SurfacePoints``' points: each point's 16 nearest Gaussians, weighed as the density weighs them, seen along
    ``-normals`` (unit, outward; None: band 0 only, as where a normal is zero).  ``sh_degree``: None for the model's
    ``active_sh_degree``.  The same bits for any ``max_workspace_bytes``; ``packed``: a ``pack_model`` result to reuse."""
    cap = int(max_workspace_bytes)
    if cap < 1:
        raise ValueError("max_workspace_bytes must be positive")
    pk = packed if packed is not None else pack_model(model)
    points = _f32c(points.detach())
    dev = _need_hip(pk.means, pk.records, points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points [P,3] expected")
    if normals is not None:
        normals = _f32c(normals.detach())
        if _need_hip(normals) != dev or normals.shape != points.shape:
            raise ValueError("normals must match points in shape and device")
    coeffs = _color_coeffs(model, pk.means.shape[0], sh_degree)
    with torch.cuda.device(dev):
        return _at_points(_lib.load(), pk, points, cap, _stream(dev), False, coeffs, along=normals)[1]


@torch.no_grad()
def extract_mesh(model, config: Optional[MeshConfig] = None, return_debug: bool = False,
                 packed: Optional[PackedModel] = None):
    """The level set ``d = config.surface_level`` of ``model`` as a ``TriangleMesh`` on the model's device.

    Stages: the Gaussians' boxes and (by default) the bounds as their union; the flags of the bricks a box reaches and
    their ascending list; per chunk of listed bricks (sized so that one chunk's buffers fit
    ``config.max_workspace_bytes``) the 9^3 corner positions, their 16 neighbours (``ts_knn``), the densities, the
    triangle counts and the triangles as edge keys and positions; then the vertices are welded by key
    (``torch.unique``: ascending key order, the first occurrence's position - all occurrences are bit-identical) and the
    normals (and, with ``config.colors``, the colours: from the same neighbour lists) evaluated at them in chunks of
    vertices.  The mesh is a fixed function of (model, config): the same for any chunk size and for
    ``sparse`` on or off.  A surface that leaves the bounds is cut there (an open boundary).  With
    ``config.target_faces`` the welded mesh is simplified to that budget (``simplify.simplify_mesh``, section 6i) before
    the normals and colours are evaluated, at the simplified vertices; ``keys`` and ``cell`` below describe the mesh
    before that, ``simplify`` (``simplify_mesh``'s debug dict) the step itself.  With ``config.clean`` the mesh is then
    cleaned (``clean.clean_mesh``, section 6j; ``clean`` in the debug dict is its debug dict), again before the normals
    and colours, which are evaluated at the vertices that stay.

    ``return_debug``: also a dict of ``active_bricks`` int64 [A], ``cell`` int64 [T] and ``keys`` int64 [T,3] per
    triangle before welding, ``corners`` float32 [A,729,3], ``knn`` int32 [A,729,16] and ``density`` float32 [A,729] of
    the active bricks, ``knn_fallback`` int32 [A] (the corner queries of each brick that took ``ts_knn``'s brute-force
    pass: the search then runs brick by brick, with the same result), ``chunks``, ``total_bricks`` and ``grid``
    (``lo``, ``h``, ``cells``).  ``packed``: a ``pack_model`` result to reuse."""
    cfg = config if config is not None else MeshConfig()
    pk = packed if packed is not None else pack_model(model)            # refuses fewer than 16 Gaussians
    dev = _need_hip(pk.means, pk.records)
    n = pk.means.shape[0]
    lib = _lib.load()
    coeffs = _color_coeffs(model, n, cfg.color_sh_degree) if cfg.colors else None     # refused before any work
    cap = int(cfg.max_workspace_bytes)
    level = float(cfg.surface_level)
    boxes = gaussian_boxes(model, cfg.extent_sigmas)
    if cfg.bounds is None:
        lo_t, hi_t = boxes[:, :3].amin(0).tolist(), boxes[:, 3:].amax(0).tolist()
        try:
            lo_hi = _check_bounds(lo_t, hi_t)
        except ValueError as e:
            raise ValueError(f"the union of the Gaussians' boxes is no usable bound ({e}); give bounds") from None
    else:
        lo_hi = _check_bounds(*cfg.bounds)
    grid = BrickGrid(*lo_hi, cfg.resolution, cap)
    grid.check_fits(int(lib.ts_mesh_chunk_bytes(n, 1)), f"one brick over {n} Gaussians")
    dbg = {k: [] for k in ("corners", "knn", "density", "knn_fallback")} if return_debug else None
    tail = {}
    with torch.cuda.device(dev):
        s = _stream(dev)

        def mark(flags):
            _call("ts_mesh_mark", lib.ts_mesh_mark, n, _ptr(boxes), grid.grid_host, grid.cells_host, _ptr(flags), s)

        def fill(ck, ids, b):
            q = b * BRICK_CORNERS
            _call("ts_mesh_corners", lib.ts_mesh_corners, b, _ptr(ids), grid.grid_host, grid.cells_host,
                  _ptr(ck.corners), s)
            if return_debug:
                # brick by brick, for the per-brick share of brute-force queries; the lists are the same
                for i in range(b):
                    r = slice(i * BRICK_CORNERS, (i + 1) * BRICK_CORNERS)
                    knn(lib, pk, ck.corners[r], BRICK_CORNERS, EXTRACT_K, ck.knn_dist[r], ck.knn_idx[r], ck.knn_ws,
                        ck.stats[i], s)
            else:
                knn(lib, pk, ck.corners, q, EXTRACT_K, ck.knn_dist, ck.knn_idx, ck.knn_ws, None, s)
            _call("ts_mesh_density", lib.ts_mesh_density, n, b, _ptr(ids), grid.grid_host, grid.cells_host,
                  _ptr(ck.corners), _ptr(ck.knn_idx), _ptr(pk.records), _ptr(ck.density), s)
            if return_debug:
                dbg["corners"].append(ck.corners[:q].view(b, BRICK_CORNERS, 3).clone())
                dbg["knn"].append(ck.knn_idx[:q].view(b, BRICK_CORNERS, EXTRACT_K).clone())
                dbg["density"].append(ck.density[:q].view(b, BRICK_CORNERS).clone())
                dbg["knn_fallback"].append(ck.stats[:b, 0].clone())
            return ck.density

        active = grid.active_bricks(cfg.sparse, mark, dev)
        keys, pos, cell, chunks = march(lib, grid, active, lambda b: lib.ts_mesh_chunk_bytes(n, b), _MAX_BRICKS,
                                        lambda b: _Chunk(lib, n, b, dev), fill, level, False, return_debug, s)
        vertices, faces = weld(keys, pos)
        del pos
        vertices, faces = mesh_tail(lib, vertices, faces, cfg, s, tail)
        normals, colors = _at_points(lib, pk, vertices, cap, s, cfg.normals, coeffs)
    mesh = TriangleMesh(vertices, faces, normals, colors)
    if not return_debug:
        return mesh
    shapes = {"corners": ((0, BRICK_CORNERS, 3), torch.float32), "knn": ((0, BRICK_CORNERS, EXTRACT_K), torch.int32),
              "density": ((0, BRICK_CORNERS), torch.float32), "knn_fallback": ((0,), torch.int32)}
    debug = {k: cat(v, *shapes[k], dev) for k, v in dbg.items()}
    debug.update(active_bricks=active, keys=keys, cell=cell, chunks=chunks, total_bricks=grid.total_bricks,
                 grid=grid.debug, **tail)
    return mesh, debug
