"""What ``mesh.py`` and ``fusion.py`` (section 6p) share on the Python side of the sparse brick
grid (csrc/mesh.hip, csrc/mesh_cells.h): the grid and its bricks, the list of active bricks, the march of a field over
chunks of them (``ts_mesh_count`` / ``ts_mesh_emit`` and their observed forms), the weld, the simplify and clean tail and
the config fields both extractors carry.  An extractor supplies how bricks are flagged and how a chunk's corner field is
filled; everything after the field is here, once."""
import ctypes
import math

import torch
from torch import Tensor

from ._field import cat, largest
from .ops import _call, _ptr

BRICK = 8                       # TS_MESH_BRICK
BRICK_CORNERS = 729             # TS_MESH_BRICK_CORNERS


def _check_bounds(lo, hi):
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("bounds must be (lo [3], hi [3])")
    if not all(math.isfinite(v) for v in lo + hi):
        raise ValueError("bounds must be finite")
    if not all(b > a for a, b in zip(lo, hi)):
        raise ValueError("bounds must be non-empty on every axis")
    return lo, hi


def check_config(cfg):
    """The fields ``MeshConfig`` and ``FusionConfig`` share: ``resolution``, ``max_workspace_bytes``, ``bounds``,
    ``target_faces`` and ``clean``."""
    if int(cfg.resolution) < 1:
        raise ValueError("resolution must be at least 1")
    if int(cfg.max_workspace_bytes) < 1:
        raise ValueError("max_workspace_bytes must be positive")
    if cfg.bounds is not None:
        _check_bounds(*cfg.bounds)
    if cfg.target_faces is not None and int(cfg.target_faces) < 1:
        raise ValueError("target_faces must be at least 1")
    if cfg.clean is not None:
        from .clean import CleanConfig
        if not isinstance(cfg.clean, CleanConfig):
            raise ValueError("clean must be a CleanConfig or None")


def make_grid(lo, hi, resolution: int):
    """-> ``(lo float32 x 3, h float32, cells per axis)``: cubes of edge ``h = max(hi - lo) / resolution`` and
    ``ceil((hi_a - lo_a) / h)`` cells on axis a (``resolution`` on the longest).  ``lo`` and ``hi`` are rounded to
    float32 first; corner (i, j, k) sits at the float32 ``lo + (i, j, k) * h``."""
    lo, hi = _check_bounds(lo, hi)
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be at least 1")
    f32 = lambda v: ctypes.c_float(v).value
    lo, hi = [f32(v) for v in lo], [f32(v) for v in hi]
    ext = [b - a for a, b in zip(lo, hi)]
    longest = max(ext)
    h = f32(longest / res)
    if not (longest > 0 and h > 0 and math.isfinite(h)):
        raise ValueError("bounds must be non-empty on every axis")
    # (hi_a - lo_a) / h with h = longest / res, taken as a ratio so that the longest axis has exactly `res` cells
    cells = [max(1, math.ceil(e / longest * res - 1e-9)) for e in ext]
    return lo, h, cells


class BrickGrid:
    """``make_grid`` and its bricks of 8^3 cells: ``lo``, ``h``, ``cells``, ``bricks`` per axis, ``total_bricks``, the
    ``grid_host`` / ``cells_host`` arguments of the C entries, and ``cap``, the ``max_workspace_bytes`` the brick flags
    and a chunk's buffers have to fit."""

    def __init__(self, lo, hi, resolution: int, max_workspace_bytes: int):
        self.lo, self.h, self.cells = make_grid(lo, hi, resolution)
        self.cap = int(max_workspace_bytes)
        self.bricks = [-(-c // BRICK) for c in self.cells]
        self.total_bricks = self.bricks[0] * self.bricks[1] * self.bricks[2]
        self.grid_host = (ctypes.c_float * 4)(*self.lo, self.h)
        self.cells_host = (ctypes.c_int32 * 3)(*self.cells)

    @property
    def debug(self) -> dict:
        """The ``grid`` entry of the extractors' debug dicts."""
        return {"lo": tuple(self.lo), "h": self.h, "cells": tuple(self.cells)}

    def check_fits(self, one_brick_bytes: int, one_brick: str):
        """Refuses a cap below the brick flags (a byte each) or below the buffers of a chunk of one brick;
        ``one_brick`` names that chunk in the extractor's words."""
        if self.total_bricks > self.cap:
            raise ValueError(f"the flags of {self.total_bricks} bricks do not fit max_workspace_bytes = {self.cap}")
        if one_brick_bytes > self.cap:
            raise ValueError(f"max_workspace_bytes = {self.cap} is below the {one_brick_bytes} bytes {one_brick} needs")

    def active_bricks(self, sparse: bool, mark, dev) -> Tensor:
        """The bricks to evaluate, int64 ascending: those ``mark(flags)`` flags (the extractor's launch over zeroed
        uint8 [total_bricks]), or with ``sparse=False`` all of them."""
        if not sparse:
            return torch.arange(self.total_bricks, dtype=torch.int64, device=dev)
        flags = torch.zeros((self.total_bricks,), dtype=torch.uint8, device=dev)
        mark(flags)
        return torch.nonzero(flags).view(-1)                    # ascending, as the survivors of section 6f


def count_and_emit(lib, grid: BrickGrid, ids: Tensor, b: int, field: Tensor, counts: Tensor, offsets: Tensor,
                   level: float, observed: bool, want_cell: bool, s):
    """The triangles of the ``b`` bricks ``ids`` whose corner values ``field`` (float32 [>= b * 729]) holds, through the
    scratch ``counts`` int32 [>= b] and ``offsets`` int64 [>= b]: count, scan, emit -> ``(keys int64 [T,3], pos float32
    [T,3,3], cell int64 [T] or None)``, or None (and no emit launch) where there is no triangle.  ``observed``: the cell
    kernel in which a cell with a NaN corner emits nothing."""
    count, emit = (lib.ts_mesh_count_observed, lib.ts_mesh_emit_observed) if observed else \
        (lib.ts_mesh_count, lib.ts_mesh_emit)
    dev = ids.device
    _call(count.__name__, count, b, _ptr(ids), grid.grid_host, grid.cells_host, level, _ptr(field), _ptr(counts), s)
    ends = torch.cumsum(counts[:b], 0, dtype=torch.int64)
    t = int(ends[-1])
    if t == 0:
        return None
    offsets[:b] = ends - counts[:b]
    keys = torch.empty((t, 3), dtype=torch.int64, device=dev)
    pos = torch.empty((t, 3, 3), dtype=torch.float32, device=dev)
    cell = torch.empty((t,), dtype=torch.int64, device=dev) if want_cell else None
    _call(emit.__name__, emit, b, _ptr(ids), grid.grid_host, grid.cells_host, level, _ptr(field), _ptr(offsets),
          _ptr(keys), _ptr(pos), _ptr(cell), s)
    return keys, pos, cell


def march(lib, grid: BrickGrid, active: Tensor, chunk_bytes, max_bricks: int, make_chunk, fill, level: float,
          observed: bool, want_cell: bool, s):
    """The triangles of the ``active`` bricks, a chunk at a time -> ``(keys int64 [T,3], pos float32 [T,3,3], cell int64
    [T] or None, chunks)``, in the order of the list.

    A chunk holds the most bricks, ``max_bricks`` at the most, whose ``chunk_bytes(bricks)`` fit ``grid.cap``;
    ``make_chunk(bricks)`` carves its buffers, ``counts`` int32 [bricks] and ``offsets`` int64 [bricks] among them, and
    ``fill(chunk, ids, b)`` issues the extractor's launches for the ``b`` bricks ``ids`` and returns their corner field
    (float32, of the chunk's buffers).  A chunk with no corner above ``level`` launches nothing more.  The buffers are
    made and dropped here, before the parts are joined, so that they never stand beside the joined triangles."""
    dev = active.device
    a = int(active.shape[0])
    parts = []
    chunks = 0
    if a:
        per = largest(lambda b: int(chunk_bytes(b)) <= grid.cap, min(a, max_bricks))
        ck = make_chunk(per)
        for b0 in range(0, a, per):
            b = min(per, a - b0)
            chunks += 1
            ids = active[b0:b0 + b]
            field = fill(ck, ids, b)
            # no corner above the level: no triangle, and nothing to launch
            if not bool((field[:b * BRICK_CORNERS] > level).any()):
                continue
            tris = count_and_emit(lib, grid, ids, b, field, ck.counts, ck.offsets, level, observed, want_cell, s)
            if tris is not None:
                parts.append(tris)
        del ck, field
    keys = cat([p[0] for p in parts], (0, 3), torch.int64, dev)
    pos = cat([p[1] for p in parts], (0, 3, 3), torch.float32, dev)
    cell = cat([p[2] for p in parts], (0,), torch.int64, dev) if want_cell else None
    return keys, pos, cell, chunks


def weld(keys: Tensor, pos: Tensor):
    """The vertices welded by key: ascending key order, the first occurrence's position (all occurrences are
    bit-identical) -> ``(vertices float32 [V,3], faces int32 [T,3])``."""
    dev = keys.device
    if not keys.shape[0]:
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev))
    uniq, inv = torch.unique(keys.view(-1), sorted=True, return_inverse=True)
    v = int(uniq.shape[0])
    if v >= 2 ** 31:
        raise ValueError(f"{v} vertices do not fit int32 faces; lower the resolution")
    occ = torch.arange(inv.shape[0], dtype=torch.int64, device=dev)
    first = torch.full((v,), inv.shape[0], dtype=torch.int64, device=dev).scatter_reduce_(
        0, inv, occ, reduce="amin", include_self=True)
    return pos.view(-1, 3).index_select(0, first), inv.view(-1, 3).to(torch.int32)


def mesh_tail(lib, vertices: Tensor, faces: Tensor, cfg, s, debug: dict):
    """``cfg.target_faces`` (section 6i) and then ``cfg.clean`` (section 6j) applied to a welded mesh -> ``(vertices,
    faces)``; ``debug`` receives ``simplify`` and ``clean``, the debug dict of each step that ran."""
    if cfg.target_faces is not None:
        from .simplify import SimplifyConfig, _simplify
        debug["simplify"] = {}
        vertices, faces = _simplify(lib, vertices, faces, SimplifyConfig(
            target_faces=int(cfg.target_faces), max_workspace_bytes=int(cfg.max_workspace_bytes)), s, debug["simplify"])
    if cfg.clean is not None:
        from .clean import _clean
        debug["clean"] = {}
        vertices, faces, _ = _clean(lib, vertices, faces, cfg.clean, s, debug["clean"])
    return vertices, faces
