"""Triangle-budget simplification of a mesh on the GPU: ``mesh -> mesh``, DESIGN.md section 6i.

Stands in for the ``simplify_quadric_decimation(250_000)`` + ``remove_degenerate_triangles`` +
``remove_duplicated_triangles`` + ``remove_duplicated_vertices`` that the reference runs on every mesh before writing it
(model_gaussian.py:376-386).  It is not a port of open3d's edge collapse, and parity with it is not a goal: this is
vertex clustering with quadric-optimal representatives (Lindstrom, "Out-of-core simplification of large polygonal
models", 2000).  The vertices are filed into the cubes of a uniform grid; every occupied cube becomes one vertex, placed
where the summed squared distance to the planes of the faces around the cube's vertices is least (kept inside the cube);
faces with two corners in one cube go, duplicates go.  The cube's edge is either given or found by bisection, the
finest of ``max extent / r`` that leaves at most ``target_faces`` faces.

Deterministic: sorts, segmented sums in a fixed order and one small solve per cluster (csrc/simplify.hip, the arithmetic
in csrc/simplify_math.h); no float atomics, the same bits for any ``max_workspace_bytes``.  There is no CPU fallback:
tensors must be on the GPU.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._field import PackedModel, largest, pack_model
from .ops import _call, _f32c, _i32c, _need_hip, _ptr, _stream

CHUNK = 128                     # TS_SIMPLIFY_CHUNK
QUADRIC = 10                    # TS_SIMPLIFY_QUADRIC
VSUM = 4                        # TS_SIMPLIFY_VSUM
FACE_CORNERS, VERTICES = 0, 1   # TS_SIMPLIFY_FACE_CORNERS, TS_SIMPLIFY_VERTICES
COUNT_BLOCK = 256               # faces per workgroup of ts_simplify_count
# The finest grid the search tries.  A float32 coordinate carries 24 bits, so at r = 2^20 a cell is 16 ulps of the
# largest extent wide: finer grids tell no more vertices apart; and 2^20 cells per axis keep the int64 key below 2^61.
R_MAX = 1 << 20
_MAX_CELLS = 1 << 62


@dataclass
class SimplifyConfig:
    """``target_faces``: the most faces the result may have (250 000: the reference's ``decimation_target``); None
    requires ``cell_size``.  ``cell_size``: the clusters' edge, given outright (the search is skipped).
    ``singular_threshold``: tau, the share of the largest eigenvalue below which a direction of the quadric is left at the
    cluster's mean.  ``max_workspace_bytes`` bounds the accumulation's per-chunk partial sums (the sorted corner lists
    and the returned tensors come on top) and the buffers of the normals and colours."""
    target_faces: Optional[int] = 250_000
    cell_size: Optional[float] = None
    singular_threshold: float = 1e-3
    max_workspace_bytes: int = 256 << 20

    def __post_init__(self):
        if self.target_faces is None and self.cell_size is None:
            raise ValueError("give target_faces or cell_size")
        if self.target_faces is not None and int(self.target_faces) < 1:
            raise ValueError("target_faces must be at least 1")
        if self.cell_size is not None and not (math.isfinite(float(self.cell_size)) and float(self.cell_size) > 0):
            raise ValueError("cell_size must be positive and finite")
        if not 0.0 < float(self.singular_threshold) < 1.0:
            raise ValueError("singular_threshold must lie in (0, 1)")
        if int(self.max_workspace_bytes) < 1:
            raise ValueError("max_workspace_bytes must be positive")


def grid_at(lo, hi, c):
    """``(grid_host, cells_host, cells)`` of the clusters of edge ``c`` (float32) over ``[lo, hi]`` (float32 [3]):
    ``max(1, ceil((hi_a - lo_a) / c))`` cells on axis a, difference and quotient in float32 as ts_simplify_cells."""
    c = np.float32(c)
    with np.errstate(over="ignore", divide="ignore"):
        q = np.ceil((hi - lo) / c)
    if not (np.isfinite(c) and c > 0 and np.isfinite(q).all()):
        raise ValueError(f"cell_size = {float(c)} is no usable cluster edge for this mesh")
    cells = [max(1, int(x)) for x in q]
    if max(cells) >= 2 ** 31 - 1 or cells[0] * cells[1] * cells[2] >= _MAX_CELLS:
        raise ValueError(f"cell_size = {float(c)} gives {cells} clusters per axis: too many for an int64 key")
    return (ctypes.c_float * 4)(*lo.tolist(), float(c)), (ctypes.c_int32 * 3)(*cells), cells


def resolution_edge(extent, r: int):
    """The float32 cluster edge at resolution ``r``: ``extent / r``, one float32 division."""
    return np.float32(extent) / np.float32(r)


def _empty(dev):
    return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev))


def _simplify(lib, vertices: Tensor, faces: Tensor, cfg: SimplifyConfig, s, info: Optional[dict] = None):
    """``(vertices, faces)`` simplified as section 6i defines -> ``(vertices, faces)``; the inputs themselves where the
    budget already holds.  ``info``: a dict that receives ``r``, ``cell_size``, ``cells``, ``probes``, ``keys`` (int64,
    the kept clusters' cell keys, ascending), ``clusters`` (before the unreferenced go) and ``pieces``; an ``info`` that
    comes with ``want_sums`` also receives ``quadrics``, ``vertex_sums`` and ``cluster_keys`` of all clusters."""
    dev = vertices.device
    f = int(faces.shape[0])
    info = info if info is not None else {}
    if cfg.cell_size is None and f <= int(cfg.target_faces):
        info.update(r=None, cell_size=None, probes=0)
        return vertices, faces
    if f == 0:
        info.update(r=None, cell_size=cfg.cell_size, probes=0)
        return _empty(dev)
    v = int(vertices.shape[0])
    if v < 1 or int(faces.min()) < 0 or int(faces.max()) >= v:
        raise ValueError("faces index outside the vertices")
    flat = faces.view(-1).long()
    used = torch.zeros((v,), dtype=torch.bool, device=dev)
    used[flat] = True
    if not bool(used.all()):                    # unreferenced vertices take no part: not in the bounds, not in a mean
        renumber = torch.cumsum(used, 0, dtype=torch.int32) - 1
        vertices = vertices[used].contiguous()
        faces = renumber[flat].view(-1, 3).contiguous()
        flat = faces.view(-1).long()
        v = int(vertices.shape[0])
    del used
    lo, hi = vertices.amin(0).cpu().numpy(), vertices.amax(0).cpu().numpy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("the vertices must be finite")
    extent = np.float32((hi - lo).max())
    if not extent > 0:                          # every vertex in one place: no face has an area
        info.update(r=None, cell_size=cfg.cell_size, probes=0)
        return _empty(dev)
    cap = int(cfg.max_workspace_bytes)
    entries = 3 * f
    nchunks = -(-max(entries, v) // CHUNK)
    per = largest(lambda k: int(lib.ts_simplify_ws_bytes(k)) <= cap, nchunks)
    if per < 1:
        raise ValueError(f"max_workspace_bytes = {cap} is below the {int(lib.ts_simplify_ws_bytes(1))} bytes one chunk "
                         "of the accumulation needs")
    i32 = dict(dtype=torch.int32, device=dev)

    # the cluster edge: given, or the finest extent / r that leaves at most target_faces faces
    probes = 0
    if cfg.cell_size is not None:
        r, c = None, np.float32(cfg.cell_size)
    else:
        counts = torch.empty((-(-f // COUNT_BLOCK),), **i32)

        def count(r):
            nonlocal probes
            probes += 1
            g, n, _ = grid_at(lo, hi, resolution_edge(extent, r))
            _call("ts_simplify_count", lib.ts_simplify_count, v, f, _ptr(vertices), _ptr(faces), g, n, _ptr(counts), s)
            return int(counts.sum(dtype=torch.int64))
        target = int(cfg.target_faces)
        r, top = 1, R_MAX                       # count(1) == 0: one cluster
        if count(top) <= target:
            r = top
        while top - r > 1:
            mid = (r + top) // 2
            if count(mid) <= target:
                r = mid
            else:
                top = mid
        c = resolution_edge(extent, r)
        del counts
    grid_host, cells_host, cells = grid_at(lo, hi, c)

    keys = torch.empty((v,), dtype=torch.int64, device=dev)
    _call("ts_simplify_keys", lib.ts_simplify_keys, v, _ptr(vertices), grid_host, cells_host, _ptr(keys), s)
    uniq, inv = torch.unique(keys, sorted=True, return_inverse=True)
    del keys
    clusters = int(uniq.shape[0])
    vertex_cluster = inv.to(torch.int32)
    del inv

    # the sums per cluster: the quadrics over the face corners, p - g and the count over the vertices
    quadrics = torch.zeros((clusters, QUADRIC), dtype=torch.float64, device=dev)
    vsums = torch.zeros((clusters, VSUM), dtype=torch.float64, device=dev)
    ws = torch.empty((int(lib.ts_simplify_ws_bytes(per)),), dtype=torch.uint8, device=dev)
    pieces = 0
    for what, n_entries, of, sums in ((FACE_CORNERS, entries, vertex_cluster[flat], quadrics),
                                      (VERTICES, v, vertex_cluster, vsums)):
        sorted_clusters, order = torch.sort(of, stable=True)
        del of
        total = -(-n_entries // CHUNK)
        for c0 in range(0, total, per):
            pieces += 1
            _call("ts_simplify_accumulate", lib.ts_simplify_accumulate, v, f, clusters, _ptr(vertices), _ptr(faces),
                  grid_host, cells_host, what, n_entries, _ptr(sorted_clusters), _ptr(order), c0, min(per, total - c0),
                  _ptr(sums), _ptr(ws), s)
        del sorted_clusters, order
    del ws, flat
    if info.get("want_sums"):                   # the tests compare the sums themselves
        info.update(quadrics=quadrics, vertex_sums=vsums, cluster_keys=uniq)
    reps = torch.empty((clusters, 3), dtype=torch.float32, device=dev)
    _call("ts_simplify_solve", lib.ts_simplify_solve, clusters, _ptr(uniq), grid_host, cells_host, _ptr(quadrics),
          _ptr(vsums), float(cfg.singular_threshold), _ptr(reps), s)
    del quadrics, vsums

    tri = torch.empty((f, 3), **i32)
    keep = torch.empty((f,), dtype=torch.uint8, device=dev)
    _call("ts_simplify_faces", lib.ts_simplify_faces, v, f, _ptr(faces), _ptr(vertex_cluster), _ptr(tri), _ptr(keep), s)
    tri = tri[keep.bool()]
    del keep, vertex_cluster
    info.update(r=r, cell_size=float(c), cells=tuple(cells), probes=probes, clusters=clusters, pieces=pieces)
    if tri.shape[0] == 0:
        info["keys"] = uniq[:0]
        return _empty(dev)
    # ascending rows, duplicates gone; (a, b, c) and (a, c, b), the same corners wound the other way, are two rows
    tri = torch.unique(tri, dim=0)
    seen = torch.zeros((clusters,), dtype=torch.bool, device=dev)
    seen[tri.view(-1).long()] = True
    renumber = torch.cumsum(seen, 0, dtype=torch.int32) - 1
    info["keys"] = uniq[seen]
    return reps[seen].contiguous(), renumber[tri.view(-1).long()].view(-1, 3).contiguous()


@torch.no_grad()
def simplify_mesh(mesh, config: Optional[SimplifyConfig] = None, model=None, color_sh_degree: Optional[int] = None,
                  packed: Optional[PackedModel] = None, return_debug: bool = False):
    """``mesh`` (a ``mesh.TriangleMesh`` on the GPU) with at most ``config.target_faces`` faces (or clustered at
    ``config.cell_size``), as section 6i defines: a fixed function of (mesh, config).  The vertices come in ascending
    order of their cluster keys, the faces in ascending lexicographic order, each starting at its smallest index and
    wound as before.  Where ``mesh`` already meets the budget and no ``cell_size`` is given, ``mesh`` itself is returned.

    ``model``: the model the mesh was extracted from; the normals and the colours are then evaluated again at the new
    vertices (each where ``mesh`` had it; the colours with the bands up to ``color_sh_degree``, None for the model's
    ``active_sh_degree``).  Without a model both are None.  ``packed``: a ``pack_model`` result to reuse.
    ``return_debug``: also a dict of ``r`` (the resolution the search chose, None without a search), ``cell_size``,
    ``cells``, ``probes`` (launches of the search), ``clusters``, ``pieces`` (launches of the accumulation) and ``keys``
    (int64, the cell key of every vertex of the result)."""
    from .mesh import MAX_COLOR_DEGREE, TriangleMesh, _at_points, _color_coeffs
    cfg = config if config is not None else SimplifyConfig()
    vertices, faces = mesh.vertices, mesh.faces
    if not (isinstance(vertices, Tensor) and isinstance(faces, Tensor)):
        raise TypeError("expected torch tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("vertices [V,3] and faces [F,3] expected")
    if color_sh_degree is not None and not 0 <= int(color_sh_degree) <= MAX_COLOR_DEGREE:
        raise ValueError(f"color_sh_degree must be in 0..{MAX_COLOR_DEGREE}")
    vertices, faces = _f32c(vertices.detach()), _i32c(faces)
    dev = _need_hip(vertices, faces)
    want_normals = model is not None and mesh.normals is not None
    coeffs = pk = None
    if model is not None and (want_normals or mesh.colors is not None):
        pk = packed if packed is not None else pack_model(model)
        if _need_hip(pk.means, pk.records) != dev:
            raise ValueError("the mesh and the model must live on the same device")
        if mesh.colors is not None:
            coeffs = _color_coeffs(model, pk.means.shape[0], color_sh_degree)
    lib = _lib.load()
    info = {}
    with torch.cuda.device(dev):
        s = _stream(dev)
        new_vertices, new_faces = _simplify(lib, vertices, faces, cfg, s, info)
        if new_vertices is vertices and new_faces is faces:
            out = mesh
        else:
            normals = colors = None
            if pk is not None:
                normals, colors = _at_points(lib, pk, new_vertices, int(cfg.max_workspace_bytes), s, want_normals, coeffs)
            out = TriangleMesh(new_vertices, new_faces, normals, colors)
    return (out, info) if return_debug else out
