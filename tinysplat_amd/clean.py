"""Mesh clean-up on the GPU: ``mesh -> mesh``, DESIGN.md section 6j.

Two steps a simplified splat mesh needs before it is written.  The first stands in for the reference's
``remove_non_manifold_edges()`` (model_gaussian.py:386), the last of its four clean-ups (``simplify.py`` stands in for the
other three): at every edge that more than two faces use, the two largest faces stay and the others go, in one pass.  It
is not a port of open3d's loop, which removes the smallest face at a time and counts again, and parity with it is not a
goal.  The second drops small connected components, the closed little shells that stray Gaussians mesh into: a
component is kept by its face count, by its share of the largest component's, or by its rank.

Both are integer work (the faces' areas: fixed IEEE operations in double), so the result is a fixed function of
(mesh, config), bit-identical from run to run.  The vertices do not move: the kept ones keep their order, their normals
and their colours.  The hot path is csrc/clean.hip (the arithmetic in csrc/clean_math.h); there is no CPU fallback:
tensors must be on the GPU.
"""
from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _i32c, _need_hip, _ptr, _stream


@dataclass
class CleanConfig:
    """``manifold_edges``: remove, at every edge of more than two faces, all but the two largest.
    ``min_component_faces``: a component with fewer faces goes.  ``min_component_fraction``: a component with fewer than
    this share of the largest component's faces goes.  ``keep_largest``: only this many components stay, the largest
    first (ties: the smaller label first); None for no limit."""
    manifold_edges: bool = True
    min_component_faces: int = 0
    min_component_fraction: float = 0.0
    keep_largest: Optional[int] = None

    def __post_init__(self):
        for name in ("min_component_faces", "keep_largest"):
            count = getattr(self, name)
            absent = count is None and name == "keep_largest"
            if isinstance(count, bool) or not (absent or isinstance(count, numbers.Integral)):
                raise ValueError(f"{name} must be an integer")
        if int(self.min_component_faces) < 0:
            raise ValueError("min_component_faces must not be negative")
        if not 0.0 <= float(self.min_component_fraction) <= 1.0:           # not-a-number fails both comparisons
            raise ValueError("min_component_fraction must lie in [0, 1]")
        if self.keep_largest is not None and int(self.keep_largest) < 1:
            raise ValueError("keep_largest must be at least 1")

    @property
    def filters(self) -> bool:
        """Whether any component can go."""
        return int(self.min_component_faces) > 1 or float(self.min_component_fraction) > 0.0 \
            or self.keep_largest is not None


def _check(vertices, faces):
    """The input errors of this module, before any of its launches -> contiguous ``(vertices, faces, device)``."""
    if not (isinstance(vertices, Tensor) and isinstance(faces, Tensor)):
        raise TypeError("expected torch tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("vertices [V,3] and faces [F,3] expected")
    vertices, faces = _f32c(vertices.detach()), _i32c(faces)
    dev = _need_hip(vertices, faces)
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    if f and (v < 1 or int(faces.min()) < 0 or int(faces.max()) >= v):
        raise ValueError("faces index outside the vertices")
    if v and not bool(torch.isfinite(vertices).all()):
        raise ValueError("the vertices must be finite")
    return vertices, faces, dev


def _nonmanifold_faces(lib, vertices: Tensor, faces: Tensor, s, info: dict) -> Optional[Tensor]:
    """uint8 [F], 1 for the faces of rank two and above at an edge of valence above two (section 6j, step 1); None where
    every edge has at most two faces.  ``faces`` has no face with two equal indices."""
    dev = faces.device
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    if f < 3:
        return None
    keys = torch.empty((3 * f,), dtype=torch.int64, device=dev)
    _call("ts_clean_edge_keys", lib.ts_clean_edge_keys, v, f, _ptr(faces), _ptr(keys), s)
    # the early exit, on the keys alone: no key three times in the sorted list
    alone = torch.sort(keys).values
    crowded = alone[2:] == alone[:-2]
    if not bool(crowded.any()):
        return None
    uniq, counts = torch.unique_consecutive(alone, return_counts=True)
    info["nonmanifold_edges"] = int((counts > 2).sum())
    del alone, crowded, uniq, counts
    weights = torch.empty((f,), dtype=torch.float64, device=dev)
    _call("ts_clean_face_weights", lib.ts_clean_face_weights, v, f, _ptr(vertices), _ptr(faces), _ptr(weights), s)
    # the edge list by (key, weight descending, face): the faces by falling weight (stable: ties by rising face), their
    # three entries each, then a stable sort by key
    by_weight = torch.sort(weights, descending=True, stable=True).indices
    entries = (by_weight.view(-1, 1) * 3 + torch.arange(3, dtype=torch.int64, device=dev)).view(-1)
    del weights, by_weight
    sorted_keys, place = torch.sort(keys[entries], stable=True)
    order = entries[place]
    del keys, entries, place
    marks = torch.zeros((f,), dtype=torch.uint8, device=dev)
    _call("ts_clean_mark", lib.ts_clean_mark, f, 3 * f, _ptr(sorted_keys), _ptr(order), _ptr(marks), s)
    return marks


def _components(lib, v: int, faces: Tensor, s):
    """``(vertex_labels int32 [V], face_labels int32 [F], labels int32 [C], sizes int64 [C])`` of section 6j, step 2."""
    dev = faces.device
    f = int(faces.shape[0])
    parent = torch.empty((v,), dtype=torch.int32, device=dev)
    vertex_labels = torch.empty((v,), dtype=torch.int32, device=dev)
    _call("ts_clean_components", lib.ts_clean_components, v, f, _ptr(faces), _ptr(parent), _ptr(vertex_labels), s)
    del parent
    face_labels = vertex_labels[faces[:, 0].long()] if f else torch.empty((0,), dtype=torch.int32, device=dev)
    labels, sizes = torch.unique(face_labels, sorted=True, return_counts=True)
    return vertex_labels, face_labels, labels, sizes


def _kept_components(cfg: CleanConfig, sizes: Tensor) -> Tensor:
    """bool [C]: the components (in ascending label order, ``sizes`` their face counts) that section 6j's step 3 keeps."""
    keep = sizes >= int(cfg.min_component_faces)
    if sizes.shape[0]:
        keep &= sizes.double() >= float(cfg.min_component_fraction) * sizes.max().double()
        if cfg.keep_largest is not None:
            ranked = torch.sort(sizes, descending=True, stable=True).indices   # ties: the smaller label first
            among = torch.zeros_like(keep)
            among[ranked[:int(cfg.keep_largest)]] = True
            keep &= among
    return keep


def _clean(lib, vertices: Tensor, faces: Tensor, cfg: CleanConfig, s, info: Optional[dict] = None,
           components: bool = False):
    """``(vertices, faces)``, checked by ``_check``, cleaned as section 6j defines -> ``(vertices, faces, kept)``:
    ``kept`` int64 [V'], the rows of the input's vertices that stay, in order, or None where every vertex stays; the
    inputs themselves where nothing changes.  ``info`` receives ``clean_mesh``'s debug entries; the components' are None
    where ``cfg`` filters none, unless ``components`` asks for them regardless."""
    dev = vertices.device
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    info = info if info is not None else {}
    alive = None                                # bool [F], or None while every face stays
    if f:
        flags = torch.empty((f,), dtype=torch.uint8, device=dev)
        _call("ts_clean_degenerate", lib.ts_clean_degenerate, f, _ptr(faces), _ptr(flags), s)
        if bool(flags.any()):
            alive = flags == 0
        del flags
    current = faces if alive is None else faces[alive].contiguous()
    removed_nonmanifold = 0
    info.update(nonmanifold_edges=0)
    if cfg.manifold_edges:
        marks = _nonmanifold_faces(lib, vertices, current, s, info)
        if marks is not None:
            stay = marks == 0
            removed_nonmanifold = int(current.shape[0]) - int(stay.sum())
            if alive is None:
                alive = stay
            else:
                alive[alive.clone()] = stay
            current = current[stay].contiguous()
    info.update(removed_nonmanifold_faces=removed_nonmanifold)
    if cfg.filters or components:
        _, face_labels, labels, sizes = _components(lib, v, current, s)
        keep = _kept_components(cfg, sizes)
        info.update(components=labels, sizes=sizes, kept_components=labels[keep])
        if not bool(keep.all()):
            of_label = torch.zeros((v,), dtype=torch.bool, device=dev)
            of_label[labels[keep].long()] = True
            stay = of_label[face_labels.long()]
            if alive is None:
                alive = stay
            else:
                alive[alive.clone()] = stay
            current = current[stay].contiguous()
    else:
        info.update(components=None, sizes=None, kept_components=None)
    used = torch.zeros((v,), dtype=torch.bool, device=dev)
    used[current.view(-1).long()] = True
    kept_vertices = int(used.sum())
    info.update(removed_faces=f - int(current.shape[0]), removed_vertices=v - kept_vertices)
    if alive is None and kept_vertices == v:
        return vertices, faces, None
    if kept_vertices == v:
        return vertices, current, None
    renumber = torch.cumsum(used, 0, dtype=torch.int32) - 1
    kept = torch.nonzero(used).view(-1)
    return vertices[kept].contiguous(), renumber[current.view(-1).long()].view(-1, 3).contiguous(), kept


@torch.no_grad()
def clean_mesh(mesh, config: Optional[CleanConfig] = None, return_debug: bool = False):
    """``mesh`` (a ``mesh.TriangleMesh`` on the GPU) cleaned as section 6j defines: a fixed function of (mesh, config).
    Faces with two equal indices go; with ``config.manifold_edges``, at every edge of more than two faces all but the two
    largest (by area, ties by the smaller face index) go; of the connected components of what remains (two vertices are
    connected when a face holds both) those that ``config`` does not keep go; vertices that no remaining face uses go.
    The faces and the vertices that stay keep their order, and ``normals`` and ``colors`` their rows, bit for bit.  A
    mesh that loses nothing is returned as the same object; nothing left gives the empty mesh.

    ``return_debug``: also a dict of ``removed_nonmanifold_faces``, ``nonmanifold_edges`` (edges of more than two faces),
    ``components`` (int32 [C], the labels: each component's smallest vertex index, ascending), ``sizes`` (int64 [C], their
    face counts), ``kept_components`` (the labels that stay), ``removed_faces`` and ``removed_vertices``.  The components
    are then found even where ``config`` filters none."""
    from .mesh import TriangleMesh
    cfg = config if config is not None else CleanConfig()
    vertices, faces, dev = _check(mesh.vertices, mesh.faces)
    v = int(vertices.shape[0])
    for name in ("normals", "colors"):
        rows = getattr(mesh, name)
        if rows is not None and (_need_hip(rows) != dev or rows.dim() != 2 or rows.shape[0] != v):
            raise ValueError(f"{name} must hold one row per vertex, on the vertices' device")
    lib = _lib.load()
    info = {}
    with torch.cuda.device(dev):
        new_vertices, new_faces, kept = _clean(lib, vertices, faces, cfg, _stream(dev), info, components=return_debug)
    if new_vertices is vertices and new_faces is faces:
        out = mesh
    else:
        def rows(t):
            return t if t is None or kept is None else t[kept].contiguous()
        out = TriangleMesh(new_vertices, new_faces, rows(mesh.normals), rows(mesh.colors))
    return (out, info) if return_debug else out


@torch.no_grad()
def mesh_components(mesh):
    """The connected components of ``mesh`` as it is (no face is removed first) -> ``(vertex_labels int32 [V],
    face_labels int32 [F], labels int32 [C], sizes int64 [C])``.  Two vertices are connected when a face holds both, so
    two sheets that touch in one vertex are one component.  A component's label is its smallest vertex index;
    ``vertex_labels[v]`` is the label of ``v``'s component (a vertex in no face: itself), ``face_labels[f]`` that of the
    face's first corner; ``labels`` lists the components that have a face, ascending, and ``sizes`` their face counts."""
    vertices, faces, dev = _check(mesh.vertices, mesh.faces)
    with torch.cuda.device(dev):
        return _components(_lib.load(), int(vertices.shape[0]), faces, _stream(dev))
