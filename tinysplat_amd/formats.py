"""Checkpoint and PLY formats either side of the render path.

Host-side mirror of the reference's persistence code:

  * ``save_checkpoint`` / ``load_checkpoint`` - scripts/train.py:122-124 writes
    ``torch.save(model.state_dict(), path)``; tinysplat/splatting/model_gaussian.py:92-110
    (``from_state_checkpoint``) reads it back: an ordered dict of the six tensors, SH degree derived
    from ``colors_rest.shape[1]``.  Files written here load in the reference and vice versa.
  * ``export_ply`` - model_gaussian.py:330-361: binary little-endian PLY, one float32 record per
    Gaussian (INRIA 3DGS attribute names).  ``load_ply`` is the inverse (the reference has none; it
    lets trained scenes from any 3DGS tool-chain stand in for the synthetic scene).
  * ``export_splat`` / ``load_splat`` - the 32-byte-per-Gaussian ``.splat`` file of the WebGL viewers (the reference's
    ``export_splat`` raises NotImplementedError): records packed and unpacked by csrc/splatfile.hip, ordered by
    ``splat_order``.

The record interleave / de-interleave runs on the GPU (csrc/formats.hip); the host moves one
contiguous buffer and writes / parses the header.  No CPU fallback: tensors must be on the GPU.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream, deg_from_sh
from .synthetic import SplatModel

FIELDS = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")   # state_dict order


def state_dict(model) -> "OrderedDict[str, Tensor]":
    return OrderedDict((f, getattr(model, f).detach().cpu()) for f in FIELDS)


def save_checkpoint(model, path) -> None:
    """train.py:124."""
    torch.save(state_dict(model), path)


def load_checkpoint(path, device, rasterize_mode: str = "classic") -> SplatModel:
    """train.py:267-270 + model_gaussian.py:92-110.  The file holds the six tensors and nothing else (the reference loads
    it): the rasterize mode of the model is the caller's to give."""
    sd = torch.load(path, map_location="cpu")
    missing = [f for f in FIELDS if f not in sd]
    if missing:
        raise KeyError(f"checkpoint lacks {missing}")
    n = sd["means"].shape[0]
    shapes = {"means": (n, 3), "colors_dc": (n, 3), "scales": (n, 3), "quats": (n, 4), "opacities": (n, 1)}
    for f, shp in shapes.items():
        if tuple(sd[f].shape) != shp:
            raise ValueError(f"{f}: expected {shp}, found {tuple(sd[f].shape)}")
    rest = sd["colors_rest"]
    if rest.dim() != 3 or rest.shape[0] != n or rest.shape[2] != 3:
        raise ValueError("colors_rest must be [N, K-1, 3]")
    degree = deg_from_sh(rest.shape[1] + 1)                   # :106-107: max = active = stored degree
    dev = torch.device(device)
    ps = [sd[f].to(device=dev, dtype=torch.float32).contiguous() for f in
          ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")]
    return SplatModel(*ps, active_sh_degree=degree, background=torch.zeros(3, device=dev), rasterize_mode=rasterize_mode)


def ply_attribute_names(k_rest: int) -> List[str]:
    """model_gaussian.py:332-342."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
            + [f"f_rest_{i}" for i in range(3 * k_rest)] + ["opacity"]
            + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def ply_records(model) -> Tensor:
    """[N, 17 + 3 k_rest] float32 on the device: the record array export_ply writes."""
    ts = [_f32c(getattr(model, f).detach()) for f in
          ("means", "colors_dc", "colors_rest", "opacities", "scales", "quats")]
    dev = _need_hip(*ts)
    n, k_rest = ts[0].shape[0], ts[2].shape[1]
    lib = _lib.load()
    w = int(lib.ts_ply_row_floats(k_rest))
    rows = torch.empty((n, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_ply_pack_rows", lib.ts_ply_pack_rows, n, k_rest, *[_ptr(t) if t.numel() else None for t in ts],
              _ptr(rows), _stream(dev))
    return rows


PLY_MODE_COMMENT = "comment rasterize_mode "      # header line of an antialiased model's file; load_ply honours it


def export_ply(model, path) -> None:
    rows = ply_records(model).cpu().numpy()
    k_rest = getattr(model, "colors_rest").shape[1]
    head = ["ply", "format binary_little_endian 1.0"]
    if getattr(model, "rasterize_mode", "classic") == "antialiased":     # (a classic model's file is what it always was)
        head += [PLY_MODE_COMMENT + "antialiased"]
    head += [f"element vertex {rows.shape[0]}"]
    head += [f"property float {a}" for a in ply_attribute_names(k_rest)] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rows.astype("<f4", copy=False).tobytes())


def load_ply(path, device, rasterize_mode: Optional[str] = None) -> SplatModel:
    """Reads a binary little-endian 3DGS PLY whose vertex element holds only float32 properties
    (what export_ply and the INRIA tool-chain write).  The model's rasterize mode is ``rasterize_mode`` if given, else
    the one a ``comment rasterize_mode ...`` header line names, else "classic"."""
    with open(path, "rb") as f:
        blob = f.read()
    marker = b"end_header\n"
    at = blob.find(marker)
    if at < 0 or not blob.startswith(b"ply"):
        raise ValueError("not a PLY file")
    lines = blob[:at].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("only binary_little_endian PLY is supported")
    n, names, mode = None, [], "classic"
    for ln in lines:
        tok = ln.split()
        if ln.startswith(PLY_MODE_COMMENT):
            mode = ln[len(PLY_MODE_COMMENT):].strip()
        elif tok[:2] == ["element", "vertex"]:
            n = int(tok[2])
        elif tok[:1] == ["element"]:
            raise ValueError("unexpected extra PLY element")
        elif tok[:1] == ["property"]:
            if tok[1] not in ("float", "float32"):
                raise ValueError(f"property {tok[-1]} is {tok[1]}; float32 expected")
            names.append(tok[2])
    if n is None:
        raise ValueError("no vertex element")
    n_rest = sum(1 for a in names if a.startswith("f_rest_"))
    if n_rest % 3:
        raise ValueError("f_rest_* count must be a multiple of 3")
    k_rest = n_rest // 3
    if names != ply_attribute_names(k_rest):
        raise ValueError("attribute names / order differ from the 3DGS layout")
    deg_from_sh(k_rest + 1)                                    # raises unless 1, 4, 9, 16, 25 bases
    body = np.frombuffer(blob, dtype="<f4", count=n * len(names), offset=at + len(marker))
    dev = torch.device(device)
    rows = torch.from_numpy(body.reshape(n, len(names)).copy()).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"means": torch.empty((n, 3), **f32), "colors_dc": torch.empty((n, 3), **f32),
           "colors_rest": torch.empty((n, k_rest, 3), **f32), "opacities": torch.empty((n, 1), **f32),
           "scales": torch.empty((n, 3), **f32), "quats": torch.empty((n, 4), **f32)}
    _need_hip(rows)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_ply_unpack_rows", lib.ts_ply_unpack_rows, n, k_rest, _ptr(rows),
              *[_ptr(out[f]) if out[f].numel() else None for f in
                ("means", "colors_dc", "colors_rest", "opacities", "scales", "quats")], _stream(dev))
    return SplatModel(out["means"], out["colors_dc"], out["colors_rest"], out["scales"], out["quats"],
                      out["opacities"], active_sh_degree=deg_from_sh(k_rest + 1),
                      background=torch.zeros(3, device=dev),
                      rasterize_mode=mode if rasterize_mode is None else rasterize_mode)


_POINT_FIELDS = ("x", "y", "z", "nx", "ny", "nz")
_COLOR_FIELDS = ("red", "green", "blue")


def _colors_of(obj, rows: int):
    """``obj.colors`` as float32 [rows,3] on the CPU, or None where the attribute is absent or None."""
    col = getattr(obj, "colors", None)
    if col is None:
        return None
    col = torch.as_tensor(col).detach().to("cpu", torch.float32)
    if col.shape != (rows, 3):
        raise ValueError(f"colors [{rows},3] expected")
    return col


def _color_bytes(col) -> np.ndarray:
    """``round(clamp(c, 0, 1) * 255)`` as uint8 [P,3] (NaN as 0)."""
    return torch.round(torch.nan_to_num(col, nan=0.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8).numpy()


def _vertex_rows(xyz, nrm, col) -> bytes:
    """The vertex element's payload: six floats per vertex and, with colours, three ``uchar`` after them."""
    floats = np.ascontiguousarray(np.concatenate((xyz, nrm), 1).astype("<f4"))
    if col is None:
        return floats.tobytes()
    rows = np.empty((floats.shape[0],), dtype=[("f", "<f4", (6,)), ("c", "u1", (3,))])
    rows["f"], rows["c"] = floats, _color_bytes(col)
    return rows.tobytes()


def export_points_ply(points, path) -> None:
    """An oriented point cloud as a binary little-endian PLY, ``x y z nx ny nz`` (float) per vertex: the input of
    Poisson reconstruction tools.  ``points``: an ``extract.SurfacePoints`` (or anything with ``points`` [P,3] and
    ``normals`` [P,3] or None: zero normals are written then), on any device.  Where it has ``colors`` [P,3] (e.g.
    ``mesh.vertex_colors``'), ``uchar red green blue`` follow as ``round(clamp(c, 0, 1) * 255)``."""
    xyz = torch.as_tensor(points.points).detach().to("cpu", torch.float32)
    nrm = getattr(points, "normals", None)
    nrm = torch.zeros_like(xyz) if nrm is None else torch.as_tensor(nrm).detach().to("cpu", torch.float32)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or nrm.shape != xyz.shape:
        raise ValueError("points [P,3] and normals [P,3] expected")
    col = _colors_of(points, xyz.shape[0])
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}",
              *(f"property float {name}" for name in _POINT_FIELDS),
              *(f"property uchar {name}" for name in (_COLOR_FIELDS if col is not None else ())), "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(_vertex_rows(xyz.numpy(), nrm.numpy(), col))


def read_points_ply(path):
    """The inverse of ``export_points_ply`` -> ``(points float32 [P,3], normals float32 [P,3])`` on the CPU.  Reads
    only what that function writes (six float properties in that order)."""
    with open(path, "rb") as f:
        blob = f.read()
    marker = b"end_header\n"
    at = blob.find(marker)
    if at < 0 or not blob.startswith(b"ply"):
        raise ValueError("not a PLY file")
    lines = [ln.strip() for ln in blob[:at].decode("ascii").split("\n") if ln.strip()]
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("only binary_little_endian PLY is supported")
    elements = [ln.split() for ln in lines if ln.startswith("element")]
    props = [ln.split() for ln in lines if ln.startswith("property")]
    if len(elements) != 1 or elements[0][1] != "vertex" or \
            [tuple(p[1:]) for p in props] != [("float", name) for name in _POINT_FIELDS]:
        raise ValueError("expected one vertex element with float x y z nx ny nz")
    n = int(elements[0][2])
    rows = np.frombuffer(blob, dtype="<f4", count=n * 6, offset=at + len(marker)).reshape(n, 6)
    t = torch.from_numpy(rows.astype(np.float32))
    return t[:, :3].contiguous(), t[:, 3:].contiguous()


def _mesh_arrays(mesh):
    """``(vertices float32 [V,3], normals float32 [V,3] (zeros without), faces int32 [F,3], colors float32 tensor [V,3]
    or None)`` of a ``mesh.TriangleMesh`` (or anything with those attributes) as little-endian arrays on the CPU."""
    xyz = torch.as_tensor(mesh.vertices).detach().to("cpu", torch.float32)
    nrm = getattr(mesh, "normals", None)
    nrm = torch.zeros_like(xyz) if nrm is None else torch.as_tensor(nrm).detach().to("cpu", torch.float32)
    faces = torch.as_tensor(mesh.faces).detach().to("cpu", torch.int32)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or nrm.shape != xyz.shape or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("vertices [V,3], normals [V,3] and faces [F,3] expected")
    if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= xyz.shape[0]):
        raise ValueError("a face refers to a vertex that does not exist")
    return xyz.numpy().astype("<f4"), nrm.numpy().astype("<f4"), faces.numpy().astype("<i4"), _colors_of(mesh, xyz.shape[0])


def export_mesh_ply(mesh, path) -> None:
    """A triangle mesh as a binary little-endian PLY: ``x y z nx ny nz`` (float) per vertex, then per face a
    ``uchar`` count (3) and ``int`` vertex indices.  ``mesh``: a ``mesh.TriangleMesh``, on any device.  With
    ``mesh.colors``, ``uchar red green blue`` follow ``nz`` as ``round(clamp(c, 0, 1) * 255)``."""
    xyz, nrm, faces, col = _mesh_arrays(mesh)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}",
              *(f"property float {name}" for name in _POINT_FIELDS),
              *(f"property uchar {name}" for name in (_COLOR_FIELDS if col is not None else ())),
              f"element face {faces.shape[0]}",
              "property list uchar int vertex_indices", "end_header"]
    rows = np.empty((faces.shape[0],), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rows["n"], rows["v"] = 3, faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(_vertex_rows(xyz, nrm, col))
        f.write(rows.tobytes())


def export_mesh_obj(mesh, path) -> None:
    """A triangle mesh as a Wavefront OBJ: ``v x y z``, ``vn x y z`` and ``f a//a b//b c//c`` with 1-based indices.
    Floats are written with nine significant digits, which a float32 survives.  ``mesh`` on any device.  With
    ``mesh.colors`` the vertex lines are ``v x y z r g b``, the colours as floats in [0, 1]."""
    xyz, nrm, faces, col = _mesh_arrays(mesh)
    with open(path, "w", encoding="ascii") as f:
        if col is None:
            f.writelines("v %.9g %.9g %.9g\n" % tuple(r) for r in xyz.tolist())
        else:
            rgb = torch.nan_to_num(col, nan=0.0).clamp(0.0, 1.0).tolist()
            f.writelines("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % (*r, *c) for r, c in zip(xyz.tolist(), rgb))
        f.writelines("vn %.9g %.9g %.9g\n" % tuple(r) for r in nrm.tolist())
        f.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (faces + 1).tolist())


# ------------------------------------------------------------------------------------------------ .splat
SPLAT_RECORD_BYTES = 32          # TS_SPLAT_RECORD_BYTES of csrc/splat_record.h


def _splat_tensors(model):
    """means, scales, colors_dc, opacities, quats of a model as contiguous float32 on one HIP device (colors_rest is
    not part of the format)."""
    ts = [_f32c(getattr(model, f).detach()) for f in ("means", "scales", "colors_dc", "opacities", "quats")]
    return ts, _need_hip(*ts)


def _order_from_keys(keys: Tensor) -> Tensor:
    """float32 keys [n] -> int64 [n]: descending, ties to the smaller index, NaN last.  One sort of unique int64 values:
    the high word is the key's bits mapped so that unsigned order is descending float order (-0 counted as +0, every
    NaN 0xFFFFFFFF, which no number maps to), the low word the index - so the tie rule needs no stable sort."""
    n = keys.shape[0]
    if n >= 1 << 32:
        raise ValueError("splat_order: more than 2^32 keys")
    bits = (keys + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ascending = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    high = torch.where(torch.isnan(keys), torch.full_like(bits, 0xFFFFFFFF), 0xFFFFFFFF - ascending)
    composed = (high << 32) | torch.arange(n, dtype=torch.int64, device=keys.device)
    # the high word can set bit 63: those values are negative as int64 and would sort first, so the top bit is flipped
    return torch.sort(composed ^ (-1 << 63)).values & 0xFFFFFFFF


def _splat_keys(ts, dev) -> Tensor:
    n = ts[0].shape[0]
    keys = torch.empty((n,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_splat_keys", lib.ts_splat_keys, n, _ptr(ts[1]), _ptr(ts[3]), _ptr(keys), _stream(dev))
    return keys


def splat_order(model):
    """``(keys float32 [n], order int64 [n])``: the importance ``exp(s0 + s1 + s2) sigmoid(opacity)`` of every Gaussian
    (csrc/splatfile.hip) and the order a .splat file lists them in: descending, ties to the smaller index, NaN last."""
    ts, dev = _splat_tensors(model)
    keys = _splat_keys(ts, dev)
    return keys, _order_from_keys(keys)


def splat_records(model, order="importance", limit=None) -> Tensor:
    """uint8 [m, 32] on the device: the records export_splat writes.  ``order``: "importance"
    (``splat_order``) or None (model order); ``limit``: keep the first ``m = min(n, limit)`` records of that order."""
    if order not in ("importance", None):
        raise ValueError('order must be "importance" or None')
    if limit is not None and int(limit) < 0:
        raise ValueError("limit must not be negative")
    ts, dev = _splat_tensors(model)
    n = ts[0].shape[0]
    m = n if limit is None else min(n, int(limit))
    perm = _order_from_keys(_splat_keys(ts, dev))[:m].contiguous() if order == "importance" else None
    records = torch.empty((m, SPLAT_RECORD_BYTES), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_splat_pack", lib.ts_splat_pack, n, m, *[_ptr(t) if t.numel() else None for t in ts],
              _ptr(perm) if perm is not None and m else None, _ptr(records) if m else None, _stream(dev))
    return records


def export_splat(model, path, order="importance", limit=None) -> None:
    """Writes the model as a .splat file: 32 bytes per Gaussian, little-endian, no header, most important first."""
    blob = splat_records(model, order=order, limit=limit).cpu().numpy().tobytes()
    with open(path, "wb") as f:
        f.write(blob)


def load_splat(path, device, rasterize_mode: str = "classic") -> SplatModel:
    """Reads a .splat file as a degree-0 model: colors_rest is [n, 0, 3], quats are not renormalised (projection does),
    opacities are finite (the alpha byte is clamped to 1..254 before the logit).  The format has no place for the
    rasterize mode: it is the caller's to give."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) % SPLAT_RECORD_BYTES:
        raise ValueError(f"a .splat file is a whole number of {SPLAT_RECORD_BYTES}-byte records; found {len(blob)} bytes")
    n = len(blob) // SPLAT_RECORD_BYTES
    dev = torch.device(device)
    records = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).reshape(n, SPLAT_RECORD_BYTES).copy()).to(dev)
    _need_hip(records)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"means": torch.empty((n, 3), **f32), "scales": torch.empty((n, 3), **f32),
           "colors_dc": torch.empty((n, 3), **f32), "opacities": torch.empty((n, 1), **f32),
           "quats": torch.empty((n, 4), **f32)}
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_splat_unpack", lib.ts_splat_unpack, n, _ptr(records) if n else None,
              *[_ptr(t) if n else None for t in out.values()], _stream(dev))
    return SplatModel(out["means"], out["colors_dc"], torch.empty((n, 0, 3), **f32), out["scales"], out["quats"],
                      out["opacities"], active_sh_degree=0, background=torch.zeros(3, device=dev),
                      rasterize_mode=rasterize_mode)
