"""Point-cloud initialisation: ``GaussianModel.from_pcd`` (tinysplat/splatting/model_gaussian.py:66-90).

Every training run of the reference that does not resume from a checkpoint starts from the structure-from-motion
point cloud of its dataset (scripts/train.py:271-274).  ``from_pcd`` turns that cloud into the six parameter
tensors; its costly part, sklearn's ``NearestNeighbors(n_neighbors=4)`` on the CPU, runs here as an exact k-NN
kernel on a hashed uniform grid (csrc/knn.hip), and one more launch writes the six tensors.

``knn_points`` is that search with general queries and k <= 16 (pytorch3d's ``knn_points``, which the reference's
density regulariser and mesh extraction call).  There is no CPU fallback: tensors must be on the GPU.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from .ops import _call, _need_hip, _ptr, _stream, num_sh_bases
from .synthetic import SplatModel

MAX_K = 16                     # TS_KNN_MAX_K


class PointCloud:
    """tinysplat/scene.py:226-239: points sorted by id."""

    def __init__(self, point_ids: Tensor, xyz: Tensor, colors: Tensor, errors: Tensor):
        idxs = torch.argsort(point_ids)
        self.point_ids = point_ids[idxs]
        self.xyz = xyz[idxs]
        self.colors = colors[idxs]
        self.errors = errors[idxs]

    def get_points(self, ids: Tensor):
        indices = torch.searchsorted(self.point_ids, ids)
        return self.xyz[indices], self.colors[indices], self.errors[indices]


def _knn(queries: Tensor, points: Tensor, k: int, stats: bool):
    dev = _need_hip(queries, points)
    if points.dim() != 2 or points.shape[1] != 3 or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError("points [n,3] and queries [m,3] expected")
    if points.dtype != torch.float32 or queries.dtype != torch.float32:
        raise ValueError("points and queries must be float32")
    n, m = points.shape[0], queries.shape[0]
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    if k > n:
        raise ValueError(f"k = {k} > number of points {n}")
    self_search = queries is points
    points = points.contiguous()
    queries = points if self_search else queries.contiguous()
    if not bool(torch.isfinite(points).all()) or not bool(torch.isfinite(queries).all()):
        raise ValueError("points and queries must be finite")
    lib = _lib.load()
    ws = torch.empty(int(lib.ts_knn_ws_bytes(n, m, k)), dtype=torch.uint8, device=dev)
    dist = torch.empty((m, k), dtype=torch.float32, device=dev)
    idx = torch.empty((m, k), dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev) if stats else None
    with torch.cuda.device(dev):
        _call("ts_knn", lib.ts_knn, n, _ptr(points), m, _ptr(queries), k, _ptr(dist), _ptr(idx), _ptr(ws),
              _ptr(st), _stream(dev))
    return dist, idx, st


def knn_points(queries: Tensor, points: Tensor, k: int, return_stats: bool = False):
    """Exact k nearest neighbours -> ``(dists float32 [m,k], idx int64 [m,k])``, each row ascending in
    (distance, index).  Distances are Euclidean, evaluated in double and rounded to float32.  Pass the same
    tensor twice for the self-search (every point finds itself, or a coincident point, at distance 0).
    ``return_stats``: also an int32 [2] tensor {queries that took the brute-force fallback, rings of grid
    cells the longest ring search visited}."""
    dist, idx, st = _knn(queries, points, k, return_stats)
    return (dist, idx.long(), st) if return_stats else (dist, idx.long())


def from_pcd(pcd: PointCloud, sh_degree: int = 3, device="cuda:0", generator=None) -> SplatModel:
    """model_gaussian.py:66-90.  ``means`` = xyz, ``colors_dc`` = RGB2SH(colors / 255), ``colors_rest`` = 0,
    ``scales`` = log of the mean distance to the 3 nearest other points (three times), ``quats`` = the
    reference's ``random_quat_tensor`` with u, v, w drawn by ``torch.rand(n, generator=generator)`` on the CPU
    in that order (the same seed gives the reference's quaternions), ``opacities`` = logit(0.1);
    ``max_sh_degree`` = ``sh_degree`` and ``active_sh_degree`` = 1 (:34-35).

    A point with 3 coincident neighbours gets scale ``-inf``, as in the reference (``np.log(0)``).
    float64 coordinates (what COLMAP gives) are rounded to float32 before the search; the reference searches
    at the input precision, so its scales can differ in the last bits there.  Raises ``ValueError`` for fewer
    than 4 points (sklearn does too) and for non-finite coordinates."""
    xyz = torch.as_tensor(pcd.xyz)
    colors = torch.as_tensor(pcd.colors)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or colors.shape != xyz.shape:
        raise ValueError("pcd.xyz and pcd.colors must be [n,3]")
    n = xyz.shape[0]
    if n < 4:
        raise ValueError(f"from_pcd needs at least 4 points (3 neighbours each), got {n}")
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("pcd.xyz holds non-finite coordinates")
    dev = torch.device(device)
    u = torch.rand(n, generator=generator)
    v = torch.rand(n, generator=generator)
    w = torch.rand(n, generator=generator)
    pts = xyz.to(device=dev, dtype=torch.float32).contiguous()
    _need_hip(pts)
    cols = colors.to(device=dev, dtype=torch.float32).contiguous()
    u, v, w = (t.to(dev) for t in (u, v, w))
    _, idx, _ = _knn(pts, pts, 4, False)
    k_rest = num_sh_bases(sh_degree) - 1
    f32 = dict(dtype=torch.float32, device=dev)
    means, dc = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
    rest, scales = torch.empty((n, k_rest, 3), **f32), torch.empty((n, 3), **f32)
    quats, opac = torch.empty((n, 4), **f32), torch.empty((n, 1), **f32)
    mean_dist = torch.empty(n, **f32)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_init_from_points", lib.ts_init_from_points, n, k_rest, _ptr(pts), _ptr(cols), _ptr(u), _ptr(v),
              _ptr(w), _ptr(idx), _ptr(means), _ptr(dc), _ptr(rest) if k_rest else None, _ptr(scales), _ptr(quats),
              _ptr(opac), _ptr(mean_dist), _stream(dev))
    model = SplatModel(means, dc, rest, scales, quats, opac, active_sh_degree=1, background=torch.zeros(3, device=dev))
    model.max_sh_degree = sh_degree
    model.mean_dist = mean_dist          # float32 mean neighbour distance behind ``scales`` (before the log)
    return model


def read_point_cloud_ply(path) -> PointCloud:
    """Reads the binary little-endian ``x y z [nx ny nz] red green blue`` vertex PLY that SfM tools export
    (float / double coordinates and normals, uchar colours; other vertex properties are skipped).
    ``point_ids`` = arange(n), ``errors`` = zeros."""
    import numpy as np
    with open(path, "rb") as f:
        blob = f.read()
    marker = b"end_header\n"
    at = blob.find(marker)
    if at < 0 or not blob.startswith(b"ply"):
        raise ValueError("not a PLY file")
    lines = [ln.strip() for ln in blob[:at].decode("ascii").split("\n")]
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("only binary_little_endian PLY is supported")
    types = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1",
             "char": "i1", "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
             "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}
    n, fields, in_vertex = None, [], False
    for ln in lines:
        tok = ln.split()
        if tok[:1] == ["element"]:
            if n is None and tok[1] != "vertex":
                raise ValueError("the vertex element must come first")
            in_vertex = n is None                     # later elements (faces, ...) follow the vertices: ignored
            if in_vertex:
                n = int(tok[2])
        elif tok[:1] == ["property"] and in_vertex:
            if tok[1] == "list" or tok[1] not in types:
                raise ValueError(f"unsupported vertex property type {tok[1]}")
            fields.append((tok[2], types[tok[1]]))
    if n is None:
        raise ValueError("no vertex element")
    names = [f[0] for f in fields]
    for need in ("x", "y", "z", "red", "green", "blue"):
        if need not in names:
            raise ValueError(f"vertex property {need} missing")
    rec = np.frombuffer(blob, dtype=np.dtype(fields), count=n, offset=at + len(marker))
    xyz = torch.from_numpy(np.stack([rec["x"], rec["y"], rec["z"]], axis=1).copy())
    colors = torch.from_numpy(np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).copy())
    return PointCloud(torch.arange(n), xyz, colors, torch.zeros(n, dtype=xyz.dtype))
