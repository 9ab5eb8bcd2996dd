"""Float64 yardstick of the iso-surface mesher (tinysplat_amd.mesh), plain torch / numpy.

Dense corner densities come from ``extract_oracle.exact_knn`` / ``extract_oracle.density`` on the float32 corner
positions ``lo + (i, j, k) * h``.  The marching tetrahedra here share nothing with csrc/mesh_cells.h but the geometry:
a cell's six tetrahedra are the monotone corner paths over the orders of the axes, a tetrahedron's triangles are
derived from its sign pattern in code, and a triangle is oriented by looking at positions (its normal must point from
the corners above the level to those below).  Vertices are welded by the same edge keys, ``id(lower corner) * 8 +
direction``.  A corner is *stable* when ``|d - level| > DELTA`` in float64, the margin of section 6f."""
import itertools
import math

import numpy as np
import torch

import extract_oracle as EO

DELTA = EO.DELTA
AXES = (1, 2, 4)


def make_grid(lo, hi, resolution):
    """(lo float32 [3], h float32, cells [3]): cubes of edge max(hi - lo) / resolution, ceil((hi_a - lo_a) / h) cells."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    h = np.float32(ext.max() / resolution)
    cells = [max(1, math.ceil(e / ext.max() * resolution - 1e-9)) for e in ext]
    return lo, h, cells


def corner_positions(lo, h, cells):
    """float32 [nz + 1, ny + 1, nx + 1, 3]: the product and the sum rounded to float32 separately."""
    ax = [np.float32(lo[a]) + np.arange(cells[a] + 1, dtype=np.float32) * np.float32(h) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack((x, y, z), -1).astype(np.float32)


def corner_densities(params, positions, dtype=torch.float64):
    """-> (d [Z,Y,X] in ``dtype``, knn [Z,Y,X,16]): every corner over its own exact 16 neighbours."""
    pts = torch.from_numpy(positions.reshape(-1, 3))
    p = {k: torch.as_tensor(params[k]).to(dtype) for k in EO.PARAMS}
    knn = EO.exact_knn(pts, torch.as_tensor(params["means"]))
    d = EO.density(pts.to(dtype), knn, p)[0]
    shape = positions.shape[:3]
    return d.reshape(shape).numpy(), knn.reshape(*shape, EO.K).numpy()


def _tetrahedra():
    return [(0, a, a | b, 7) for a, b, _ in itertools.permutations(AXES)]


def _bits(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def cell_triangles(above, ids):
    """One cell from its sign pattern: ``above[c]`` and ``ids[c]`` of the local corners c = 0..7 (bit 0 x, bit 1 y, bit 2
    z) -> a list of triangles, each three (key, lo corner, hi corner), oriented from above to below."""
    out = []
    for tet in _tetrahedra():
        up = [v for v in tet if above[v]]
        down = [v for v in tet if not above[v]]
        if not up or not down:
            continue
        if len(up) == 1 or len(down) == 1:
            lone, rest = (up[0], down) if len(up) == 1 else (down[0], up)
            loops = [[(lone, r) for r in rest]]
        else:
            (a, b), (c, d) = up, down
            quad = [(a, c), (a, d), (b, d), (b, c)]
            loops = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        towards = sum(_bits(v) for v in down) / len(down) - sum(_bits(v) for v in up) / len(up)
        for tri in loops:
            mid = [(_bits(u) + _bits(v)) / 2 for u, v in tri]
            if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), towards) < 0:
                tri = [tri[0], tri[2], tri[1]]
            out.append([(ids[min(u, v)] * 8 + (u ^ v), min(u, v), max(u, v)) for u, v in tri])
    return out


def march(d, level, positions=None):
    """The mesh of a corner field ``d`` [Z,Y,X] -> dict(keys int64 [T,3], cell int64 [T], ends int64 [T,3,2] (the corner
    ids an edge runs between, lower first), crossed (the ids of the cells with triangles), and with ``positions``
    [Z,Y,X,3]: pos float64 [T,3,3], interpolated from the lower corner to the higher in d's own precision)."""
    d = np.asarray(d)
    nz, ny, nx = (s - 1 for s in d.shape)
    sx, sy = nx + 1, ny + 1
    above = d > level
    mixed = np.zeros((nz, ny, nx), dtype=bool)
    cnt = np.zeros((nz, ny, nx), dtype=np.int32)
    for c in range(8):
        cnt += above[(c >> 2):(c >> 2) + nz, ((c >> 1) & 1):((c >> 1) & 1) + ny, (c & 1):(c & 1) + nx]
    mixed = (cnt > 0) & (cnt < 8)
    keys, cell, ends = [], [], []
    for k, j, i in zip(*np.nonzero(mixed)):
        ids = [int(((k + (c >> 2)) * sy + (j + ((c >> 1) & 1))) * sx + (i + (c & 1))) for c in range(8)]
        ab = [bool(above[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)]) for c in range(8)]
        for tri in cell_triangles(ab, ids):
            keys.append([t[0] for t in tri])
            ends.append([[ids[t[1]], ids[t[2]]] for t in tri])
            cell.append((int(k) * ny + int(j)) * nx + int(i))
    out = {"keys": np.asarray(keys, dtype=np.int64).reshape(-1, 3), "cell": np.asarray(cell, dtype=np.int64),
           "ends": np.asarray(ends, dtype=np.int64).reshape(-1, 3, 2),
           "crossed": np.flatnonzero(mixed.reshape(-1)).astype(np.int64)}
    if positions is not None:
        out["pos"] = interpolate(d, level, positions, out["ends"])
    return out


def interpolate(d, level, positions, ends):
    """p_lo + (level - d_lo) / (d_hi - d_lo) (p_hi - p_lo) per edge [..., 2] of corner ids, in d's precision."""
    d = np.asarray(d)
    flat_d = d.reshape(-1)
    flat_p = np.asarray(positions).reshape(-1, 3).astype(d.dtype)
    lo, hi = ends[..., 0], ends[..., 1]
    t = (d.dtype.type(level) - flat_d[lo]) / (flat_d[hi] - flat_d[lo])
    return flat_p[lo] + t[..., None] * (flat_p[hi] - flat_p[lo])


def weld(keys, pos=None):
    """-> (sorted unique keys, faces [T,3] into them, vertices (the first occurrence's position) or None)."""
    uniq, first, inv = np.unique(keys.reshape(-1), return_index=True, return_inverse=True)
    return uniq, inv.reshape(-1, 3), (None if pos is None else pos.reshape(-1, 3)[first])


def edge_census(faces):
    """The directed edges of the faces -> (every undirected edge is used exactly twice, once in each direction;
    the number of undirected edges)."""
    f = np.asarray(faces, dtype=np.int64)
    if f.size == 0:
        return True, 0
    a = np.concatenate((f[:, 0], f[:, 1], f[:, 2]))
    b = np.concatenate((f[:, 1], f[:, 2], f[:, 0]))
    n = int(f.max()) + 1
    directed = a * n + b
    und, counts = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    ok = bool(np.all(a != b)) and np.unique(directed).size == directed.size and bool(np.all(counts == 2))
    return ok, int(und.size)


def rotation_set(keys):
    """Key triples up to rotation (not reflection), as a sorted list of tuples."""
    out = []
    for t in np.asarray(keys).reshape(-1, 3).tolist():
        r = min(range(3), key=lambda s: t[s])
        out.append((t[r], t[(r + 1) % 3], t[(r + 2) % 3]))
    return sorted(out)


def enclosed_volume(vertices, faces):
    """Divergence theorem: sum of v0 . (v1 x v2) / 6 over outward-wound faces."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def stable_corners(d64, level):
    return np.abs(np.asarray(d64) - level) > DELTA


def cells_all_stable(stable):
    """[Z,Y,X] corner flags -> [nz,ny,nx] cell flags: all eight corners stable."""
    nz, ny, nx = (s - 1 for s in stable.shape)
    ok = np.ones((nz, ny, nx), dtype=bool)
    for c in range(8):
        ok &= stable[(c >> 2):(c >> 2) + nz, ((c >> 1) & 1):((c >> 1) & 1) + ny, (c & 1):(c & 1) + nx]
    return ok


def sphere_params(sigma=0.5, centre=(0.0, 0.0, 0.0), share=0.05):
    """16 coincident isotropic Gaussians with sigmoid(o) = ``share``: d = 16 share exp(-r^2 / 2 sigma^2)."""
    n = 16
    return {"means": np.tile(np.asarray(centre, dtype=np.float32), (n, 1)),
            "scales": np.full((n, 3), math.log(sigma), dtype=np.float32),
            "quats": np.tile(np.asarray([1.0, 0.0, 0.0, 0.0], dtype=np.float32), (n, 1)),
            "opacities": np.full((n, 1), math.log(share / (1 - share)), dtype=np.float32)}


def sphere_radius(sigma=0.5, share=0.05, level=0.3):
    return sigma * math.sqrt(2.0 * math.log(16 * share / level))


def sheet_scene(seed, n=260, blob=40):
    """``n`` Gaussians flattened onto the wavy sheet of tests/golden/make_extract_fixtures.py (a smaller patch) and a
    small blob of ``blob`` more above it."""
    g = torch.Generator().manual_seed(seed)

    def sheet(x, y):
        return 3.0 + 0.1 * torch.sin(2.0 * x) * torch.cos(1.5 * y)
    xy = 1.0 * (2 * torch.rand(n, 2, generator=g) - 1)
    means = torch.cat((xy, sheet(xy[:, 0], xy[:, 1])[:, None] + 0.005 * torch.randn(n, 1, generator=g)), 1)
    scales = torch.log(torch.cat((0.10 + 0.05 * torch.rand(n, 2, generator=g),
                                  0.025 + 0.01 * torch.rand(n, 1, generator=g)), 1))
    quats = torch.cat((torch.ones(n, 1), 0.08 * torch.randn(n, 3, generator=g)), 1)
    opac = 1.5 + 1.0 * torch.randn(n, 1, generator=g)
    b_means = torch.tensor([0.3, -0.2, 2.2]) + 0.05 * torch.randn(blob, 3, generator=g)
    b_scales = torch.log(0.06 + 0.03 * torch.rand(blob, 3, generator=g))
    b_quats = torch.nn.functional.normalize(torch.randn(blob, 4, generator=g), dim=-1)
    b_opac = 0.5 + 0.5 * torch.randn(blob, 1, generator=g)
    return {"means": torch.cat((means, b_means)).numpy(), "scales": torch.cat((scales, b_scales)).numpy(),
            "quats": torch.cat((quats, b_quats)).numpy(), "opacities": torch.cat((opac, b_opac)).numpy()}
