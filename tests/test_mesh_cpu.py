"""The iso-surface mesher without a GPU: the per-cell routine of csrc/mesh_cells.h, built for
the host from tests/hostmath/meshcells.cpp, against the independent marching tetrahedra of tests/mesh_oracle.py on
every corner sign pattern; closed, consistently oriented surfaces on random sign fields; the float64 oracle on an
analytic sphere; the C entries' argument checks; ``MeshConfig``; the PLY and OBJ writers."""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_oracle as MO

ROOT = Path(__file__).resolve().parent.parent
I64P, I32P, F32P = (ctypes.POINTER(t) for t in (ctypes.c_int64, ctypes.c_int32, ctypes.c_float))


@pytest.fixture(scope="module")
def meshcells(tmp_path_factory):
    """g++ build of tests/hostmath/meshcells.cpp: the kernel's per-cell header compiled for the host."""
    so = tmp_path_factory.mktemp("meshcells") / "_meshcells.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "meshcells.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.mc_cell.restype = ctypes.c_int
    lib.mc_cell.argtypes = [F32P, ctypes.c_float, I64P, I64P, I32P, I32P]
    lib.mc_cell_count.restype = ctypes.c_int
    lib.mc_cell_count.argtypes = [ctypes.c_uint]
    lib.mc_corner_pos.restype = ctypes.c_float
    lib.mc_corner_pos.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int32]
    lib.mc_block.restype = ctypes.c_int64
    lib.mc_block.argtypes = [ctypes.c_int32] * 3 + [F32P, ctypes.c_float, F32P, ctypes.c_float, ctypes.c_int64, I64P,
                                                   F32P, I64P]
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _block(lib, d, level, lo=(0.0, 0.0, 0.0), h=1.0):
    """mc_block on a corner field [Z,Y,X] -> (keys [T,3], positions [T,3,3], cells [T])."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    nz, ny, nx = (s - 1 for s in d.shape)
    room = 12 * nx * ny * nz
    keys, pos, cells = np.zeros((room, 3), np.int64), np.zeros((room, 3, 3), np.float32), np.zeros(room, np.int64)
    lo = np.asarray(lo, dtype=np.float32)
    t = lib.mc_block(nx, ny, nz, _ptr(d, F32P), level, _ptr(lo, F32P), h, room, _ptr(keys, I64P), _ptr(pos, F32P),
                     _ptr(cells, I64P))
    assert 0 <= t <= room
    return keys[:t], pos[:t], cells[:t]


def test_every_corner_sign_pattern(meshcells):
    """All 256 patterns of one cell: the vertices sit on exactly the cell edges whose ends differ, and the triangles
    are the oracle's as key triples up to rotation (so with the oracle's orientation, taken from positions)."""
    ids = np.array([((c >> 2) * 2 + ((c >> 1) & 1)) * 2 + (c & 1) for c in range(8)], dtype=np.int64) + 1000
    edges = [(a, b) for a in range(8) for b in range(8) if a < b and (a & b) == a]       # the 19 edges of the split
    assert len(edges) == 19
    for pattern in range(256):
        above = [(pattern >> c) & 1 == 1 for c in range(8)]
        d = np.array([0.75 if a else 0.25 for a in above], dtype=np.float32)
        keys, lo, hi = np.zeros((12, 3), np.int64), np.zeros((12, 3), np.int32), np.zeros((12, 3), np.int32)
        n = meshcells.mc_cell(_ptr(d, F32P), 0.5, _ptr(ids, I64P), _ptr(keys, I64P), _ptr(lo, I32P), _ptr(hi, I32P))
        assert n == meshcells.mc_cell_count(pattern) and 0 <= n <= 12
        keys, lo, hi = keys[:n], lo[:n], hi[:n]
        assert np.array_equal(keys, ids[lo] * 8 + (lo ^ hi)) and bool(np.all((lo & hi) == lo)) and bool(np.all(lo < hi))
        want = {int(ids[a]) * 8 + (a ^ b) for a, b in edges if above[a] != above[b]}
        assert set(keys.reshape(-1).tolist()) == want, pattern
        oracle = MO.cell_triangles(above, [int(i) for i in ids])
        assert MO.rotation_set(keys) == MO.rotation_set([[v[0] for v in t] for t in oracle]), pattern
        # every triangle's normal points from the corners above to the corners below (checked on positions here too)
        for t in range(n):
            p = [(MO._bits(int(lo[t, k])) + MO._bits(int(hi[t, k]))) / 2 for k in range(3)]
            nrm = np.cross(p[1] - p[0], p[2] - p[0])
            for k in range(3):
                a, b = int(lo[t, k]), int(hi[t, k])
                down = (MO._bits(b) - MO._bits(a)) * (1.0 if above[a] else -1.0)
                assert np.dot(nrm, down) > 0, (pattern, t)
    # a corner exactly at the level counts as below: the strict comparison of the march
    d = np.full(8, 0.5, dtype=np.float32)
    assert meshcells.mc_cell(_ptr(d, F32P), 0.5, _ptr(ids, I64P), _ptr(keys, I64P), _ptr(lo, I32P), _ptr(hi, I32P)) == 0


def test_random_sign_fields_give_closed_oriented_surfaces(meshcells):
    """4^3 cells, all boundary corners below: every undirected edge of the welded surface is used by exactly two
    triangles, once in each direction; the block's triangles are the oracle's."""
    rng = np.random.default_rng(7)
    total = 0
    for seed in range(300):
        d = np.full((5, 5, 5), 0.2, dtype=np.float32)
        d[1:4, 1:4, 1:4] = rng.random((3, 3, 3), dtype=np.float32)
        keys, pos, cells = _block(meshcells, d, 0.5)
        uniq, faces, _ = MO.weld(keys)
        ok, edges = MO.edge_census(faces)
        assert ok, seed
        total += keys.shape[0]
        # all occurrences of a key carry the same bits
        flat_k, flat_p = keys.reshape(-1), pos.reshape(-1, 3)
        order = np.argsort(flat_k, kind="stable")
        same = flat_k[order][1:] == flat_k[order][:-1]
        assert np.array_equal(flat_p[order][1:][same], flat_p[order][:-1][same])
        if seed < 20:
            o = MO.march(d, 0.5)
            assert MO.rotation_set(keys) == MO.rotation_set(o["keys"])
            assert sorted(set(cells.tolist())) == o["crossed"].tolist()
    assert total > 300 * 20


def _sphere_mesh(resolution, dtype=torch.float64):
    params = MO.sphere_params()
    lo, h, cells = MO.make_grid((-1.03, -0.98, -1.01), (0.97, 1.02, 0.99), resolution)
    positions = MO.corner_positions(lo, h, cells)
    d, _ = MO.corner_densities(params, positions, dtype)
    m = MO.march(d, 0.3, positions)
    uniq, faces, verts = MO.weld(m["keys"], m["pos"])
    return float(h), uniq, faces, verts.astype(np.float64)


def test_oracle_meshes_the_analytic_sphere():
    """d = 0.8 exp(-r^2 / 2 s^2): the level set is the sphere r = s sqrt(2 ln(0.8 / 0.3)).  Closed, Euler
    characteristic 2, outward normals; the radial error falls when h halves (the figures are printed: the GPU test
    computes the same yardstick for its own grid)."""
    r = MO.sphere_radius()
    errs = []
    for res in (16, 32):
        h, uniq, faces, verts = _sphere_mesh(res)
        ok, edges = MO.edge_census(faces)
        assert ok and verts.shape[0] - edges + faces.shape[0] == 2
        v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
        nrm = np.cross(v1 - v0, v2 - v0)
        assert bool(np.all(np.einsum("ij,ij->i", nrm, (v0 + v1 + v2) / 3) > 0))
        vol = MO.enclosed_volume(verts, faces)
        err = float(np.abs(np.linalg.norm(verts, axis=1) - r).max())
        print(f"\nsphere at resolution {res}: h {h:.5f}, {verts.shape[0]} vertices, {faces.shape[0]} faces, radial "
              f"error max {err:.3e}, volume {vol:.6f} (sphere {4 / 3 * math.pi * r ** 3:.6f})")
        assert 0.9 < vol / (4 / 3 * math.pi * r ** 3) <= 1.0           # an inscribed polyhedron, up to the radial error
        errs.append(err)
    assert errs[1] < errs[0] and errs[1] < 0.5 * errs[0]


def test_header_corner_positions_are_the_oracles(meshcells):
    lo, h, cells = MO.make_grid((-1.03, -0.98, 2.3), (0.97, 1.02, 3.1), 37)
    pos = MO.corner_positions(lo, h, cells)
    assert cells[0] == 37 and pos.shape == (cells[2] + 1, cells[1] + 1, 38, 3)
    for a in range(3):
        got = np.array([meshcells.mc_corner_pos(float(lo[a]), float(h), i) for i in range(cells[a] + 1)], np.float32)
        want = np.moveaxis(pos[..., a], 2 - a, 0).reshape(cells[a] + 1, -1)[:, 0]
        assert np.array_equal(got, want)
    from tinysplat_amd.mesh import make_grid
    glo, gh, gcells = make_grid((-1.03, -0.98, 2.3), (0.97, 1.02, 3.1), 37)
    assert list(gcells) == list(cells) and np.float32(gh) == h and np.array_equal(np.float32(glo), lo)


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    bad = -1
    p = ctypes.c_void_p(16)
    grid = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.1)
    cells = (ctypes.c_int32 * 3)(10, 10, 10)
    grids = [(ctypes.c_float * 4)(0.0, float("nan"), 0.0, 0.1), (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0),
             (ctypes.c_float * 4)(0.0, 0.0, 0.0, -1.0), (ctypes.c_float * 4)(float("inf"), 0.0, 0.0, 0.1), None]
    # zero and negative sizes, and corner ids that would overflow int64 (2^21 corners per axis: 2^63 * 8)
    cellss = [(ctypes.c_int32 * 3)(0, 10, 10), (ctypes.c_int32 * 3)(10, -3, 10),
              (ctypes.c_int32 * 3)(2 ** 21, 2 ** 21, 2 ** 21), (ctypes.c_int32 * 3)(2 ** 31 - 1, 1, 1), None]
    too_many = (2 ** 31 - 1) // (729 * 16) + 1

    def each(fn, args, cases):
        for i, v in cases:
            a = list(args)
            a[i] = v
            assert fn(*a) == bad, (fn.__name__, i, v)

    each(lib.ts_mesh_boxes, [20, p, p, p, 3.0, p, None],
         [(0, 0), (0, -1), (4, 0.0), (4, float("inf")), (4, float("nan"))] + [(i, None) for i in (1, 2, 3, 5)])
    each(lib.ts_mesh_mark, [20, p, grid, cells, p, None],
         [(0, 0), (1, None), (4, None)] + [(2, g) for g in grids] + [(3, c) for c in cellss])
    each(lib.ts_mesh_corners, [4, p, grid, cells, p, None],
         [(0, 0), (0, -2), (0, too_many), (1, None), (4, None)] + [(2, g) for g in grids] + [(3, c) for c in cellss])
    each(lib.ts_mesh_density, [20, 4, p, grid, cells, p, p, p, p, None],
         [(0, 15), (1, 0), (1, too_many)] + [(i, None) for i in (2, 5, 6, 7, 8)] + [(3, g) for g in grids]
         + [(4, c) for c in cellss])
    each(lib.ts_mesh_count, [4, p, grid, cells, 0.3, p, p, None],
         [(0, 0), (0, too_many), (4, float("nan")), (4, float("inf"))] + [(i, None) for i in (1, 5, 6)]
         + [(2, g) for g in grids] + [(3, c) for c in cellss])
    each(lib.ts_mesh_emit, [4, p, grid, cells, 0.3, p, p, p, p, None, None],
         [(0, 0), (0, too_many), (4, float("nan"))] + [(i, None) for i in (1, 5, 6, 7, 8)]
         + [(2, g) for g in grids] + [(3, c) for c in cellss])
    for n, bricks in ((15, 4), (20, 0), (20, -1), (20, too_many)):
        assert lib.ts_mesh_chunk_bytes(n, bricks) == bad
    one, two = lib.ts_mesh_chunk_bytes(2000, 10), lib.ts_mesh_chunk_bytes(2000, 20)
    assert 0 < one < two and one >= lib.ts_knn_ws_bytes(2000, 7290, 16) + 7290 * (12 + 128 + 4) + 10 * 20
    assert lib.ts_abi_version() == 9


def test_mesh_config_validation():
    from tinysplat_amd.mesh import MeshConfig, level_floor, make_grid
    c = MeshConfig()
    assert (c.surface_level, c.resolution, c.bounds, c.extent_sigmas, c.sparse, c.normals, c.max_workspace_bytes) == \
        (0.3, 256, None, 3.0, True, True, 256 << 20)
    assert level_floor(3.0) == pytest.approx(16 * math.exp(-4.5)) and 0.177 < level_floor(3.0) < 0.178
    MeshConfig(surface_level=0.18)
    MeshConfig(surface_level=0.01, extent_sigmas=4.0)           # 16 exp(-8) = 0.0054
    nan, inf = float("nan"), float("inf")
    for bad in (dict(surface_level=level_floor(3.0)), dict(surface_level=0.17), dict(surface_level=0.3, extent_sigmas=2.0),
                dict(surface_level=nan), dict(resolution=0), dict(resolution=-4), dict(extent_sigmas=0.0),
                dict(extent_sigmas=inf), dict(max_workspace_bytes=0), dict(bounds=((0, 0, 0), (1, 1, nan))),
                dict(bounds=((0, 0, 0), (1, 0, 1))), dict(bounds=((0, 0, 0), (1, -1, 1))),
                dict(bounds=((0, 0, 0), (inf, 1, 1))), dict(bounds=((0, 0), (1, 1)))):
        with pytest.raises(ValueError):
            MeshConfig(**bad)
    lo, h, cells = make_grid((0, 0, 0), (2, 1, 0.26), 8)
    assert cells == [8, 4, 2] and h == 0.25
    with pytest.raises(ValueError):
        make_grid((0, 0, 0), (1, 1, 1), 0)


def test_the_one_weld_is_the_oracles():
    """``_bricks.weld``, the weld of both extractors, against ``mesh_oracle.weld``: 200 triangles over 50 keys, every
    occurrence with a position of its own (so that the first occurrence shows), and no triangle at all."""
    from tinysplat_amd import _bricks, fusion, mesh
    assert mesh.weld is _bricks.weld and fusion.weld is _bricks.weld
    rng = np.random.default_rng(5)
    pool = rng.choice(2 ** 40, 50, replace=False).astype(np.int64)
    keys = pool[rng.integers(0, 50, (200, 3))]
    pos = rng.standard_normal((200, 3, 3)).astype(np.float32)
    uniq, faces, verts = MO.weld(keys, pos)
    got_v, got_f = _bricks.weld(torch.from_numpy(keys), torch.from_numpy(pos))
    assert got_f.dtype == torch.int32 and got_v.dtype == torch.float32
    assert np.array_equal(got_f.numpy(), faces) and np.array_equal(got_v.numpy(), verts)
    assert bool(np.all(np.diff(uniq) > 0)) and np.array_equal(uniq[got_f.numpy()], keys)      # ascending key order
    first = np.array([np.flatnonzero(keys.reshape(-1) == k)[0] for k in uniq])
    assert np.array_equal(got_v.numpy(), pos.reshape(-1, 3)[first])                          # the first occurrence's
    none_v, none_f = _bricks.weld(torch.empty((0, 3), dtype=torch.int64), torch.empty((0, 3, 3)))
    assert none_v.shape == (0, 3) and none_v.dtype == torch.float32
    assert none_f.shape == (0, 3) and none_f.dtype == torch.int32


@pytest.mark.parametrize("resolution", [21, 37])
def test_brick_grid_is_the_arithmetic_of_its_callers(resolution):
    """``BrickGrid`` against what ``extract_mesh`` and ``fuse_depth_maps`` each derived from ``make_grid`` themselves, on
    cell counts that are no multiple of 8; the flags (a byte per brick) fit a cap of exactly that many bytes."""
    from tinysplat_amd._bricks import BrickGrid
    from tinysplat_amd.mesh import BRICK, BRICK_CORNERS, make_grid
    bounds = ((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2))
    lo, h, cells = make_grid(*bounds, resolution)
    assert (BRICK, BRICK_CORNERS) == (8, 729) and all(c % 8 for c in cells)
    grid = BrickGrid(*bounds, resolution, 1 << 20)
    assert (grid.lo, grid.h, grid.cells, grid.cap) == (lo, h, cells, 1 << 20)
    assert grid.bricks == [math.ceil(c / 8) for c in cells]
    total = grid.bricks[0] * grid.bricks[1] * grid.bricks[2]
    assert grid.total_bricks == total > 1
    assert list(grid.grid_host) == [*lo, h] and isinstance(grid.grid_host, ctypes.c_float * 4)
    assert list(grid.cells_host) == cells and isinstance(grid.cells_host, ctypes.c_int32 * 3)
    assert grid.debug == {"lo": tuple(lo), "h": h, "cells": tuple(cells)}
    BrickGrid(*bounds, resolution, total).check_fits(total, "one brick")
    with pytest.raises(ValueError, match=f"the flags of {total} bricks do not fit max_workspace_bytes = {total - 1}"):
        BrickGrid(*bounds, resolution, total - 1).check_fits(1, "one brick")
    with pytest.raises(ValueError, match=f"max_workspace_bytes = {total} is below the {total + 1} bytes one brick over "
                                         "300 Gaussians needs"):
        BrickGrid(*bounds, resolution, total).check_fits(total + 1, "one brick over 300 Gaussians")
    dense = grid.active_bricks(False, None, "cpu")
    assert dense.dtype == torch.int64 and dense.tolist() == list(range(total))

    def mark(flags):
        assert flags.shape == (total,) and flags.dtype == torch.uint8 and not bool(flags.any())
        flags[[total - 1, 0, 5]] = 1
    assert grid.active_bricks(True, mark, "cpu").tolist() == [0, 5, total - 1]


def test_mesh_refuses_cpu_tensors_and_small_models():
    from tinysplat_amd.mesh import extract_mesh, gaussian_boxes
    from tinysplat_amd.synthetic import make_scene
    model, _ = make_scene(40, 0, 32, 32, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_mesh(model)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gaussian_boxes(model)


def read_mesh_ply(path):
    """What ``export_mesh_ply`` writes -> (vertices, normals, faces) as numpy arrays."""
    blob = Path(path).read_bytes()
    marker = b"end_header\n"
    at = blob.find(marker)
    lines = blob[:at].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert lines[3:9] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    assert lines[10] == "property list uchar int vertex_indices"
    v, f = int(lines[2].split()[2]), int(lines[9].split()[2])
    assert lines[2].split()[:2] == ["element", "vertex"] and lines[9].split()[:2] == ["element", "face"]
    body = at + len(marker)
    rows = np.frombuffer(blob, dtype="<f4", count=v * 6, offset=body).reshape(v, 6)
    faces = np.frombuffer(blob, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=f, offset=body + v * 24)
    assert len(blob) == body + v * 24 + f * 13 and bool(np.all(faces["n"] == 3))
    return rows[:, :3].copy(), rows[:, 3:].copy(), faces["v"].astype(np.int32).reshape(f, 3)


def read_mesh_obj(path):
    v, vn, f = [], [], []
    for ln in Path(path).read_text().splitlines():
        tag, *rest = ln.split()
        if tag == "v":
            v.append([float(x) for x in rest])
        elif tag == "vn":
            vn.append([float(x) for x in rest])
        elif tag == "f":
            pairs = [r.split("//") for r in rest]
            assert all(a == b for a, b in pairs)
            f.append([int(a) - 1 for a, _ in pairs])
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(vn, np.float32).reshape(-1, 3),
            np.asarray(f, np.int32).reshape(-1, 3))


def test_writers_round_trip(tmp_path):
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply
    from tinysplat_amd.mesh import TriangleMesh
    g = torch.Generator().manual_seed(3)
    verts = torch.randn(7, 3, generator=g) * 1e3
    verts[0, 0] = 1.0000001
    nrm = torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=-1)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 0, 3]], dtype=torch.int32)
    mesh = TriangleMesh(verts, faces, nrm)
    for write, read, name in ((export_mesh_ply, read_mesh_ply, "m.ply"), (export_mesh_obj, read_mesh_obj, "m.obj")):
        write(mesh, tmp_path / name)
        v, n, f = read(tmp_path / name)
        assert np.array_equal(v, verts.numpy()) and np.array_equal(n, nrm.numpy()) and np.array_equal(f, faces.numpy())
        write(TriangleMesh(verts, faces, None), tmp_path / ("z" + name))
        assert np.array_equal(read(tmp_path / ("z" + name))[1], np.zeros((7, 3), np.float32))
        write(TriangleMesh(verts[:0], faces[:0], nrm[:0]), tmp_path / ("e" + name))
        v, n, f = read(tmp_path / ("e" + name))
        assert v.shape == (0, 3) and n.shape == (0, 3) and f.shape == (0, 3)
        with pytest.raises(ValueError):
            write(TriangleMesh(verts, faces + 5, nrm), tmp_path / ("b" + name))
