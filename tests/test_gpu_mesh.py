"""The iso-surface mesher on the GPU (tinysplat_amd.mesh, csrc/mesh.hip) against the float64
oracle (tests/mesh_oracle.py): corner positions, neighbour lists, densities, triangles, vertices and normals on a
sheet-and-blob scene; sparse against dense; chunk sizes; the analytic sphere; the grid's edges.

The bars follow section 6f: 4 x the deviation of the oracle's own float32 restatement from its float64 run on the same
values (``E_d`` densities, ``E_v`` vertices, ``E_n`` normals), computed here and printed before they are asserted.
Triangles are compared in cells whose eight corners are all stable (``|d - level| > 1e-4`` in float64); with SEED and
BOUNDS below the oracle leaves out 0 of the 2164 cells its surface crosses at resolution 37 (checked on the CPU)."""
import functools

import numpy as np
import pytest
import torch

import extract_oracle as EO
import mesh_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
LEVEL = 0.3
SEED = 11
BOUNDS = ((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2))


def _model(params, dev=DEV):
    from tinysplat_amd.synthetic import SplatModel
    p = {k: torch.as_tensor(v, dtype=torch.float32).to(dev) for k, v in params.items()}
    n = p["means"].shape[0]
    return SplatModel(p["means"], torch.full((n, 3), 0.5, device=dev), torch.zeros((n, 0, 3), device=dev), p["scales"],
                      p["quats"], p["opacities"], 0, background=torch.zeros(3, device=dev))


@functools.lru_cache(maxsize=None)
def _oracle(resolution, bounds=BOUNDS):
    """The float64 run and its float32 restatement on the dense grid, computed once and left unchanged."""
    params = MO.sheet_scene(SEED)
    lo, h, cells = MO.make_grid(*bounds, resolution)
    positions = MO.corner_positions(lo, h, cells)
    d64, knn = MO.corner_densities(params, positions, torch.float64)
    d32, _ = MO.corner_densities(params, positions, torch.float32)
    m = MO.march(d64, LEVEL, positions)
    return dict(params=params, lo=lo, h=h, cells=cells, positions=positions, d64=d64, d32=d32, knn=knn, march=m)


def _extract(params, **cfg):
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    out = extract_mesh(_model(params), MeshConfig(**cfg), return_debug=True)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return (torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
            and (a.normals is None) == (b.normals is None) and (a.normals is None or torch.equal(a.normals, b.normals)))


def _brick_corner_index(active, cells):
    """[A,729] global corner coordinates of the listed bricks and the mask of corners inside the grid."""
    nb = [-(-c // 8) for c in cells]
    b = np.stack((active % nb[0], (active // nb[0]) % nb[1], active // (nb[0] * nb[1])), -1)
    l = np.arange(729)
    loc = np.stack((l % 9, (l // 9) % 9, l // 81), -1)
    g = b[:, None, :] * 8 + loc[None, :, :]
    inside = np.all(g <= np.asarray(cells)[None, None, :], axis=-1)
    return g, inside


def test_mesh_matches_the_oracle():
    o = _oracle(37)
    params, cells, d64 = o["params"], o["cells"], o["d64"]
    mesh, dbg = _extract(params, resolution=37, bounds=BOUNDS)
    assert dbg["grid"]["cells"] == tuple(cells) and np.float32(dbg["grid"]["h"]) == o["h"]
    assert cells[0] == 37 and any(c % 8 for c in cells)
    active = dbg["active_bricks"].cpu().numpy()
    print(f"\nactive bricks {active.size} of {dbg['total_bricks']}, chunks {dbg['chunks']}, brute-force corner queries "
          f"{int(dbg['knn_fallback'].sum())} of {active.size * 729}")
    assert 0 < active.size < dbg["total_bricks"] and bool(np.all(np.diff(active) > 0))
    g, inside = _brick_corner_index(active, cells)
    assert not inside.all()                                           # corners past the last cell exist
    gi, gj, gk = (np.minimum(g[..., a], cells[a]) for a in range(3))
    # corner positions: the same float32 bits as the oracle's expression (clamped past the last cell)
    assert np.array_equal(dbg["corners"].cpu().numpy(), o["positions"][gk, gj, gi])
    # neighbour lists: the brute force
    assert np.array_equal(dbg["knn"].cpu().numpy().astype(np.int64)[inside], o["knn"][gk, gj, gi][inside])
    dens = dbg["density"].cpu().numpy()
    assert bool(np.all(dens[~inside] == 0.0)) and bool(np.isfinite(dens).all())
    stable = MO.stable_corners(d64, LEVEL)
    sel = inside & stable[gk, gj, gi]
    e_d = float(np.abs(o["d32"].astype(np.float64) - d64)[gk, gj, gi][sel].max())
    err_d = float(np.abs(dens.astype(np.float64) - d64[gk, gj, gi])[sel].max())
    print(f"density: err {err_d:.3e}, E_d {e_d:.3e} (bar {FACTOR * e_d:.3e}) over {int(sel.sum())} corners")
    assert err_d <= FACTOR * e_d
    # every cell the oracle's surface crosses lies in an active brick (the sparsity condition)
    m = o["march"]
    nx, ny, nz = cells
    nb = [-(-c // 8) for c in cells]

    def brick_of(cell):
        i, j, k = cell % nx, (cell // nx) % ny, cell // (nx * ny)
        return ((k // 8) * nb[1] + j // 8) * nb[0] + i // 8
    assert bool(np.isin(brick_of(m["crossed"]), active).all())
    # triangles, in cells whose eight corners are all stable
    ok_cell = MO.cells_all_stable(stable).reshape(-1)
    left_out = int((~ok_cell[m["crossed"]]).sum())
    print(f"cells crossed {m['crossed'].size}, left out (an unstable corner) {left_out}")
    assert left_out <= 0.01 * m["crossed"].size
    keys, cell = dbg["keys"].cpu().numpy(), dbg["cell"].cpu().numpy()
    assert keys.shape == (cell.shape[0], 3)
    mine, theirs = keys[ok_cell[cell]], m["keys"][ok_cell[m["cell"]]]
    assert MO.rotation_set(mine) == MO.rotation_set(theirs) and mine.shape[0] > 1000
    # the welded mesh: vertices in ascending key order, faces the inverse
    uniq, faces, _ = MO.weld(keys)
    assert np.array_equal(mesh.faces.cpu().numpy(), faces.astype(np.int32)) and mesh.vertices.shape == (uniq.size, 3)
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.dtype == torch.float32
    # vertices by key, on the compared cells: float32 restatement (E_v) and the GPU against the float64 oracle
    ends = m["ends"][ok_cell[m["cell"]]].reshape(-1, 2)
    okeys, first = np.unique(theirs.reshape(-1), return_index=True)
    ends = ends[first]
    p64 = MO.interpolate(d64, LEVEL, o["positions"], ends)
    p32 = MO.interpolate(o["d32"], np.float32(LEVEL), o["positions"], ends)
    at = np.searchsorted(uniq, okeys)
    assert np.array_equal(uniq[at], okeys)
    verts = mesh.vertices.cpu().numpy()
    e_v = float(np.abs(p32.astype(np.float64) - p64).max())
    err_v = float(np.abs(verts[at].astype(np.float64) - p64).max())
    print(f"vertices: err {err_v:.3e}, E_v {e_v:.3e} (bar {FACTOR * e_v:.3e}) over {okeys.size} vertices")
    assert err_v <= FACTOR * e_v
    # normals at the GPU's vertices: float32 restatement of the oracle against its float64 evaluation (E_n)
    pts = torch.from_numpy(verts[at])
    p = {k: torch.as_tensor(params[k]) for k in EO.PARAMS}
    nbr = EO.exact_knn(pts, p["means"])
    n32 = EO.normals(pts, nbr, p)
    n64 = EO.normals(pts.double(), nbr, {k: v.double() for k, v in p.items()})
    nrm = mesh.normals.cpu()
    e_n = float((n32.double() - n64).abs().max())
    err_n = float((nrm[at].double() - n64).abs().max())
    print(f"normals: err {err_n:.3e}, E_n {e_n:.3e} (bar {FACTOR * e_n:.3e})")
    assert err_n <= FACTOR * e_n
    nl = nrm.norm(dim=-1)
    assert bool(((nl - 1).abs() < 1e-5).logical_or(nl == 0).all()) and bool(torch.isfinite(mesh.vertices).all())
    # recorded, not asserted: how many non-degenerate faces have a geometric normal opposing -grad d at their vertices
    f = mesh.faces.cpu().long()
    v = mesh.vertices.cpu().double()
    gn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    big = gn.norm(dim=-1) > 1e-3 * float(o["h"]) ** 2
    along = (torch.nn.functional.normalize(gn, dim=-1) * nrm.double()[f].mean(1)).sum(-1)
    print(f"faces whose geometric normal opposes the mean vertex normal: {int((along[big] < 0).sum())} of {int(big.sum())}")


def test_sparse_equals_dense():
    params = MO.sheet_scene(SEED)
    sparse, ds = _extract(params, resolution=24, bounds=BOUNDS)
    dense, dd = _extract(params, resolution=24, bounds=BOUNDS, sparse=False)
    assert 0 < ds["active_bricks"].shape[0] < dd["active_bricks"].shape[0] == dd["total_bricks"]
    assert sparse.faces.shape[0] > 300 and _same(sparse, dense)
    assert torch.equal(ds["keys"], dd["keys"]) and torch.equal(ds["cell"], dd["cell"])


def test_chunking_and_repeat_runs_are_bit_identical():
    from tinysplat_amd import _lib
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    params = MO.sheet_scene(SEED)
    one, d1 = _extract(params, resolution=37, bounds=BOUNDS)
    two, d2 = _extract(params, resolution=37, bounds=BOUNDS)
    a = int(d1["active_bricks"].shape[0])
    cap = int(_lib.load().ts_mesh_chunk_bytes(int(params["means"].shape[0]), -(-a // 5)))
    small, d3 = _extract(params, resolution=37, bounds=BOUNDS, max_workspace_bytes=cap)
    print(f"\n{a} active bricks: chunks {d1['chunks']} and, with a {cap} byte cap, {d3['chunks']}")
    assert d1["chunks"] == 1 and d3["chunks"] >= 4
    assert _same(one, two) and _same(one, small)
    for k in ("keys", "cell", "density", "knn", "corners", "active_bricks", "knn_fallback"):
        assert torch.equal(d1[k], d2[k]) and torch.equal(d1[k], d3[k]), k
    # without the debug output the neighbour search runs once per chunk instead of once per brick: the same mesh
    plain = extract_mesh(_model(params), MeshConfig(resolution=37, bounds=BOUNDS))
    assert _same(one, plain)
    bare = extract_mesh(_model(params), MeshConfig(resolution=37, bounds=BOUNDS, normals=False))
    assert bare.normals is None and torch.equal(bare.vertices, one.vertices)
    with pytest.raises(ValueError):
        extract_mesh(_model(params), MeshConfig(resolution=37, bounds=BOUNDS, max_workspace_bytes=1024))
    with pytest.raises(ValueError):                                         # the brick flags alone
        extract_mesh(_model(params), MeshConfig(resolution=4096, bounds=BOUNDS, max_workspace_bytes=1 << 20))
    with pytest.raises(ValueError):                                         # fewer than 16 Gaussians
        extract_mesh(_model({k: v[:15] for k, v in params.items()}), MeshConfig(resolution=8))


def test_default_bounds_are_the_union_of_the_boxes():
    from tinysplat_amd.mesh import gaussian_boxes
    params = MO.sheet_scene(SEED)
    model = _model(params)
    boxes = gaussian_boxes(model, 3.0).cpu().double()
    # sqrt(Sigma_aa) in float64: R diag(exp(2 s)) R^T
    p = {k: torch.as_tensor(params[k]).double() for k in EO.PARAMS}
    R = EO.quat_to_rot(p["quats"])
    half = 3.0 * torch.sqrt(torch.einsum("nac,nc->na", R * R, torch.exp(2 * p["scales"])))
    lo, hi = p["means"] - half, p["means"] + half
    assert bool((boxes[:, :3] <= lo).all()) and bool((boxes[:, 3:] >= hi).all())          # rounded outwards
    assert float((boxes[:, :3] - lo).abs().max()) < 1e-6 and float((boxes[:, 3:] - hi).abs().max()) < 1e-6
    mesh, dbg = _extract(params, resolution=24)
    assert np.allclose(dbg["grid"]["lo"], boxes[:, :3].amin(0).numpy(), atol=1e-6) and max(dbg["grid"]["cells"]) == 24
    assert mesh.faces.shape[0] > 300
    ok, _ = MO.edge_census(mesh.faces.cpu().numpy())
    assert ok                                                               # nothing is cut: the surface is closed


def test_analytic_sphere():
    params = MO.sphere_params()
    r = MO.sphere_radius()
    bounds = ((-1.03, -0.98, -1.01), (0.97, 1.02, 0.99))
    mesh, dbg = _extract(params, resolution=32, bounds=bounds)
    verts, faces = mesh.vertices.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy()
    ok, edges = MO.edge_census(faces)
    assert ok and verts.shape[0] - edges + faces.shape[0] == 2
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    assert bool(np.all(np.einsum("ij,ij->i", np.cross(v1 - v0, v2 - v0), (v0 + v1 + v2) / 3) > 0))
    nrm = mesh.normals.cpu().numpy()
    assert bool(np.all(np.einsum("ij,ij->i", nrm, verts) > 0.99 * np.linalg.norm(verts, axis=1)))
    # the float64 oracle on the same grid, and its float32 restatement for E_v
    lo, h, cells = MO.make_grid(*bounds, 32)
    positions = MO.corner_positions(lo, h, cells)
    d64, _ = MO.corner_densities(params, positions, torch.float64)
    d32, _ = MO.corner_densities(params, positions, torch.float32)
    m = MO.march(d64, LEVEL, positions)
    uniq, ofaces, overts = MO.weld(m["keys"], m["pos"])
    ends = m["ends"].reshape(-1, 2)[np.unique(m["keys"].reshape(-1), return_index=True)[1]]
    e_v = float(np.abs(MO.interpolate(d32, np.float32(LEVEL), positions, ends).astype(np.float64) - overts).max())
    oracle_err = float(np.abs(np.linalg.norm(overts, axis=1) - r).max())
    err = float(np.abs(np.linalg.norm(verts, axis=1) - r).max())
    print(f"\nsphere at resolution 32: {verts.shape[0]} vertices, {faces.shape[0]} faces; radial error {err:.4e}, the "
          f"float64 oracle's {oracle_err:.4e}, E_v {e_v:.3e}; volume {MO.enclosed_volume(verts, faces):.6f}")
    assert err <= oracle_err + FACTOR * e_v
    assert int(dbg["knn_fallback"].sum()) >= 0 and dbg["knn_fallback"].shape == dbg["active_bricks"].shape


def test_grid_edges_cut_the_mesh():
    from tinysplat_amd.mesh import gaussian_boxes
    params = MO.sheet_scene(SEED)
    lo, hi = (-0.52, -0.47, 2.05), (0.61, 0.58, 3.3)
    boxes = gaussian_boxes(_model(params), 3.0).cpu().numpy()
    outside = np.any((boxes[:, 3:] < np.float32(lo)) | (boxes[:, :3] > np.float32(hi)), axis=1)
    within = np.all((boxes[:, :3] > np.float32(lo)) & (boxes[:, 3:] < np.float32(hi)), axis=1)
    assert outside.any() and (~outside & ~within).any()             # wholly outside, and straddling
    mesh, dbg = _extract(params, resolution=21, bounds=(lo, hi))
    nx, ny, nz = dbg["grid"]["cells"]
    v = mesh.vertices.shape[0]
    assert v > 100 and int(mesh.faces.max()) < v and int(mesh.faces.min()) >= 0
    keys = dbg["keys"].cpu().numpy().reshape(-1)
    cid, direction = keys >> 3, keys & 7
    i, j, k = cid % (nx + 1), (cid // (nx + 1)) % (ny + 1), cid // ((nx + 1) * (ny + 1))
    assert bool(np.all((direction >= 1) & (cid >= 0)))
    assert bool(np.all(i + (direction & 1) <= nx) and np.all(j + ((direction >> 1) & 1) <= ny)
                and np.all(k + (direction >> 2) <= nz))
    cell = dbg["cell"].cpu().numpy()
    assert bool(np.all((cell >= 0) & (cell < nx * ny * nz)))
    lo32, h = np.float32(dbg["grid"]["lo"]), np.float32(dbg["grid"]["h"])
    top = lo32 + np.float32([nx, ny, nz]) * h
    verts = mesh.vertices.cpu().numpy()
    assert bool(np.all(verts >= lo32 - 1e-6) and np.all(verts <= top + 1e-6))
    ok, _ = MO.edge_census(mesh.faces.cpu().numpy())
    assert not ok                                                   # cut at the boundary: open edges
    # and the same triangles as the oracle's on that grid, where stable
    o = _oracle(21, (lo, hi))
    ok_cell = MO.cells_all_stable(MO.stable_corners(o["d64"], LEVEL)).reshape(-1)
    m = o["march"]
    assert MO.rotation_set(dbg["keys"].cpu().numpy()[ok_cell[cell]]) == MO.rotation_set(m["keys"][ok_cell[m["cell"]]])


def test_a_faint_model_gives_an_empty_mesh_and_launches_no_mesher():
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    from tinysplat_amd.ops import kernel_timer
    params = MO.sheet_scene(SEED)
    params["opacities"] = np.full_like(params["opacities"], np.log(0.01 / 0.99))
    kernel_timer.start()
    try:
        mesh = extract_mesh(_model(params), MeshConfig(resolution=16, bounds=BOUNDS))
    finally:
        parts = kernel_timer.stop()
    assert "ts_mesh_density" in parts and "ts_mesh_count" not in parts and "ts_mesh_emit" not in parts
    assert mesh.vertices.shape == (0, 3) and mesh.vertices.dtype == torch.float32 and mesh.vertices.is_cuda
    assert mesh.faces.shape == (0, 3) and mesh.faces.dtype == torch.int32
    assert mesh.normals.shape == (0, 3) and mesh.normals.dtype == torch.float32


def test_ply_of_a_gpu_mesh_reads_back(tmp_path):
    from test_mesh_cpu import read_mesh_obj, read_mesh_ply
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply
    mesh, _ = _extract(MO.sheet_scene(SEED), resolution=16, bounds=BOUNDS)
    assert mesh.vertices.is_cuda and mesh.faces.shape[0] > 100
    for write, read, name in ((export_mesh_ply, read_mesh_ply, "m.ply"), (export_mesh_obj, read_mesh_obj, "m.obj")):
        write(mesh, tmp_path / name)
        v, n, f = read(tmp_path / name)
        assert np.array_equal(v, mesh.vertices.cpu().numpy()) and np.array_equal(n, mesh.normals.cpu().numpy())
        assert np.array_equal(f, mesh.faces.cpu().numpy())


def test_mesh_and_march_evaluate_one_density():
    """``ts_mesh_density`` and ``ts_extract_march`` are handed the same positions, neighbour lists and records: their
    densities are equal bit for bit (one ``density_at``, csrc/density_field.h).  One brick of 8 x 8 x 7 cells; the
    float64 oracle gives 648 corners inside the grid, 32 above the level and 51 in (1e-6, 0.3)."""
    from tinysplat_amd import _lib
    from tinysplat_amd.extract import pack_model
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    from tinysplat_amd.ops import _call, _ptr, _stream
    model = _model(MO.sheet_scene(SEED))
    pk = pack_model(model)
    _, dbg = extract_mesh(model, MeshConfig(resolution=8, bounds=BOUNDS), return_debug=True, packed=pk)
    assert dbg["grid"]["cells"] == (8, 8, 7) and dbg["active_bricks"].tolist() == [0]
    # the brick's 729 corners as 243 rays of 3 samples; what the march reads besides is arbitrary and finite
    m, steps = 243, 3
    corners, knn = dbg["corners"].view(m * steps, 3), dbg["knn"].view(m * steps, 16)
    dev = corners.device
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    p_world, dirs, p_std, valid = torch.zeros((m, 3), **f32), torch.zeros((m, 3), **f32), torch.ones((m,), **f32), \
        torch.ones((m,), **i32)
    keep, first, t, points = torch.empty((m,), **i32), torch.empty((m,), **i32), torch.empty((m,), **f32), \
        torch.empty((m, 3), **f32)
    march = torch.empty((m * steps,), **f32)
    with torch.cuda.device(dev):
        _call("ts_extract_march", _lib.load().ts_extract_march, pk.means.shape[0], m, steps, 3.0, LEVEL, _ptr(corners),
              _ptr(knn), _ptr(pk.records), _ptr(p_world), _ptr(dirs), _ptr(p_std), _ptr(valid), _ptr(keep), _ptr(first),
              _ptr(t), _ptr(points), _ptr(march), _stream(dev))
    torch.cuda.synchronize()
    _, inside = _brick_corner_index(np.zeros(1, dtype=np.int64), dbg["grid"]["cells"])
    sel = torch.from_numpy(inside.reshape(-1)).to(dev)
    mesh_d, march_d = dbg["density"].view(-1)[sel], march[sel]
    above, below = int((mesh_d > LEVEL).sum()), int(((mesh_d > 1e-6) & (mesh_d < LEVEL)).sum())
    print(f"\n{int(sel.sum())} corners compared, {above} above the level, {below} in (1e-6, level)")
    assert int(sel.sum()) >= 600 and above >= 20 and below >= 20
    assert torch.equal(march_d, mesh_d)


def _record_entries(monkeypatch):
    """-> the list that receives, in order, the name of every C-ABI entry ``_lib.check`` is handed a status of."""
    from tinysplat_amd import _lib
    names, check = [], _lib.check

    def spy(code, what):
        names.append(what)
        check(code, what)
    monkeypatch.setattr(_lib, "check", spy)
    return names


def test_the_launches_of_a_chunked_run_in_order(monkeypatch):
    """What ``extract_mesh`` launches, entry by entry, with a cap that takes at least 3 chunks: the model's records, the
    boxes, the marking; per chunk the corners, one neighbour search, the densities and - where a corner is above the
    level - the count, and the emit where the count is not zero; then the normals per chunk of vertices.  Which chunks
    count and emit follows from the densities and the triangles' cells of an uncapped run."""
    from tinysplat_amd import _lib
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    params = MO.sheet_scene(SEED)
    n = int(params["means"].shape[0])
    whole, d0 = _extract(params, resolution=16, bounds=BOUNDS)
    a = int(d0["active_bricks"].shape[0])
    per = a // 3
    assert n == 300 and per >= 1 and d0["chunks"] == 1
    cap = int(_lib.load().ts_mesh_chunk_bytes(n, per))
    # the triangles of each active brick, from their cells: cell = (k ny + j) nx + i, brick = (bz nby + by) nbx + bx
    nx, ny, _ = d0["grid"]["cells"]
    nbx, nby = -(-nx // 8), -(-ny // 8)
    cell = d0["cell"].cpu().numpy()
    brick = (cell // (nx * ny) // 8 * nby + cell // nx % ny // 8) * nbx + cell % nx // 8
    active = d0["active_bricks"].cpu().numpy()
    assert bool(np.isin(brick, active).all())
    tris = np.bincount(np.searchsorted(active, brick), minlength=a)
    above = (d0["density"] > LEVEL).any(1).cpu().numpy()
    want = ["ts_extract_pack", "ts_mesh_boxes", "ts_mesh_mark"]
    groups = 0
    for b0 in range(0, a, per):
        want += ["ts_mesh_corners", "ts_knn", "ts_mesh_density"]
        if above[b0:b0 + per].any():
            want.append("ts_mesh_count")
            if tris[b0:b0 + per].sum():
                want.append("ts_mesh_emit")
        groups += 1
    assert groups >= 3 and "ts_mesh_emit" in want
    names = _record_entries(monkeypatch)
    mesh = extract_mesh(_model(params), MeshConfig(resolution=16, bounds=BOUNDS, max_workspace_bytes=cap))
    monkeypatch.undo()
    torch.cuda.synchronize()
    got, normals = names[:len(want)], names[len(want):]
    assert got == want
    assert len(normals) >= 2 and normals == ["ts_knn", "ts_extract_normals"] * (len(normals) // 2)
    _, d1 = _extract(params, resolution=16, bounds=BOUNDS, max_workspace_bytes=cap)
    assert d1["chunks"] == groups and _same(mesh, whole)


def test_the_observed_cell_kernel_marches_the_density_as_the_plain_one():
    """The shared driver (``_bricks.march``) over the density mesher's own field, which holds no NaN: with
    ``observed=True`` (the fusion's cell kernel) it emits the keys and positions it emits with ``observed=False``, the
    ones ``extract_mesh`` returned."""
    from types import SimpleNamespace
    from tinysplat_amd import _bricks, _lib
    from tinysplat_amd.ops import _stream
    _, dbg = _extract(MO.sheet_scene(SEED), resolution=16, bounds=BOUNDS)
    density, active = dbg["density"].contiguous(), dbg["active_bricks"]
    a = int(active.shape[0])
    assert a > 1 and not bool(torch.isnan(density).any())
    grid = _bricks.BrickGrid(*BOUNDS, 16, 1 << 20)
    assert grid.debug == dbg["grid"]
    per = -(-a // 2)                                                        # two chunks, by a cap in bricks

    def make_chunk(bricks):
        return SimpleNamespace(counts=torch.empty((bricks,), dtype=torch.int32, device=DEV),
                               offsets=torch.empty((bricks,), dtype=torch.int64, device=DEV))

    def fill(ck, ids, b):
        b0 = next(rows)
        assert torch.equal(ids, active[b0:b0 + b])
        return density[b0:b0 + b].view(-1)
    out = {}
    with torch.cuda.device(DEV):
        for observed in (False, True):
            rows = iter(range(0, a, per))
            out[observed] = _bricks.march(_lib.load(), grid, active, lambda b: b, per, make_chunk, fill, LEVEL, observed,
                                          True, _stream(torch.device(DEV)))
    torch.cuda.synchronize()
    (keys, pos, cell, chunks), (okeys, opos, ocell, ochunks) = out[False], out[True]
    assert chunks == ochunks == 2 and keys.shape[0] > 100
    assert torch.equal(keys, dbg["keys"]) and torch.equal(cell, dbg["cell"])
    assert torch.equal(okeys, keys) and torch.equal(opos, pos) and torch.equal(ocell, cell)
