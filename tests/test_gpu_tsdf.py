"""The depth-map fusion on the GPU (tinysplat_amd.fusion, csrc/tsdf.hip and the observed cell kernel of csrc/mesh.hip;
DESIGN.md section 6p) against the float64 oracle (tests/tsdf_oracle.py) on the cases of tests/tsdf_cases.py: the field, the
mesh of the GPU's own field, the invariances bit for bit, the closed sphere, the end-to-end route and the untouched
density mesher.

The field's bar is the oracle's derived per-corner bound (its header: 8 x 2^-24 (A_z + |d|) / trunc per observation, plus
one float32 rounding of F), asserted at the decision-stable corners; the worst |dF| / bound over all corners, unstable ones
included, is printed."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_oracle as MO
import tsdf_cases as TC
import tsdf_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _config(c, **kw):
    from tinysplat_amd import FusionConfig
    base = dict(resolution=c.resolution, bounds=c.bounds, trunc_voxels=c.trunc_voxels, znear=TC.ZNEAR,
                min_observations=c.min_observations)
    base.update(kw)
    return FusionConfig(**base)


def _fuse(name, frustum_cull=True, **kw):
    from tinysplat_amd import fuse_depth_maps
    c = TC.case(name)
    cams, depths = TC.torch_inputs(c, DEV)
    out = fuse_depth_maps(cams, depths, _config(c, **kw), return_debug=True, frustum_cull=frustum_cull)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _default(name):
    """The default run of a case, shared by the tests that only read it."""
    return _fuse(name)


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and a.normals is None and b.normals is None


def _dense_field(dbg, cells):
    """The GPU's field of the listed bricks on the dense corner array (NaN elsewhere), float32 [Z,Y,X]; asserts that a
    corner two bricks hold came out bit-identical in both."""
    active = dbg["active_bricks"].cpu().numpy()
    field = dbg["field"].cpu().numpy()
    g, inside = TO.brick_corner_index(active, cells)
    assert bool(np.isnan(field[~inside]).all())                          # corners beyond the grid's last cell
    sx, sy = cells[0] + 1, cells[1] + 1
    ids = ((g[..., 2] * sy + g[..., 1]) * sx + g[..., 0])[inside]
    bits = field.view(np.uint32)[inside]
    order = np.argsort(ids, kind="stable")
    ids, bits = ids[order], bits[order]
    twin = ids[1:] == ids[:-1]
    assert twin.any() and bool(np.all(bits[1:][twin] == bits[:-1][twin]))
    dense = np.full((cells[2] + 1) * sy * sx, np.nan, dtype=np.float32)
    dense.view(np.uint32)[ids] = bits
    return dense.reshape(cells[2] + 1, sy, sx)


@pytest.mark.parametrize("name", ["plane1", "plane2", "plane7", "plane7_thin", "slab3", "sphere"])
def test_field_matches_the_oracle(name):
    c = TC.case(name)
    mesh, dbg = _default(name)
    assert dbg["grid"]["cells"] == tuple(c.cells) and np.float32(dbg["grid"]["h"]) == c.h
    assert np.float32(dbg["trunc"]) == c.trunc
    active = dbg["active_bricks"].cpu().numpy()
    assert bool(np.all(np.diff(active) > 0)) and 0 < active.size <= dbg["total_bricks"]
    assert bool(np.isin(TC.active_bricks(c), active).all())              # the sparsity condition
    g, inside = TO.brick_corner_index(active, c.cells)
    gi, gj, gk = (np.minimum(g[..., a], c.cells[a]) for a in range(3))
    field = dbg["field"].cpu().numpy().astype(np.float64)
    count = dbg["count"].cpu().numpy()
    assert bool(np.isnan(field[~inside]).all()) and bool((count[~inside] == 0).all())
    stable = inside & ~c.unstable[gk, gj, gi]
    want_f, want_n, bound = c.F[gk, gj, gi], c.count[gk, gj, gi], c.bound[gk, gj, gi]
    assert np.array_equal(count[stable], want_n[stable])
    assert np.array_equal(np.isnan(field[stable]), np.isnan(want_f[stable]))
    known = inside & ~np.isnan(field) & ~np.isnan(want_f)
    ratio = np.abs(field - want_f)[known] / bound[known]
    at_stable = stable[known]
    print(f"\n{name}: {active.size} of {dbg['total_bricks']} bricks, {int(stable.sum())} stable corners of {int(inside.sum())}; "
          f"worst |dF| / bound {ratio[at_stable].max():.3f} at stable corners, {ratio.max():.3f} over all corners "
          f"(largest bound {bound[known].max():.3e})")
    assert int(known.sum()) > 1000 and float(ratio[at_stable].max()) <= 1.0


@pytest.mark.parametrize("name", ["plane7", "slab3", "sphere"])
def test_mesh_is_the_march_of_the_gpus_own_field(name):
    c = TC.case(name)
    mesh, dbg = _default(name)
    dense = _dense_field(dbg, c.cells)
    m = TO.march_observed(dense, c.positions)
    keys, cell = dbg["keys"].cpu().numpy(), dbg["cell"].cpu().numpy()
    assert keys.shape == (cell.shape[0], 3) and keys.shape[0] > 1000
    assert MO.rotation_set(keys) == MO.rotation_set(m["keys"])
    assert np.array_equal(np.sort(cell), np.sort(m["cell"]))
    assert not TO.nan_cells(dense).reshape(-1)[cell].any()               # the NaN rule
    uniq, faces, _ = MO.weld(keys)
    assert np.array_equal(mesh.faces.cpu().numpy(), faces.astype(np.int32)) and mesh.vertices.shape == (uniq.size, 3)
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.dtype == torch.float32 and mesh.colors is None
    # vertices by key: within one float32 ulp (of the edge's larger end) of the float32 interpolation on that field
    okeys, first = np.unique(m["keys"].reshape(-1), return_index=True)
    assert np.array_equal(okeys, uniq)
    ends = m["ends"].reshape(-1, 2)[first]
    p32 = MO.interpolate(dense, np.float32(0), c.positions, ends)
    flat = c.positions.reshape(-1, 3)
    ulp = np.spacing(np.maximum(np.abs(flat[ends[:, 0]]), np.abs(flat[ends[:, 1]])).astype(np.float32))
    verts = mesh.vertices.cpu().numpy()
    off = np.abs(verts.astype(np.float64) - p32.astype(np.float64))
    print(f"\n{name}: {keys.shape[0]} triangles, {uniq.size} vertices, {int((off > 0).sum())} coordinates differ from the "
          f"float32 interpolation, worst {float((off / ulp).max()):.2f} ulp")
    assert bool(np.all(off <= ulp)) and bool(np.isfinite(verts).all())


@pytest.mark.parametrize("name", ["plane7", "narrow2", "slab3"])
def test_invariances_bit_for_bit(name):
    from tinysplat_amd import _lib
    mesh, dbg = _default(name)
    assert mesh.faces.shape[0] > 100
    dense, dense_dbg = _fuse(name, sparse=False)
    assert _same(mesh, dense) and dense_dbg["active_bricks"].shape[0] == dbg["total_bricks"] > dbg["active_bricks"].shape[0]
    uncull, uncull_dbg = _fuse(name, frustum_cull=False)
    assert _same(mesh, uncull)
    assert torch.equal(uncull_dbg["field"].view(torch.int32), dbg["field"].view(torch.int32))
    assert torch.equal(uncull_dbg["count"], dbg["count"])
    one = int(_lib.load().ts_tsdf_chunk_bytes(1))
    small, small_dbg = _fuse(name, max_workspace_bytes=one)
    assert _same(mesh, small) and small_dbg["chunks"] == dbg["active_bricks"].shape[0] > dbg["chunks"] == 1
    single, single_dbg = _fuse(name, camera_batch=1)
    assert _same(mesh, single) and torch.equal(single_dbg["field"].view(torch.int32), dbg["field"].view(torch.int32))
    again, _ = _fuse(name)
    assert _same(mesh, again)


@pytest.mark.parametrize("camera_batch", [1, None])
def test_the_launches_of_one_brick_chunks_in_order(camera_batch, monkeypatch):
    """What ``fuse_depth_maps`` launches, entry by entry, with chunks of one brick: the marking; per brick one integration
    per camera batch, the field and - where a corner is inside - the observed count, and the observed emit where the
    count is not zero; never the plain cell kernel.  Which bricks count and emit follows from the field and the
    triangles' cells of the default run."""
    from tinysplat_amd import _lib, fuse_depth_maps
    name = "plane2"
    c = TC.case(name)
    mesh, dbg = _default(name)
    active = dbg["active_bricks"].cpu().numpy()
    a = active.size
    assert a > 1
    # the triangles of each active brick, from their cells: cell = (k ny + j) nx + i, brick = (bz nby + by) nbx + bx
    nx, ny, _ = dbg["grid"]["cells"]
    nbx, nby = -(-nx // 8), -(-ny // 8)
    cell = dbg["cell"].cpu().numpy()
    brick = (cell // (nx * ny) // 8 * nby + cell // nx % ny // 8) * nbx + cell % nx // 8
    assert bool(np.isin(brick, active).all())
    tris = np.bincount(np.searchsorted(active, brick), minlength=a)
    inside = (dbg["field"] > 0).any(1).cpu().numpy()
    cams, depths = TC.torch_inputs(c, DEV)
    launches = 1 if camera_batch is None else math.ceil(len(cams) / camera_batch)
    want = ["ts_tsdf_mark"]
    for i in range(a):
        want += ["ts_tsdf_integrate"] * launches + ["ts_tsdf_field"]
        if inside[i]:
            want.append("ts_mesh_count_observed")
            if tris[i]:
                want.append("ts_mesh_emit_observed")
    assert len(cams) == 2 and "ts_mesh_emit_observed" in want
    cfg = _config(c, max_workspace_bytes=int(_lib.load().ts_tsdf_chunk_bytes(1)), camera_batch=camera_batch)
    names, check = [], _lib.check

    def spy(code, what):
        names.append(what)
        check(code, what)
    monkeypatch.setattr(_lib, "check", spy)
    small = fuse_depth_maps(cams, depths, cfg)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert names == want and "ts_mesh_count" not in names and "ts_mesh_emit" not in names
    assert _same(small, mesh)


def test_sphere_is_closed():
    c = TC.case("sphere")
    m = TO.march_observed(c.F, c.positions)
    assert MO.edge_census(MO.weld(m["keys"])[1])[0]                      # the oracle's mesh is (chosen on the CPU)
    mesh, _ = _default("sphere")
    closed, edges = MO.edge_census(mesh.faces.cpu().numpy())
    verts = mesh.vertices.cpu().numpy().astype(np.float64)
    r = np.linalg.norm(verts - TC.SPHERE_C, axis=1)
    print(f"\n{mesh.faces.shape[0]} faces, {edges} edges, radius {r.min():.3f} .. {r.max():.3f}")
    assert closed and edges > 10000
    assert MO.enclosed_volume(verts, mesh.faces.cpu().numpy()) > 0      # wound outwards


def _shell_model(n=3000, seed=3):
    """``n`` flat, nearly opaque Gaussians on the sphere of radius 1 around (0, 0, 4)."""
    from tinysplat_amd.synthetic import SplatModel
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    means = d + torch.tensor([0.0, 0.0, 4.0])
    # the rotation that takes the z axis to d: the flat axis along the normal
    z = torch.tensor([0.0, 0.0, 1.0]).expand(n, 3)
    axis = torch.cross(z, d, dim=-1)
    w = 1.0 + (z * d).sum(-1, keepdim=True)
    quats = torch.nn.functional.normalize(torch.cat((w, axis), 1) + 1e-6, dim=-1)
    scales = torch.log(torch.tensor([0.07, 0.07, 0.01])).expand(n, 3).contiguous()
    return SplatModel(means.to(DEV), torch.full((n, 3), 0.5, device=DEV), torch.zeros((n, 0, 3), device=DEV),
                      scales.to(DEV), quats.to(DEV), torch.full((n, 1), 4.0, device=DEV), 0,
                      background=torch.zeros(3, device=DEV))


def test_end_to_end_from_a_model(tmp_path):
    from tinysplat_amd import CleanConfig, FusionConfig, extract_mesh_tsdf, formats, render_depth_alpha
    from tinysplat_amd.synthetic import PinholeCamera
    model = _shell_model()
    cams = [PinholeCamera.look_at_origin_plus_z(64, 48, 60.0, position=p) for p in ((-1.0, 0.0, 0.0), (0.0, 0.0, 0.0),
                                                                                    (1.0, 0.3, 0.0))]
    depth, alpha = render_depth_alpha(model, cams[1])
    assert depth.shape == alpha.shape == (48, 64) and depth.dtype == torch.float32
    hit = alpha >= 0.5
    assert 200 < int(hit.sum()) < 48 * 64 and 2.9 < float(depth[hit].min()) and float(depth[hit].max()) < 4.2
    assert float(alpha.max()) <= 1.0 + 1e-5 and float(alpha.min()) >= 0.0
    cfg = FusionConfig(resolution=40)
    mesh, dbg = extract_mesh_tsdf(model, cams, cfg, DEV, return_debug=True)
    again = extract_mesh_tsdf(model, cams, cfg, DEV)
    torch.cuda.synchronize()
    assert mesh.faces.shape[0] > 500 and bool(torch.isfinite(mesh.vertices).all()) and _same(mesh, again)
    lo = torch.tensor(dbg["grid"]["lo"], device=DEV)
    hi = lo + dbg["grid"]["h"] * torch.tensor(dbg["grid"]["cells"], device=DEV)
    assert bool((mesh.vertices >= lo - 1e-5).all()) and bool((mesh.vertices <= hi + 1e-5).all())
    r = (mesh.vertices - torch.tensor([0.0, 0.0, 4.0], device=DEV)).norm(dim=-1)
    assert 0.8 < float(r.median()) < 1.2                                # the shell's front
    budget = FusionConfig(resolution=40, target_faces=400, clean=CleanConfig())
    small = extract_mesh_tsdf(model, cams, budget, DEV)
    assert 0 < small.faces.shape[0] <= 400 and small.normals is None and bool(torch.isfinite(small.vertices).all())
    path = tmp_path / "fused.ply"
    formats.export_mesh_ply(mesh, path)
    assert path.stat().st_size > 12 * mesh.vertices.shape[0]
    formats.export_mesh_obj(small, tmp_path / "fused.obj")
    # a .splat file's model (degree 0, byte-quantised) goes the same way
    formats.export_splat(model, tmp_path / "shell.splat")
    loaded = extract_mesh_tsdf(formats.load_splat(tmp_path / "shell.splat", DEV), cams, cfg, DEV)
    assert loaded.faces.shape[0] > 500 and bool(torch.isfinite(loaded.vertices).all())


def test_the_density_mesher_is_untouched_by_a_fusion():
    """``extract_mesh`` before and after the fusion module ran its kernels (the two share csrc/mesh.hip's cell kernel):
    identical tensors."""
    from tinysplat_amd import MeshConfig, extract_mesh
    from tinysplat_amd.synthetic import SplatModel
    p = {k: torch.as_tensor(v, dtype=torch.float32).to(DEV) for k, v in MO.sheet_scene(11).items()}
    n = p["means"].shape[0]
    model = SplatModel(p["means"], torch.full((n, 3), 0.5, device=DEV), torch.zeros((n, 0, 3), device=DEV), p["scales"],
                       p["quats"], p["opacities"], 0, background=torch.zeros(3, device=DEV))
    cfg = MeshConfig(resolution=37, bounds=((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2)))
    before, dbg0 = extract_mesh(model, cfg, return_debug=True)
    _fuse("plane2")
    after, dbg1 = extract_mesh(model, cfg, return_debug=True)
    torch.cuda.synchronize()
    assert before.faces.shape[0] > 1000
    assert torch.equal(before.vertices, after.vertices) and torch.equal(before.faces, after.faces)
    assert torch.equal(before.normals, after.normals) and torch.equal(dbg0["keys"], dbg1["keys"])
    # the density's field holds no NaN, so the observed kernel must agree with the plain one on it
    import ctypes
    from tinysplat_amd import _lib
    lib = _lib.load()
    ids, density = dbg0["active_bricks"].contiguous(), dbg0["density"].contiguous()
    grid = (ctypes.c_float * 4)(*dbg0["grid"]["lo"], dbg0["grid"]["h"])
    cells = (ctypes.c_int32 * 3)(*dbg0["grid"]["cells"])
    counts = torch.zeros((2, ids.shape[0]), dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ts_mesh_count(ids.shape[0], ids.data_ptr(), grid, cells, 0.3, density.data_ptr(), counts[0].data_ptr(),
                             stream) == 0
    assert lib.ts_mesh_count_observed(ids.shape[0], ids.data_ptr(), grid, cells, 0.3, density.data_ptr(),
                                      counts[1].data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(counts[0], counts[1]) and int(counts[0].sum()) == dbg0["keys"].shape[0]
