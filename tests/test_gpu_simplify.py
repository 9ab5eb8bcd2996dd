"""The mesh simplifier on the GPU (tinysplat_amd.simplify, csrc/simplify.hip) against the float64
oracle (tests/simplify_oracle.py), run on the GPU's own input mesh: the sheet-and-blob scene of tests/test_gpu_mesh.py at
resolution 37 with the seeded SH coefficients of tests/test_gpu_color.py, budgets 2000 and 200.

The topology (the resolution the search picks, the clusters, the faces) is exact: it hangs on float32 expressions that
the kernels and numpy round alike, so any difference is a bug.  The positions are compared on *stable* clusters, those
with no eigenvalue ratio within a relative 1e-6 of tau and no coordinate of the unconstrained solution within 1e-9 c of
the cell's wall (in the oracle's float64 run): there both sides solve one problem in double, conditioned at most 1 / tau,
and only the final rounding to float32 can differ, so the bar is one float32 ulp at max(|coordinate|, c).  On the CPU,
with the oracle on its own mesh of this scene, no cluster is unstable at either budget (0 of 929 and 0 of 51); on the
MI355X, on the GPU's own mesh, the same, and every vertex equals the oracle's float32 vertex bit for bit."""
import functools

import numpy as np
import pytest
import torch

import mesh_oracle as MO
import simplify_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = ((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2))
TARGETS = (2000, 200)


def _model():
    from test_gpu_color import _model as colored_model
    return colored_model()


@functools.lru_cache(maxsize=None)
def _input():
    """The GPU's coloured mesh of the scene and its model, computed once and left unchanged."""
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    model = _model()
    mesh = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, colors=True, color_sh_degree=3))
    torch.cuda.synchronize()
    assert 6000 < mesh.vertices.shape[0] < 9000
    return model, mesh


@functools.lru_cache(maxsize=None)
def _simplified(target):
    from tinysplat_amd import SimplifyConfig, simplify_mesh
    model, mesh = _input()
    out = simplify_mesh(mesh, SimplifyConfig(target_faces=target), model=model, color_sh_degree=3, return_debug=True)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(target):
    _, mesh = _input()
    return SO.simplify(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), target=target, parts=True)


def _same(a, b):
    def eq(x, y):
        return (x is None) == (y is None) and (x is None or torch.equal(x, y))
    return eq(a.vertices, b.vertices) and eq(a.faces, b.faces) and eq(a.normals, b.normals) and eq(a.colors, b.colors)


def _run(vertices, faces, info=None, **cfg):
    """``simplify._simplify`` on CPU arrays -> (vertices, faces) as numpy."""
    from tinysplat_amd import SimplifyConfig, _lib, simplify
    from tinysplat_amd.ops import _stream
    v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32)).to(DEV)
    f = torch.as_tensor(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV)
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        ov, of = simplify._simplify(_lib.load(), v, f, SimplifyConfig(**cfg), _stream(dev), info)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), of.cpu().numpy()


@pytest.mark.parametrize("target", TARGETS)
def test_topology_is_the_oracles(target):
    mesh, info = _simplified(target)
    ov, of, o = _oracle(target)
    print(f"\ntarget {target}: r {info['r']} (oracle {o['r']}), probes {info['probes']}, clusters {info['clusters']}, "
          f"{mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces (oracle {ov.shape[0]}, {of.shape[0]})")
    assert info["r"] == o["r"] and info["probes"] == o["probes"] and np.float32(info["cell_size"]) == o["c"]
    assert info["cells"] == tuple(o["cells"].tolist())
    assert np.array_equal(info["keys"].cpu().numpy(), o["keys"])
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.dtype == torch.float32
    assert np.array_equal(mesh.faces.cpu().numpy(), of) and mesh.vertices.shape == ov.shape
    assert 0 < mesh.faces.shape[0] <= target


@pytest.mark.parametrize("target", TARGETS)
def test_positions_on_stable_clusters(target):
    mesh, _ = _simplified(target)
    ov, of, o = _oracle(target)
    got = mesh.vertices.cpu().numpy()
    unstable = SO.unstable(o)
    share = float(unstable.mean())
    c = np.float32(o["c"])
    ulp = np.spacing(np.maximum(np.abs(ov), c))
    dev = np.abs(got.astype(np.float64) - ov.astype(np.float64)) / ulp
    worst_stable = float(dev[~unstable].max())
    print(f"\ntarget {target}: unstable clusters {int(unstable.sum())} of {unstable.size} ({share:.3%}); worst deviation "
          f"in float32 ulps at max(|x|, c): stable clusters {worst_stable:.2f}, all clusters {float(dev.max()):.2f}; "
          f"against the float64 solution {float((np.abs(got - o['x64']) / ulp).max()):.3f} ulp")
    assert share <= 0.01
    assert worst_stable <= 1.0
    # every vertex within its cluster's cell, to one ulp
    wall = o["lo"].astype(np.float64) + o["cell"] * np.float64(c)
    assert bool(((got >= wall - ulp) & (got <= wall + np.float64(c) + ulp)).all())


def test_bit_identity():
    from tinysplat_amd import SimplifyConfig, _lib, simplify_mesh
    from tinysplat_amd.mesh import MeshConfig, TriangleMesh, extract_mesh
    from tinysplat_amd.ops import kernel_timer
    model, mesh = _input()
    target = TARGETS[0]
    one, info = _simplified(target)
    again = simplify_mesh(mesh, SimplifyConfig(target_faces=target), model=model, color_sh_degree=3)
    assert _same(one, again) and one.normals is not None and one.colors is not None
    # the accumulation in one piece per pass (the default cap) and in many: pieces of 50 chunks, and of three (the
    # smallest a cap can ask for), where most clusters that cross a chunk end are finished from recomputed sums
    lib = _lib.load()
    bare = TriangleMesh(mesh.vertices, mesh.faces, None)
    assert info["pieces"] == 2
    chunks = -(-3 * mesh.faces.shape[0] // 128)
    for per in (50, 3):
        small, si = simplify_mesh(bare, SimplifyConfig(target_faces=target, max_workspace_bytes=int(
            lib.ts_simplify_ws_bytes(per))), return_debug=True)
        assert si["pieces"] >= -(-chunks // per) >= 4 and small.normals is None and small.colors is None
        assert torch.equal(small.vertices, one.vertices) and torch.equal(small.faces, one.faces)
    with pytest.raises(ValueError):
        simplify_mesh(bare, SimplifyConfig(target_faces=target, max_workspace_bytes=int(lib.ts_simplify_ws_bytes(1)) - 1))
    # extract_mesh with a budget is extract_mesh followed by simplify_mesh
    for cfg in (dict(colors=True, color_sh_degree=3), dict(), dict(normals=False, colors=True, color_sh_degree=3),
                dict(normals=False)):
        whole = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, target_faces=target, **cfg))
        plain = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, **cfg))
        two = simplify_mesh(plain, SimplifyConfig(target_faces=target), model=model,
                            color_sh_degree=cfg.get("color_sh_degree"))
        assert _same(whole, two), cfg
        assert len(cfg) != 2 or _same(whole, one)
        assert (whole.normals is None) == ("normals" in cfg) and (whole.colors is None) == ("colors" not in cfg)
    # without a budget: the launches and the mesh of before (the welded triangles of the debug keys)
    kernel_timer.start()
    try:
        plain, dbg = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, colors=True, color_sh_degree=3),
                                  return_debug=True)
    finally:
        parts = kernel_timer.stop()
    assert not any(name.startswith("ts_simplify") for name in parts) and "simplify" not in dbg
    assert sorted(parts) == ["ts_extract_normals", "ts_extract_pack", "ts_field_colors", "ts_knn", "ts_mesh_boxes", "ts_mesh_corners",
                             "ts_mesh_count", "ts_mesh_density", "ts_mesh_emit", "ts_mesh_mark"]
    assert _same(plain, mesh)
    uniq, faces, _ = MO.weld(dbg["keys"].cpu().numpy())
    assert np.array_equal(plain.faces.cpu().numpy(), faces.astype(np.int32)) and plain.vertices.shape == (uniq.size, 3)
    # a budget the mesh already meets: the same object from simplify_mesh, the same mesh from extract_mesh
    assert simplify_mesh(mesh, SimplifyConfig(target_faces=mesh.faces.shape[0]), model=model) is mesh
    loose = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, colors=True, color_sh_degree=3,
                                           target_faces=10 ** 6))
    assert _same(loose, mesh)


def test_attributes_are_evaluated_at_the_new_vertices():
    from tinysplat_amd import _field, _lib, vertex_colors
    from tinysplat_amd.mesh import _at_points
    from tinysplat_amd.ops import _stream
    model, _ = _input()
    mesh, _ = _simplified(TARGETS[0])
    v = mesh.vertices.shape[0]
    assert mesh.normals.shape == (v, 3) and mesh.colors.shape == (v, 3)
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        normals, _ = _at_points(_lib.load(), _field.pack_model(model), mesh.vertices, 256 << 20, _stream(dev), True, None)
    assert torch.equal(normals, mesh.normals)
    assert torch.equal(vertex_colors(model, mesh.vertices, mesh.normals, sh_degree=3), mesh.colors)
    assert float((mesh.normals.norm(dim=-1) - 1).abs().max()) < 1e-5 and 0.0 <= float(mesh.colors.min()) \
        and float(mesh.colors.max()) <= 1.0
    # without a model: no attributes
    from tinysplat_amd import SimplifyConfig, simplify_mesh
    bare = simplify_mesh(_input()[1], SimplifyConfig(target_faces=TARGETS[0]))
    assert bare.normals is None and bare.colors is None and torch.equal(bare.vertices, mesh.vertices)


# ------------------------------------------------------------------------------------------------ the entries alone
def _heightfield(n=31, seed=3):
    """A jittered n x n height field: float32 vertices at least 0.06 apart and 2 (n - 1)^2 faces."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    xy = 0.1 * ij + rng.uniform(-0.02, 0.02, ij.shape)
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    verts = np.concatenate((xy, z[:, None]), 1).astype(np.float32)
    at = lambda i, j: i * n + j
    faces = [(at(i, j), at(i + 1, j), at(i, j + 1)) for i in range(n - 1) for j in range(n - 1)] + \
            [(at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)) for i in range(n - 1) for j in range(n - 1)]
    rng.shuffle(faces)
    return verts, np.asarray(faces, dtype=np.int32)


@pytest.mark.parametrize("f", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_count_entry(f):
    """One wave, a wave and one face, one workgroup of four waves, a workgroup and one face, several workgroups."""
    import ctypes
    from tinysplat_amd import _lib
    from tinysplat_amd.ops import _ptr, _stream
    verts, faces = _heightfield()
    faces = faces[:f]
    lo, hi = verts.min(0), verts.max(0)
    c = np.float32(0.13)
    n = SO.cells_per_axis(lo, hi, c)
    k = SO.keys_of(SO.cell_of(verts, lo, c, n), n)[faces]
    want = (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])
    assert f < 10 or 0 < want.sum() < f
    blocks = -(-f // 256)
    dev = torch.device(DEV)
    out = torch.full((blocks + 1,), -7, dtype=torch.int32, device=dev)      # a guard behind the last workgroup
    v_d, f_d = torch.as_tensor(verts).to(dev), torch.as_tensor(faces).to(dev)
    with torch.cuda.device(dev):
        code = _lib.load().ts_simplify_count(verts.shape[0], f, _ptr(v_d), _ptr(f_d), (ctypes.c_float * 4)(*lo.tolist(), c),
                                             (ctypes.c_int32 * 3)(*n.tolist()), _ptr(out), _stream(dev))
    assert code == 0
    got = out.cpu().numpy()
    per_block = np.add.reduceat(want.astype(np.int64), np.arange(0, f, 256))
    assert got[-1] == -7 and np.array_equal(got[:-1], per_block) and int(got[:-1].sum()) == int(want.sum())


def _fan(k, c=0.1):
    """A cone of ``k`` triangles around an apex that is alone in its cell of edge ``c``: the apex's cluster takes exactly
    ``k`` face corners.  The ring lies a unit away, several of its vertices to a cell."""
    ang = 2 * np.pi * np.arange(k) / k
    ring = np.stack((1.0 + np.cos(ang), 1.0 + np.sin(ang), np.full(k, 0.013)), -1)
    apex = np.array([[1.03, 0.98, 0.54]])
    verts = np.concatenate((apex, ring)).astype(np.float32)
    faces = np.stack((np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k), -1).astype(np.int32)
    return verts, faces


@pytest.mark.parametrize("k", [128, 129, 1000])
def test_accumulate_a_cluster_that_spans_chunks(k):
    """The sums of every cluster against the oracle's.  The bar: a sum of at most 1000 terms accumulated in double, in
    any order, is within 1000 x 2^-53 = 1.1e-13 of the exact sum relative to the sum of the terms' magnitudes; two such
    sums differ by at most twice that, and 1e-12 leaves room for the terms' own rounding.  The magnitudes are bounded
    from the sums themselves: |n_i n_j| <= |n|^2 (the trace of A), sum |n_i d| <= sqrt(trace x sum d^2)."""
    verts, faces = _fan(k)
    c = 0.1
    ov, of, o = SO.simplify(verts, faces, cell_size=c, parts=True)
    results = []
    from tinysplat_amd import _lib
    for per in (None, 3):                                               # one piece, and pieces of three chunks
        info = {"want_sums": True}
        cfg = {} if per is None else {"max_workspace_bytes": int(_lib.load().ts_simplify_ws_bytes(per))}
        gv, gf = _run(verts, faces, info, target_faces=None, cell_size=c, **cfg)
        results.append((gv, gf, info["quadrics"].cpu().numpy(), info["vertex_sums"].cpu().numpy()))
        assert per is None or info["pieces"] >= -(-3 * k // (128 * 3))
    gv, gf, quad, vs = results[0]
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    keys = info["cluster_keys"].cpu().numpy()
    n = o["cells"]
    cell = SO.cell_of(verts, o["lo"], o["c"], n)
    okeys, inv = np.unique(SO.keys_of(cell, n), return_inverse=True)
    assert np.array_equal(keys, okeys)
    apex = inv.reshape(-1)[0]
    corners = np.bincount(inv.reshape(-1)[faces.reshape(-1)], minlength=okeys.size)
    assert corners[apex] == k and corners.max() == k and (inv.reshape(-1) == apex).sum() == 1
    want, want_vs = o["all_quad"], o["all_vsum"]
    trace = want[:, 0] + want[:, 3] + want[:, 5]
    scale = np.concatenate((np.repeat(trace[:, None], 6, 1), np.repeat(np.sqrt(trace * want[:, 9])[:, None], 3, 1),
                            want[:, 9:10]), 1)
    rel = np.abs(quad - want) / scale
    print(f"\nfan of {k}: {okeys.size} clusters, worst relative deviation of the quadrics {rel.max():.3e} (the apex's "
          f"{rel[apex].max():.3e}), of the vertex sums {np.abs(vs - want_vs).max():.3e}")
    assert rel.max() <= 1e-12
    assert np.array_equal(vs[:, 3], want_vs[:, 3]) and np.abs(vs[:, :3] - want_vs[:, :3]).max() <= 1e-12 * c * vs[:, 3].max()
    assert np.array_equal(gf, of) and gv.shape == ov.shape


def test_all_vertices_in_one_cell_and_every_vertex_alone():
    verts, faces = _heightfield()
    # one cell holds everything: no face survives, the empty mesh of extract_mesh's shapes
    for cfg in (dict(target_faces=None, cell_size=100.0), dict(target_faces=1)):
        info = {}
        gv, gf = _run(verts, faces, info, **cfg)
        assert gv.shape == (0, 3) and gf.shape == (0, 3) and gv.dtype == np.float32 and gf.dtype == np.int32
        assert info["keys"].shape == (0,) and info["clusters"] == 1
    # an edge below the closest pair over sqrt(3): every vertex is its own cluster
    c = 0.03
    info = {}
    gv, gf = _run(verts, faces, info, target_faces=None, cell_size=c)
    ov, of, o = SO.simplify(verts, faces, cell_size=c, parts=True)
    assert gv.shape == verts.shape and info["clusters"] == verts.shape[0] and np.array_equal(gf, of)
    keys = SO.keys_of(SO.cell_of(verts, o["lo"], o["c"], o["cells"]), o["cells"])
    order = np.argsort(keys)
    assert np.array_equal(info["keys"].cpu().numpy(), keys[order])
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    assert MO.rotation_set(gf) == MO.rotation_set(rank[faces])           # unchanged up to rotation and order
    ulp = np.spacing(np.maximum(np.abs(gv), np.float32(c)))
    wall = o["lo"].astype(np.float64) + o["cell"] * np.float64(o["c"])
    assert bool(((gv >= wall - ulp) & (gv <= wall + np.float64(o["c"]) + ulp)).all())
    moved = np.abs(gv.astype(np.float64) - verts[order]) / ulp
    print(f"\nevery vertex alone: moved by at most {moved.max():.2f} float32 ulps")
    assert moved.max() <= 1.0                                           # all its planes pass through it
    # argument errors come before any launch
    from tinysplat_amd import SimplifyConfig, TriangleMesh, simplify_mesh
    v_d, f_d = torch.as_tensor(verts).to(DEV), torch.as_tensor(faces).to(DEV)
    bad = f_d.clone()
    bad[5, 1] = verts.shape[0]
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v_d, bad, None), SimplifyConfig(target_faces=10))
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v_d, f_d, None), SimplifyConfig(target_faces=None, cell_size=1e-30))
    nan = v_d.clone()
    nan[7, 2] = float("nan")
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(nan, f_d, None), SimplifyConfig(target_faces=10))


def test_unreferenced_vertices_take_no_part():
    """Vertices no face uses, far outside the mesh and inside it: the bounds, the clusters and the means are those of the
    mesh without them."""
    verts, faces = _heightfield()
    extra = np.array([[50.0, -30.0, 9.0], [1.0, 1.0, 0.0], [-7.0, 2.0, 2.0]], dtype=np.float32)
    at = np.array([0, 400, 961])
    padded = np.insert(verts, at, extra, axis=0)
    shift = np.zeros(verts.shape[0], np.int64)
    for k, a in enumerate(at):
        shift[a:] = k + 1
    moved = (faces + shift[faces]).astype(np.int32)
    assert np.array_equal(padded[moved], verts[faces])
    info, ref = {}, {}
    gv, gf = _run(padded, moved, info, target_faces=300)
    rv, rf = _run(verts, faces, ref, target_faces=300)
    ov, of, o = SO.simplify(padded, moved, target=300, parts=True)
    assert info["r"] == ref["r"] == o["r"] and 0 < gf.shape[0] <= 300
    assert np.array_equal(gf, rf) and np.array_equal(gv, rv) and np.array_equal(gf, of)
    assert np.array_equal(info["keys"].cpu().numpy(), o["keys"])


def test_sphere():
    """Section 6g's analytic sphere, about 10 000 faces, to a budget of 1000: a vertex and the surface points it stands
    for share a cell, and its radial error must stay below the cell's half diagonal c sqrt(3) / 2."""
    from test_gpu_mesh import _model as grey_model
    from tinysplat_amd import SimplifyConfig, simplify_mesh
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    r = MO.sphere_radius()
    model = grey_model(MO.sphere_params())
    mesh = extract_mesh(model, MeshConfig(bounds=((-1.03, -0.98, -1.01), (0.97, 1.02, 0.99)), resolution=27))
    out, info = simplify_mesh(mesh, SimplifyConfig(target_faces=1000), model=model, return_debug=True)
    torch.cuda.synchronize()
    assert 9000 < mesh.faces.shape[0] < 11500 and 250 < out.faces.shape[0] <= 1000

    def radial(m):
        return np.abs(np.linalg.norm(m.vertices.cpu().numpy().astype(np.float64), axis=1) - r)
    before, after = radial(mesh), radial(out)
    c = info["cell_size"]
    print(f"\nsphere: {mesh.faces.shape[0]} -> {out.faces.shape[0]} faces, r {info['r']}, c {c:.5f}; radial error max "
          f"{after.max():.4e} mean {after.mean():.4e} (unsimplified max {before.max():.4e} mean {before.mean():.4e}); "
          f"half diagonal {c * 3 ** 0.5 / 2:.4e}")
    assert after.max() < c * 3 ** 0.5 / 2
    nrm = out.normals.cpu().numpy()
    radial_dir = out.vertices.cpu().numpy() / np.linalg.norm(out.vertices.cpu().numpy(), axis=1, keepdims=True)
    assert out.colors is None and float((nrm * radial_dir).sum(-1).min()) > 0.99
    # the faces keep their orientation: the enclosed volume is the sphere's, up to what ~500 flat faces cut off
    vol = MO.enclosed_volume(out.vertices.cpu().numpy(), out.faces.cpu().numpy()) / (4 / 3 * np.pi * r ** 3)
    print(f"volume against the sphere's {vol:.4f}")
    assert 0.9 < vol < 1.05


def test_writers_round_trip_a_simplified_coloured_mesh(tmp_path):
    from test_color_cpu import read_colored_ply
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply
    mesh, _ = _simplified(TARGETS[0])
    export_mesh_ply(mesh, tmp_path / "m.ply")
    v, n, c, f = read_colored_ply(tmp_path / "m.ply")
    assert np.array_equal(v, mesh.vertices.cpu().numpy()) and np.array_equal(n, mesh.normals.cpu().numpy())
    assert np.array_equal(f, mesh.faces.cpu().numpy())
    assert np.array_equal(c, np.round(np.clip(mesh.colors.cpu().numpy(), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
    export_mesh_obj(mesh, tmp_path / "m.obj")
    lines = (tmp_path / "m.obj").read_text().splitlines()
    vs = np.asarray([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")], dtype=np.float32)
    assert np.array_equal(vs[:, :3], mesh.vertices.cpu().numpy())
    assert np.array_equal(vs[:, 3:], mesh.colors.clamp(0, 1).cpu().numpy())
    fs = [[int(t.split("/")[0]) for t in ln.split()[1:]] for ln in lines if ln.startswith("f ")]
    assert np.array_equal(np.asarray(fs, dtype=np.int32) - 1, mesh.faces.cpu().numpy())
