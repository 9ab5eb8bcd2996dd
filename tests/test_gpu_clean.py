"""The mesh clean-up on the GPU (tinysplat_amd.clean, csrc/clean.hip) against the numpy oracle
(tests/clean_oracle.py), run on the GPU's own meshes: the sheet-and-blob scene of tests/test_gpu_simplify.py at
resolution 37, unsimplified and simplified on the GPU to 2000 and 200 faces, and small meshes with known answers
(tests/clean_cases.py).

Every comparison is for equality.  The clean-up is integer work; the one floating-point quantity, a face's weight A2,
is formed by the same IEEE operations in the kernel and in numpy, and only its ranking is used."""
import functools

import numpy as np
import pytest
import torch

import clean_cases as CC
import clean_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = (2000, 200)


def _input():
    from test_gpu_simplify import _input as scene
    return scene()


def _simplified(target):
    from test_gpu_simplify import _simplified as simplified
    return simplified(target)[0]


def _mesh(verts, faces, normals=None, colors=None):
    from tinysplat_amd import TriangleMesh
    up = lambda a, t: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=t)).to(DEV)
    return TriangleMesh(up(verts, np.float32), up(faces, np.int32), up(normals, np.float32), up(colors, np.float32))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same(a, b):
    def eq(x, y):
        return (x is None) == (y is None) and (x is None or torch.equal(x, y))
    return eq(a.vertices, b.vertices) and eq(a.faces, b.faces) and eq(a.normals, b.normals) and eq(a.colors, b.colors)


def _components_equal_the_oracles(verts, faces):
    from tinysplat_amd import mesh_components
    got = mesh_components(_mesh(verts, faces))
    torch.cuda.synchronize()
    want = CO.components(faces, verts.shape[0])
    assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.int32, torch.int64]
    for g, w, what in zip(got, want, ("vertex_labels", "face_labels", "labels", "sizes")):
        assert g.shape == w.shape and np.array_equal(_np(g), w), what
    return want


@functools.lru_cache(maxsize=None)
def _scene_oracle():
    """The oracle's components of the GPU's unsimplified mesh, computed once."""
    _, mesh = _input()
    return CO.components(_np(mesh.faces), mesh.vertices.shape[0])


# ------------------------------------------------------------------------------------------------ components
def test_components_of_the_scene():
    from tinysplat_amd import mesh_components
    _, mesh = _input()
    got = mesh_components(mesh)
    want = _scene_oracle()
    print(f"\nscene: {mesh.faces.shape[0]} faces, components {want[2].tolist()} of {want[3].tolist()} faces")
    assert want[2].size >= 2 and int(want[3].sum()) == mesh.faces.shape[0]
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(_np(g), w)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 1000])
def test_disjoint_tetrahedra(k):
    verts, faces = CC.tetrahedra(k, seed=k)
    vl, fl, labels, sizes = _components_equal_the_oracles(verts, faces)
    assert labels.size == k and sizes.tolist() == [4] * k and np.unique(vl).size == k


@pytest.mark.parametrize("numbering", ["ascending", "descending", "random"])
@pytest.mark.parametrize("f", [1, 63, 64, 65, 255, 256, 257, 20_000])
def test_one_triangle_strip(f, numbering):
    """One component whatever the numbering; descending numbering builds the deepest trees."""
    verts, faces = CC.strip(f, numbering, seed=f)
    vl, fl, labels, sizes = _components_equal_the_oracles(verts, faces)
    assert labels.tolist() == [0] and sizes.tolist() == [f] and not vl.any() and not fl.any()


def test_fan_around_the_largest_index():
    """4096 triangles around the vertex with the largest index: every join contends for one root."""
    verts, faces = CC.fan(4096)
    assert faces[:, 0].min() == verts.shape[0] - 1 == 4097
    vl, fl, labels, sizes = _components_equal_the_oracles(verts, faces)
    assert labels.tolist() == [0] and sizes.tolist() == [4096] and not vl.any()


def test_shuffled_grids_over_every_compute_unit():
    """Three disjoint 250 x 250 height fields, 372 006 faces in random order over randomly numbered vertices: 1454
    workgroups, several to every compute unit of every XCD, joining long chains at once."""
    verts, faces = CC.grids(250, pieces=3, seed=5)
    vl, fl, labels, sizes = _components_equal_the_oracles(verts, faces)
    assert labels.size == 3 and sizes.tolist() == [2 * 249 * 249] * 3
    from tinysplat_amd import mesh_components
    again = mesh_components(_mesh(verts, faces))
    assert np.array_equal(_np(again[0]), vl)


def test_unreferenced_vertices_are_labelled_themselves():
    verts, faces = CC.tetrahedra(65, seed=3)
    at = np.array([0, 0, 17, 130, 260])
    padded = np.insert(verts, at, np.float32(9.0), axis=0)
    shift = np.zeros(verts.shape[0], np.int64)
    for k, a in enumerate(at):
        shift[a:] = k + 1
    moved = (faces + shift[faces]).astype(np.int32)
    vl, fl, labels, sizes = _components_equal_the_oracles(padded, moved)
    alone = np.setdiff1d(np.arange(padded.shape[0]), moved.reshape(-1))
    assert alone.size == 5 and np.array_equal(vl[alone], alone) and labels.size == 65
    assert not np.isin(alone, labels).any()
    # no face at all: every vertex its own label, no component listed
    vl, fl, labels, sizes = _components_equal_the_oracles(verts, np.zeros((0, 3), np.int32))
    assert np.array_equal(vl, np.arange(verts.shape[0])) and labels.size == 0 and sizes.size == 0


# ------------------------------------------------------------------------------------------------ edges
def _clean_equals_the_oracles(verts, faces, **cfg):
    from tinysplat_amd import CleanConfig, clean_mesh
    out, info = clean_mesh(_mesh(verts, faces), CleanConfig(**cfg), return_debug=True)
    torch.cuda.synchronize()
    ov, of, o = CO.clean(verts, faces, **cfg)
    assert out.faces.dtype == torch.int32 and out.vertices.dtype == torch.float32
    assert out.faces.shape == of.shape and np.array_equal(_np(out.faces), of)
    assert out.vertices.shape == ov.shape and np.array_equal(_np(out.vertices), ov)
    assert info["removed_nonmanifold_faces"] == o["removed_nonmanifold_faces"]
    assert info["nonmanifold_edges"] == o["nonmanifold_edges"]
    assert np.array_equal(_np(info["components"]), o["components"]) and np.array_equal(_np(info["sizes"]), o["sizes"])
    assert np.array_equal(_np(info["kept_components"]), o["kept_components"])
    assert info["removed_faces"] == int((~o["face_kept"]).sum())
    assert info["removed_vertices"] == int((~o["vertex_kept"]).sum())
    return out, info, o


@pytest.mark.parametrize("k", [3, 4, 5])
def test_books(k):
    verts, faces, heights = CC.book(k)
    out, info, o = _clean_equals_the_oracles(verts, faces)
    assert np.array_equal(np.flatnonzero(o["face_kept"]), np.sort(np.argsort(-heights)[:2]))
    assert info["removed_nonmanifold_faces"] == k - 2 and info["nonmanifold_edges"] == 1 and out.faces.shape[0] == 2
    verts, faces, _ = CC.book(k, equal=True)                           # a k-way tie: the two lowest face indices stay
    out, info, o = _clean_equals_the_oracles(verts, faces)
    assert np.flatnonzero(o["face_kept"]).tolist() == [0, 1] and out.faces.shape[0] == 2
    assert np.array_equal(_np(out.vertices)[_np(out.faces)], verts[faces[:2]])
    out, info, o = _clean_equals_the_oracles(verts, faces, manifold_edges=False)
    assert out.faces.shape[0] == k and info["removed_faces"] == 0


def test_degenerate_faces_go_and_zero_area_faces_stay():
    v = np.zeros((8, 3), np.float32)
    v[1], v[2], v[3] = (1, 0, 0), (2, 0, 0), (3, 0, 0)
    out, info, o = _clean_equals_the_oracles(v, np.array([[1, 1, 2], [1, 2, 3], [5, 4, 5]], np.int32))
    assert out.faces.tolist() == [[0, 1, 2]] and info["removed_faces"] == 2 and info["removed_vertices"] == 5


@pytest.mark.parametrize("target", TARGETS)
def test_simplified_scene_loses_every_edge_above_valence_two(target):
    from tinysplat_amd import CleanConfig, clean_mesh
    mesh = _simplified(target)
    verts, faces = _np(mesh.vertices), _np(mesh.faces)
    before = CO.valence_histogram(faces, verts.shape[0])
    out, info = clean_mesh(mesh, CleanConfig(), return_debug=True)
    torch.cuda.synchronize()
    ov, of, o = CO.clean(verts, faces)
    after = CO.valence_histogram(_np(out.faces), out.vertices.shape[0])
    print(f"\ntarget {target}: {faces.shape[0]} faces, edge valences {before}; cleaned: {out.faces.shape[0]} faces "
          f"({info['removed_nonmanifold_faces']} removed at {info['nonmanifold_edges']} edges), edge valences {after}")
    assert max(before) > 2 and max(after) <= 2
    assert np.array_equal(_np(out.faces), of) and np.array_equal(_np(out.vertices), ov)
    assert info["removed_nonmanifold_faces"] == o["removed_nonmanifold_faces"] == int((~o["face_kept"]).sum()) > 0
    assert info["nonmanifold_edges"] == o["nonmanifold_edges"] == sum(n for val, n in before.items() if val > 2)
    # order kept; the normals and the colours are the input's rows, bit for bit
    assert np.array_equal(ov[of], verts[faces[o["face_kept"]]])
    assert np.array_equal(_np(out.normals), _np(mesh.normals)[o["vertex_kept"]])
    assert np.array_equal(_np(out.colors), _np(mesh.colors)[o["vertex_kept"]])
    # clean once more: nothing to do, the same object
    assert clean_mesh(out, CleanConfig()) is out


def test_unsimplified_mesh_comes_back_as_the_same_object():
    from tinysplat_amd import CleanConfig, TriangleMesh, clean_mesh
    from tinysplat_amd.ops import kernel_timer
    _, mesh = _input()
    kernel_timer.start()
    try:
        out = clean_mesh(mesh, CleanConfig())
    finally:
        parts = kernel_timer.stop()
    assert out is mesh
    assert sorted(parts) == ["ts_clean_degenerate", "ts_clean_edge_keys"]      # the early exit: no weights, no marks
    assert clean_mesh(mesh) is mesh and clean_mesh(mesh, CleanConfig(min_component_faces=1, keep_largest=99)) is mesh
    # argument errors come before any launch
    bad = mesh.faces.clone()
    bad[5, 1] = mesh.vertices.shape[0]
    with pytest.raises(ValueError):
        clean_mesh(TriangleMesh(mesh.vertices, bad, None))
    bad[5, 1] = -1
    with pytest.raises(ValueError):
        clean_mesh(TriangleMesh(mesh.vertices, bad, None))
    nan = mesh.vertices.clone()
    nan[7, 2] = float("inf")
    with pytest.raises(ValueError):
        clean_mesh(TriangleMesh(nan, mesh.faces, None))
    with pytest.raises(ValueError):
        clean_mesh(TriangleMesh(mesh.vertices, mesh.faces, mesh.normals[:-1]))


# ------------------------------------------------------------------------------------------------ filter and result
def _filters():
    """Configs that each drop some but not all components, from the oracle's sizes of the GPU's mesh."""
    sizes = np.sort(_scene_oracle()[3])[::-1]
    largest, second = int(sizes[0]), int(sizes[1])
    assert second < largest
    return [dict(min_component_faces=second + 1), dict(min_component_fraction=(second + 1) / largest),
            dict(keep_largest=1)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_filter_drops_what_the_oracle_drops(which):
    from tinysplat_amd import CleanConfig, clean_mesh
    _, mesh = _input()
    cfg = _filters()[which]
    verts, faces = _np(mesh.vertices), _np(mesh.faces)
    out, info = clean_mesh(mesh, CleanConfig(manifold_edges=False, **cfg), return_debug=True)
    torch.cuda.synchronize()
    ov, of, o = CO.clean(verts, faces, manifold_edges=False, **cfg)
    labels, sizes = _scene_oracle()[2:]
    print(f"\n{cfg}: kept {o['kept_components'].tolist()} of {labels.tolist()}, {of.shape[0]} of {faces.shape[0]} faces")
    assert o["kept_components"].tolist() == [int(labels[np.argmax(sizes)])]
    assert 0 < of.shape[0] == int(sizes.max()) < faces.shape[0]
    assert np.array_equal(_np(info["kept_components"]), o["kept_components"])
    assert np.array_equal(_np(info["components"]), labels) and np.array_equal(_np(info["sizes"]), sizes)
    assert np.array_equal(_np(out.faces), of) and np.array_equal(_np(out.vertices), ov)
    assert info["removed_faces"] == faces.shape[0] - of.shape[0] and info["removed_nonmanifold_faces"] == 0
    assert info["removed_vertices"] == verts.shape[0] - ov.shape[0] > 0
    # the faces and the vertices that stay keep their order and their bits, and the attributes their rows
    assert np.array_equal(ov[of], verts[faces[o["face_kept"]]]) and np.array_equal(ov, verts[o["vertex_kept"]])
    assert np.array_equal(_np(out.normals), _np(mesh.normals)[o["vertex_kept"]])
    assert np.array_equal(_np(out.colors), _np(mesh.colors)[o["vertex_kept"]])
    # at the threshold itself everything stays
    sizes_desc = np.sort(sizes)[::-1]
    at = [dict(min_component_faces=int(sizes.min())),
          dict(min_component_fraction=float(sizes.min()) / float(sizes.max())),
          dict(keep_largest=int(sizes.size))][which]
    assert clean_mesh(mesh, CleanConfig(manifold_edges=False, **at)) is mesh, sizes_desc
    # a bar nothing meets: the empty mesh of extract_mesh's shapes
    none = clean_mesh(mesh, CleanConfig(min_component_faces=int(sizes.max()) + 1))
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.faces.dtype == torch.int32
    assert none.normals.shape == (0, 3) and none.colors.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ bit identity
def test_bit_identity():
    from tinysplat_amd import CleanConfig, clean_mesh
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    from tinysplat_amd.ops import kernel_timer
    from test_gpu_simplify import BOUNDS
    model, mesh = _input()
    clean = CleanConfig(keep_largest=1)
    small = _simplified(TARGETS[0])
    for m in (mesh, small):
        one, again = clean_mesh(m, clean), clean_mesh(m, clean)
        assert _same(one, again) and one is not m and one.faces.shape[0] < m.faces.shape[0]
    # extract_mesh with a clean-up is extract_mesh followed by clean_mesh: the attributes evaluated at the kept vertices
    # alone are those gathered from an evaluation at all of them
    for target in (None, TARGETS[0]):
        for cfg in (dict(colors=True, color_sh_degree=3), dict()):
            kernel_timer.start()
            try:
                whole = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, target_faces=target, clean=clean,
                                                       **cfg))
            finally:
                parts = kernel_timer.stop()
            assert "ts_clean_components" in parts and "ts_clean_edge_keys" in parts
            assert ("ts_clean_mark" in parts) == (target is not None)
            plain = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, target_faces=target, **cfg))
            two = clean_mesh(plain, clean)
            assert _same(whole, two), (target, cfg)
            assert whole.normals is not None and (whole.colors is None) == ("colors" not in cfg)
            assert 0 < whole.faces.shape[0] < plain.faces.shape[0]
    # without a clean-up: the launches and the mesh of before
    kernel_timer.start()
    try:
        plain, dbg = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, colors=True, color_sh_degree=3),
                                  return_debug=True)
    finally:
        parts = kernel_timer.stop()
    assert not any(name.startswith("ts_clean") for name in parts) and "clean" not in dbg
    assert sorted(parts) == ["ts_extract_normals", "ts_extract_pack", "ts_field_colors", "ts_knn", "ts_mesh_boxes",
                             "ts_mesh_corners", "ts_mesh_count", "ts_mesh_density", "ts_mesh_emit", "ts_mesh_mark"]
    assert _same(plain, mesh)
    # a clean-up that finds nothing to remove: the same mesh from extract_mesh
    idle = extract_mesh(model, MeshConfig(bounds=BOUNDS, resolution=37, colors=True, color_sh_degree=3,
                                          clean=CleanConfig()))
    assert _same(idle, mesh)


def test_writers_round_trip_a_cleaned_coloured_mesh(tmp_path):
    from test_color_cpu import read_colored_ply
    from tinysplat_amd import CleanConfig, clean_mesh
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply
    mesh = clean_mesh(_simplified(TARGETS[0]), CleanConfig(keep_largest=1))
    assert mesh.colors is not None and mesh.normals is not None and mesh.faces.shape[0] > 0
    export_mesh_ply(mesh, tmp_path / "m.ply")
    v, n, c, f = read_colored_ply(tmp_path / "m.ply")
    assert np.array_equal(v, _np(mesh.vertices)) and np.array_equal(n, _np(mesh.normals))
    assert np.array_equal(f, _np(mesh.faces))
    assert np.array_equal(c, np.round(np.clip(_np(mesh.colors), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
    export_mesh_obj(mesh, tmp_path / "m.obj")
    lines = (tmp_path / "m.obj").read_text().splitlines()
    vs = np.asarray([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")], dtype=np.float32)
    assert np.array_equal(vs[:, :3], _np(mesh.vertices))
    assert np.array_equal(vs[:, 3:], _np(mesh.colors.clamp(0, 1)))
    fs = [[int(t.split("/")[0]) for t in ln.split()[1:]] for ln in lines if ln.startswith("f ")]
    assert np.array_equal(np.asarray(fs, dtype=np.int32) - 1, _np(mesh.faces))
