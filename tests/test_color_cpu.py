"""The field colours without a GPU: known answers of the float64 oracle (tests/color_oracle.py)
and its SH basis against ``oracle/gsplat_oracle.py``; ``ts_field_colors``' argument checks through the loaded library;
the new ``MeshConfig`` / ``TriangleMesh`` fields; the PLY and OBJ writers with and without colours."""
import ctypes
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import color_oracle as CO
import mesh_oracle as MO
from oracle import gsplat_oracle as O

C0 = 0.5 * math.sqrt(1.0 / math.pi)
C1 = math.sqrt(3.0 / (4.0 * math.pi))
SEED = 11


def _scene(m=40, seed=3):
    """The sheet scene, ``m`` points near the sheet with their exact neighbours, unit normals and K = 16 coefficients."""
    params = MO.sheet_scene(SEED)
    g = torch.Generator().manual_seed(seed)
    xy = 0.9 * (2 * torch.rand(m, 2, generator=g) - 1)
    pts = torch.cat((xy, 3.0 + 0.1 * torch.sin(2.0 * xy[:, :1]) * torch.cos(1.5 * xy[:, 1:])
                     + 0.03 * torch.randn(m, 1, generator=g)), 1)
    nrm = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=-1)
    dc, rest = CO.coefficients(params["means"].shape[0], 15, seed)
    return params, pts, nrm, CO.exact_knn(pts, params), dc, rest


def test_sh_basis_is_the_reference_oracles():
    g = torch.Generator().manual_seed(0)
    d = torch.nn.functional.normalize(torch.randn(500, 3, generator=g, dtype=torch.float64), dim=-1)
    coeffs = torch.randn(500, 16, 3, generator=g, dtype=torch.float64)
    for deg in range(4):
        nb = (deg + 1) ** 2
        Y = CO.sh_basis(deg, d)
        assert Y.shape == (500, nb)
        mine = (Y[:, :, None] * coeffs[:, :nb]).sum(1)
        theirs = O.spherical_harmonics(deg, 3.7 * d, coeffs)                # it normalises its directions
        assert float((mine - theirs).abs().max()) < 1e-14
    with pytest.raises(ValueError):
        CO.sh_basis(4, d)


def test_oracle_known_answers():
    params, pts, nrm, knn, dc, rest = _scene()
    m = pts.shape[0]
    # one colour everywhere: that colour whatever the weights (they differ by orders of magnitude here)
    one_dc, one_rest = dc[:1].expand(300, 3), rest[:1].expand(300, 15, 3)
    for deg in range(4):
        got, w, c, fell = CO.colors(params, one_dc, one_rest, pts, nrm, knn, deg, parts=True)
        assert not fell.any() and float(w.max() / w.min().clamp_min(1e-300)) > 1e3
        assert float((got - c[:, 0].clamp(max=1)).abs().max()) < 1e-14 and float((c - c[:, :1]).abs().max()) == 0.0
    # degree 0: clamp(C0 dc + 0.5, 0, 1) of the weighted mean, whatever the normal
    got0, w, c, _ = CO.colors(params, dc, rest, pts, nrm, knn, 0, parts=True)
    assert float((c - (C0 * dc.double()[knn] + 0.5).clamp(min=0)).abs().max()) < 1e-15
    want = ((w[..., None] * c).sum(1) / w.sum(-1, keepdim=True)).clamp(max=1)
    assert float((got0 - want).abs().max()) < 1e-15
    assert torch.equal(got0, CO.colors(params, dc, rest, pts, -nrm, knn, 0))
    assert torch.equal(got0, CO.colors(params, dc, rest, pts, None, knn, 0))
    # a zero normal, a non-finite one and no normals at all: the degree-0 result at any degree
    odd = nrm.clone()
    odd[::2] = 0.0
    odd[1::4, 1] = float("nan")
    odd[3::4, 2] = float("inf")
    for deg in (1, 2, 3):
        assert torch.equal(CO.colors(params, dc, rest, pts, odd, knn, deg), got0)
        assert torch.equal(CO.colors(params, dc, rest, pts, None, knn, deg), got0)
    # degree 1 along the axes: the direction is -n, Y = (C0, -C1 y, C1 z, -C1 x)
    cases = {(1, 0, 0): (2, 1.0), (-1, 0, 0): (2, -1.0), (0, 1, 0): (0, 1.0), (0, -1, 0): (0, -1.0),
             (0, 0, 1): (1, -1.0), (0, 0, -1): (1, 1.0)}
    for axis, (band, sign) in cases.items():
        n_ax = torch.tensor(axis, dtype=torch.float32).expand(m, 3)
        _, w, c, _ = CO.colors(params, dc, rest, pts, n_ax, knn, 1, parts=True)
        want = (C0 * dc.double()[knn] + sign * C1 * rest.double()[knn][:, :, band] + 0.5).clamp(min=0)
        assert float((c - want).abs().max()) < 1e-14, axis
    # no weight at all (1e6 away: every q clamps to 1e8): the first listed neighbour's colour, finite
    far = pts + torch.tensor([1e6, 0.0, 0.0])
    got, w, c, fell = CO.colors(params, dc, rest, far, nrm, CO.exact_knn(far, params), 3, parts=True)
    assert fell.all() and float(w.sum()) == 0.0 and torch.equal(got, c[:, 0].clamp(max=1)) and bool(torch.isfinite(got).all())
    # an index outside [0, N) weighs nothing
    bad = knn.clone()
    bad[:, 5] = -1
    bad[:, 9] = 300
    keep = [k for k in range(16) if k not in (5, 9)]
    _, w, c, _ = CO.colors(params, dc, rest, pts, nrm, bad, 2, parts=True)
    _, w2, c2, _ = CO.colors(params, dc, rest, pts, nrm, knn, 2, parts=True)
    assert float(w[:, [5, 9]].abs().max()) == 0.0 and torch.equal(w[:, keep], w2[:, keep]) and torch.equal(c[:, keep], c2[:, keep])
    with pytest.raises(ValueError):
        CO.colors(params, dc, rest[:, :3], pts, nrm, knn, 2)


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    # n, m, points, normals, knn, records, colors_dc, colors_rest, k_rest, degree, colors, stream
    good = [20, 5, p, p, p, p, p, p, 15, 3, p, None]

    def call(**change):
        a = list(good)
        for i, v in change.items():
            a[int(i[1:])] = v
        return lib.ts_field_colors(*a)
    for i in (2, 4, 5, 6, 10):                                              # a NULL pointer (normals may be)
        assert call(**{f"a{i}": None}) == -1, i
    assert call(a7=None) == -1                                              # colors_rest is read above degree 0
    assert call(a0=0) == -1 and call(a0=-4) == -1 and call(a1=-1) == -1 and call(a8=-1) == -1
    for degree, k_rest in ((-1, 15), (4, 15), (4, 24), (1, 2), (2, 7), (3, 14), (1, 0)):
        assert call(a8=k_rest, a9=degree) == -2, (degree, k_rest)
    # nothing to do: no launch, whatever the pointers; the degree is still checked
    assert call(a1=0) == 0 and lib.ts_field_colors(20, 0, None, None, None, None, None, None, 0, 0, None, None) == 0
    assert call(a1=0, a9=4) == -2 and call(a0=0, a1=0) == -1
    assert lib.ts_abi_version() == 9 == _lib.ABI_VERSION


def test_config_and_mesh_fields():
    from tinysplat_amd import vertex_colors
    from tinysplat_amd.mesh import MeshConfig, TriangleMesh
    c = MeshConfig()
    assert c.colors is False and c.color_sh_degree is None
    assert MeshConfig(colors=True, color_sh_degree=2).color_sh_degree == 2
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            MeshConfig(colors=True, color_sh_degree=bad)
    v, f = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    three = TriangleMesh(v, f, None)
    assert three.colors is None and three.normals is None
    assert TriangleMesh(v, f, v, v + 0.5).colors is not None
    # no CPU fallback
    from tinysplat_amd.synthetic import make_scene
    model, _ = make_scene(40, 0, 32, 32, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vertex_colors(model, torch.zeros(4, 3))


def _mesh(colors=True):
    g = torch.Generator().manual_seed(3)
    verts = torch.randn(7, 3, generator=g) * 1e3
    nrm = torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=-1)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 0, 3]], dtype=torch.int32)
    # 0, 1, the rounding's half-way case, both sides of it, and values outside [0, 1]
    col = torch.tensor([[0.0, 1.0, 0.5 / 255], [0.49 / 255, 0.51 / 255, 1.5 / 255], [-0.3, 1.7, 0.5], [254.5 / 255, 0.999, 0.25],
                        [1e-9, -0.0, 100.0], [0.2, 0.4, 0.6], [127.4 / 255, 127.6 / 255, 2.5 / 255]])
    return verts, nrm, faces, (col if colors else None)


BYTES = np.array([[0, 255, 0], [0, 1, 2], [0, 255, 128], [254, 255, 64], [0, 0, 255], [51, 102, 153], [127, 128, 2]],
                 dtype=np.uint8)            # round half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, 127.5 -> 128


def test_rounding_table_is_round_of_the_clamp():
    col = _mesh()[3].numpy()
    prod = np.clip(col, 0.0, 1.0).astype(np.float32) * np.float32(255.0)
    # the half-way inputs really are half-way in float32, or the table above would test nothing
    assert prod[0, 2] == 0.5 and prod[1, 2] == 1.5 and prod[6, 2] == 2.5 and prod[3, 0] == 254.5
    assert np.array_equal(np.round(prod).astype(np.uint8), BYTES)


def test_colourless_output_is_byte_for_byte_the_old_one(tmp_path):
    """The expected bytes are built here the way the writers built them before they knew colours."""
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply, export_points_ply
    from tinysplat_amd.mesh import TriangleMesh
    verts, nrm, faces, _ = _mesh(False)
    rows = np.concatenate((verts.numpy(), nrm.numpy()), 1).astype("<f4")
    fields = [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    head = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex 7", *fields])
    frows = np.empty((4,), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frows["n"], frows["v"] = 3, faces.numpy()
    ply = (head + "\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii") \
        + rows.tobytes() + frows.tobytes()
    obj = "".join("v %.9g %.9g %.9g\n" % tuple(r) for r in verts.tolist()) \
        + "".join("vn %.9g %.9g %.9g\n" % tuple(r) for r in nrm.tolist()) \
        + "".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (faces + 1).tolist())
    pts = (head + "\nend_header\n").encode("ascii") + rows.tobytes()
    for mesh in (TriangleMesh(verts, faces, nrm), TriangleMesh(verts, faces, nrm, None),
                 SimpleNamespace(vertices=verts, faces=faces, normals=nrm)):
        export_mesh_ply(mesh, tmp_path / "m.ply")
        export_mesh_obj(mesh, tmp_path / "m.obj")
        assert (tmp_path / "m.ply").read_bytes() == ply and (tmp_path / "m.obj").read_bytes() == obj.encode("ascii")
    for cloud in (SimpleNamespace(points=verts, normals=nrm), SimpleNamespace(points=verts, normals=nrm, colors=None)):
        export_points_ply(cloud, tmp_path / "p.ply")
        assert (tmp_path / "p.ply").read_bytes() == pts
    from tinysplat_amd.formats import read_points_ply
    back = read_points_ply(tmp_path / "p.ply")
    assert torch.equal(back[0], verts) and torch.equal(back[1], nrm)


def read_colored_ply(path, faces=True):
    """A coloured ``export_mesh_ply`` / ``export_points_ply`` file -> (vertices, normals, uint8 colours, faces or None)."""
    blob = Path(path).read_bytes()
    marker = b"end_header\n"
    at = blob.find(marker)
    lines = blob[:at].decode("ascii").split("\n")
    assert lines.pop() == ""                                                # the header's lines all end in a newline
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].split()[:2] == ["element", "vertex"]
    assert lines[3:12] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"property uchar {k}" for k in ("red", "green", "blue")]
    v = int(lines[2].split()[2])
    body = at + len(marker)
    rows = np.frombuffer(blob, dtype=[("f", "<f4", (6,)), ("c", "u1", (3,))], count=v, offset=body)
    assert rows.dtype.itemsize == 27
    out_faces = None
    if faces:
        assert lines[12].split()[:2] == ["element", "face"] and lines[13:] == ["property list uchar int vertex_indices"]
        f = int(lines[12].split()[2])
        fr = np.frombuffer(blob, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=f, offset=body + v * 27)
        assert len(blob) == body + v * 27 + f * 13 and bool(np.all(fr["n"] == 3))
        out_faces = fr["v"].astype(np.int32).reshape(f, 3)
    else:
        assert len(lines) == 12 and len(blob) == body + v * 27
    return rows["f"][:, :3].copy(), rows["f"][:, 3:].copy(), rows["c"].copy(), out_faces


def test_writers_with_colours(tmp_path):
    from tinysplat_amd.formats import export_mesh_obj, export_mesh_ply, export_points_ply
    from tinysplat_amd.mesh import TriangleMesh
    verts, nrm, faces, col = _mesh()
    export_mesh_ply(TriangleMesh(verts, faces, nrm, col), tmp_path / "m.ply")
    v, n, c, f = read_colored_ply(tmp_path / "m.ply")
    assert np.array_equal(v, verts.numpy()) and np.array_equal(n, nrm.numpy()) and np.array_equal(f, faces.numpy())
    assert np.array_equal(c, BYTES)
    export_mesh_ply(TriangleMesh(verts, faces, None, col), tmp_path / "z.ply")          # colours without normals
    v, n, c, f = read_colored_ply(tmp_path / "z.ply")
    assert np.array_equal(n, np.zeros((7, 3), np.float32)) and np.array_equal(c, BYTES)
    export_points_ply(SimpleNamespace(points=verts, normals=nrm, colors=col), tmp_path / "p.ply")
    v, n, c, f = read_colored_ply(tmp_path / "p.ply", faces=False)
    assert np.array_equal(v, verts.numpy()) and np.array_equal(n, nrm.numpy()) and np.array_equal(c, BYTES) and f is None
    export_mesh_obj(TriangleMesh(verts, faces, nrm, col), tmp_path / "m.obj")
    lines = (tmp_path / "m.obj").read_text().splitlines()
    vs = [ln.split() for ln in lines if ln.startswith("v ")]
    assert len(vs) == 7 and all(len(t) == 7 for t in vs)
    got = np.asarray([[float(x) for x in t[1:]] for t in vs], dtype=np.float32)
    assert np.array_equal(got[:, :3], verts.numpy()) and np.array_equal(got[:, 3:], col.clamp(0, 1).numpy())
    want = "v %.9g %.9g %.9g %.9g %.9g %.9g" % (*verts[5].tolist(), *col[5].tolist())
    assert lines[5] == want and sum(ln.startswith("vn ") for ln in lines) == 7 and sum(ln.startswith("f ") for ln in lines) == 4
    # the empty mesh, and colours of the wrong shape
    export_mesh_ply(TriangleMesh(verts[:0], faces[:0], nrm[:0], col[:0]), tmp_path / "e.ply")
    v, n, c, f = read_colored_ply(tmp_path / "e.ply")
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    for write in (export_mesh_ply, export_mesh_obj):
        with pytest.raises(ValueError):
            write(TriangleMesh(verts, faces, nrm, col[:5]), tmp_path / "b")
    with pytest.raises(ValueError):
        export_points_ply(SimpleNamespace(points=verts, normals=nrm, colors=col[:, :2]), tmp_path / "b")
