"""The field colours on the GPU (``MeshConfig(colors=True)``, ``vertex_colors``, ``ts_field_colors``; csrc/field_color.hip,
DESIGN.md section 6h) against the float64 oracle (tests/color_oracle.py) on the sheet-and-blob scene of
tests/test_gpu_mesh.py with seeded SH coefficients.

The bar follows sections 6f / 6g: 4 x ``E_c``, the largest deviation of the oracle's float32 run from its float64 run
on the same inputs, printed before it is asserted.  Every vertex is compared: the definition has no discrete decision.
On the CPU (the oracle's own mesh of this scene, 7206 vertices) ``E_c`` is 4.3e-7, 4.5e-7, 5.9e-7 and 5.6e-7 at
degree 0..3, the colours span 0.007..1 and under 3 % of the channels sit at the upper clamp."""
import functools

import numpy as np
import pytest
import torch

import color_oracle as CO
import mesh_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
SEED = 11
COEFF_SEED = 5
BOUNDS = ((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2))
U = 2.0 ** -24                      # float32's unit roundoff
C0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def _scene():
    params = MO.sheet_scene(SEED)
    dc, rest = CO.coefficients(params["means"].shape[0], 15, COEFF_SEED)
    return params, dc, rest


def _model(k_rest=15, active=3):
    from tinysplat_amd.synthetic import SplatModel
    params, dc, rest = _scene()
    p = {k: torch.as_tensor(v, dtype=torch.float32).to(DEV) for k, v in params.items()}
    return SplatModel(p["means"], dc.to(DEV), rest[:, :k_rest].contiguous().to(DEV), p["scales"], p["quats"],
                      p["opacities"], active, background=torch.zeros(3, device=DEV))


def _extract(model=None, **cfg):
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    cfg.setdefault("resolution", 37)
    mesh = extract_mesh(model if model is not None else _model(), MeshConfig(bounds=BOUNDS, **cfg))
    torch.cuda.synchronize()
    return mesh


@functools.lru_cache(maxsize=None)
def _colored(degree):
    return _extract(colors=True, color_sh_degree=degree)


def _oracle_pair(points, normals, degree, knn=None):
    """The float64 colours and ``E_c`` at the given float32 points and normals (CPU tensors)."""
    params, dc, rest = _scene()
    knn = CO.exact_knn(points, params) if knn is None else knn
    c64 = CO.colors(params, dc, rest, points, normals, knn, degree, torch.float64)
    c32 = CO.colors(params, dc, rest, points, normals, knn, degree, torch.float32)
    return c64, float((c32.double() - c64).abs().max())


@functools.lru_cache(maxsize=None)
def _near_sheet(m=1000, seed=7):
    g = torch.Generator().manual_seed(seed)
    xy = 0.95 * (2 * torch.rand(m, 2, generator=g) - 1)
    z = 3.0 + 0.1 * torch.sin(2.0 * xy[:, :1]) * torch.cos(1.5 * xy[:, 1:]) + 0.03 * torch.randn(m, 1, generator=g)
    return torch.cat((xy, z), 1), torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=-1)


@functools.lru_cache(maxsize=None)
def _near_oracle():
    return _oracle_pair(*_near_sheet(), 3)


def _entry(model, points, normals, degree):
    """``ts_knn`` and ``ts_field_colors`` called directly on all of ``points`` (device tensors) in one launch each."""
    from tinysplat_amd import _field, _lib
    from tinysplat_amd.ops import _stream
    lib = _lib.load()
    pk = _field.pack_model(model)
    m = points.shape[0]
    dev = points.device
    ws = torch.empty((int(lib.ts_knn_ws_bytes(pk.means.shape[0], m, 16)),), dtype=torch.uint8, device=dev)
    dist = torch.empty((m, 16), device=dev)
    idx = torch.empty((m, 16), dtype=torch.int32, device=dev)
    out = torch.full((m + 1, 3), -7.0, device=dev)                          # a guard row behind the last point
    with torch.cuda.device(dev):
        _field.colors_at(lib, pk, model.colors_dc, model.colors_rest, points, normals, m, degree, out, dist, idx, ws,
                         _stream(dev))
    torch.cuda.synchronize()
    assert bool((out[m] == -7.0).all())
    return out[:m].clone(), idx


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_mesh_colors_match_the_oracle(degree):
    mesh = _colored(degree)
    v = mesh.vertices.shape[0]
    assert v > 5000 and mesh.colors.shape == (v, 3) and mesh.colors.dtype == torch.float32 and mesh.colors.is_cuda
    col = mesh.colors.cpu()
    assert bool(torch.isfinite(col).all()) and float(col.min()) >= 0.0 and float(col.max()) <= 1.0
    c64, e_c = _oracle_pair(mesh.vertices.cpu(), mesh.normals.cpu(), degree)
    err = float((col.double() - c64).abs().max())
    print(f"\ndegree {degree}: {v} vertices, err {err:.3e}, E_c {e_c:.3e} (bar {FACTOR * e_c:.3e}); colours "
          f"{float(c64.min()):.3f}..{float(c64.max()):.3f}, at the upper clamp {float((c64 == 1).double().mean()):.4f}")
    assert 1e-8 < e_c < 1e-5                                                # a sane float32 yardstick
    assert err <= FACTOR * e_c
    if degree:                                                              # the bands do change the picture
        assert float((col - _colored(0).colors.cpu()).abs().max()) > 0.05


@pytest.mark.parametrize("m", [1, 3, 4, 5, 15, 16, 17, 64, 1000])
def test_entry_on_partial_rows_and_tail_blocks(m):
    """One 16-lane row per point, 4 rows per wave, 16 per workgroup: ``m`` around those sizes.  The points are the first
    ``m`` of one draw of 1000 and the bar is 4 x E_c of the whole draw: a single point's float32 restatement can agree
    with float64 by chance, which says nothing about the error scale of the scene."""
    pts, nrm = _near_sheet()
    c64, e_c = _near_oracle()
    got, _ = _entry(_model(), pts[:m].to(DEV), nrm[:m].to(DEV), 3)
    err = float((got.cpu().double() - c64[:m]).abs().max())
    print(f"\nm {m}: err {err:.3e}, E_c {e_c:.3e} (bar {FACTOR * e_c:.3e})")
    assert 1e-8 < e_c < 1e-5 and err <= FACTOR * e_c


def test_bit_identity():
    from tinysplat_amd import _lib, vertex_colors
    from tinysplat_amd.ops import kernel_timer
    one = _colored(3)
    two = _extract(colors=True, color_sh_degree=3)
    assert torch.equal(one.colors, two.colors) and torch.equal(one.normals, two.normals)
    # at least four chunks of vertices against one
    lib = _lib.load()
    v, n = one.vertices.shape[0], _scene()[0]["means"].shape[0]
    per = -(-v // 5)
    cap = int(lib.ts_knn_ws_bytes(n, per, 16)) + 2 * (-(-per * 64 // 256) * 256)
    assert cap >= int(lib.ts_mesh_chunk_bytes(n, 1))
    kernel_timer.start()
    try:
        small = _extract(colors=True, color_sh_degree=3, max_workspace_bytes=cap)
    finally:
        parts = kernel_timer.stop()
    launches = parts["ts_field_colors"][0]
    print(f"\n{v} vertices: with a {cap} byte cap {launches} colour launches, {parts['ts_extract_normals'][0]} of the "
          f"normals, {parts['ts_knn'][0]} searches")
    assert launches >= 4 and parts["ts_extract_normals"][0] == launches
    assert torch.equal(small.colors, one.colors) and torch.equal(small.vertices, one.vertices)
    # vertex_colors on the mesh's own vertices and normals, in one chunk and in several
    model = _model()
    assert torch.equal(vertex_colors(model, one.vertices, one.normals), one.colors)
    assert torch.equal(vertex_colors(model, one.vertices, one.normals, max_workspace_bytes=cap), one.colors)
    # a point's colour does not depend on the call it is part of
    pts, nrm = (t.to(DEV) for t in _near_sheet())
    big, idx = _entry(model, pts, nrm, 3)
    few, _ = _entry(model, pts[:17].contiguous(), nrm[:17].contiguous(), 3)
    assert torch.equal(big[:17], few)
    assert torch.equal(vertex_colors(model, pts, nrm), big)
    # ts_knn's contract, which the fallback to the first listed neighbour leans on: ascending distance
    d = (pts[:, None, :] - model.means[idx.long()]).norm(dim=-1)
    assert bool((d[:, 1:] >= d[:, :-1] - 1e-6).all())


def test_the_colourless_path_is_unchanged():
    from tinysplat_amd.ops import kernel_timer
    with_colors = _colored(3)
    kernel_timer.start()
    try:
        plain = _extract()
    finally:
        parts = kernel_timer.stop()
    assert "ts_field_colors" not in parts and plain.colors is None
    assert torch.equal(plain.vertices, with_colors.vertices) and torch.equal(plain.faces, with_colors.faces)
    assert torch.equal(plain.normals, with_colors.normals)
    bare = _extract(normals=False, colors=True, color_sh_degree=3)
    assert bare.normals is None and torch.equal(bare.colors, with_colors.colors)
    assert torch.equal(bare.vertices, with_colors.vertices)
    # the model's active degree is the default, a lower one may be asked for
    assert torch.equal(_extract(colors=True).colors, with_colors.colors)
    assert torch.equal(_extract(_model(active=1), colors=True).colors, _colored(1).colors)
    assert torch.equal(_extract(_model(k_rest=3, active=1), colors=True).colors, _colored(1).colors)


def test_degenerate_inputs():
    from test_gpu_mesh import _model as grey_model
    from tinysplat_amd import vertex_colors
    from tinysplat_amd.mesh import MeshConfig, extract_mesh
    from tinysplat_amd.ops import kernel_timer
    params, dc, rest = _scene()
    # no higher bands stored, every Gaussian 0.5: one colour, up to the rounding of sum(w c) / sum(w) - a product, four
    # levels of the butterfly above and below and the division: 10 roundings at most
    grey = extract_mesh(grey_model(params), MeshConfig(resolution=37, bounds=BOUNDS, colors=True))
    want = float(np.float32(C0) * np.float32(0.5) + np.float32(0.5))
    assert grey.colors.shape[0] > 5000 and float((grey.colors - want).abs().max()) <= 10 * U * want
    for model, kw in ((grey_model(params), dict(color_sh_degree=1)), (_model(k_rest=8), dict(color_sh_degree=3)),
                      (_model(k_rest=8), {})):
        with pytest.raises(ValueError):
            extract_mesh(model, MeshConfig(resolution=8, bounds=BOUNDS, colors=True, **kw))
    with pytest.raises(ValueError):
        vertex_colors(_model(k_rest=3, active=1), torch.zeros((4, 3), device=DEV), sh_degree=2)
    # no normals: band 0 alone; so for a zero or non-finite normal among good ones
    model = _model()
    pts, nrm = (t.to(DEV) for t in _near_sheet())
    flat = vertex_colors(model, pts, None)
    assert torch.equal(flat, vertex_colors(model, pts, nrm, sh_degree=0))
    assert torch.equal(flat, vertex_colors(model, pts, None, sh_degree=0))
    odd = nrm.clone()
    odd[::3] = 0.0
    odd[1::6, 1] = float("nan")
    odd[4::6, 2] = float("inf")
    mixed, full = vertex_colors(model, pts, odd), vertex_colors(model, pts, nrm)
    bad = ~(torch.isfinite(odd).all(-1) & (odd.norm(dim=-1) > 0))
    assert int(bad.sum()) > 400 and torch.equal(mixed[bad], flat[bad]) and torch.equal(mixed[~bad], full[~bad])
    assert bool(torch.isfinite(mixed).all()) and not torch.equal(full[bad], flat[bad])
    # 1e6 away from every Gaussian no weight is left: the nearest Gaussian's own colour
    far = (pts[:40] + torch.tensor([1e6, -2e6, 5e5], device=DEV)).contiguous()
    got = vertex_colors(model, far, nrm[:40].contiguous()).cpu()
    knn = CO.exact_knn(far.cpu(), params)
    c64, w, c, fell = CO.colors(params, dc, rest, far.cpu(), nrm[:40].cpu(), knn, 3, parts=True)
    assert bool(fell.all()) and bool(torch.isfinite(got).all()) and float(got.min()) >= 0 and float(got.max()) <= 1
    # among equidistant candidates (float32 distances at 1e6) any may be "the nearest": compare with the one taken
    _, idx = _entry(model, far, nrm[:40].contiguous(), 3)
    first = idx[:, :1].cpu().long().expand(40, 16)
    c_first = CO.colors(params, dc, rest, far.cpu(), nrm[:40].cpu(), first, 3)
    # 16 products and 16 sums on top of the basis's own few roundings (the normalised direction, the polynomials), each
    # relative to at most sum_k |Y_k| |coeff_k| + 0.5 with |Y_k| < 0.75 on the unit sphere for the bands 0..3
    mag = C0 * dc.abs().max() + 0.75 * rest.abs().max() * 15 + 0.5
    assert float((got.double() - c_first).abs().max()) <= 40 * U * float(mag)
    # the empty mesh: colours [0,3], nothing launched
    faint = _model()
    faint.opacities = torch.full_like(faint.opacities, float(np.log(0.01 / 0.99)))
    kernel_timer.start()
    try:
        empty = extract_mesh(faint, MeshConfig(resolution=16, bounds=BOUNDS, colors=True))
    finally:
        parts = kernel_timer.stop()
    assert empty.colors.shape == (0, 3) and empty.colors.dtype == torch.float32 and empty.colors.is_cuda
    assert empty.vertices.shape == (0, 3) and "ts_field_colors" not in parts and "ts_extract_normals" not in parts
    assert vertex_colors(model, torch.zeros((0, 3), device=DEV)).shape == (0, 3)


def test_ply_of_a_coloured_gpu_mesh_reads_back(tmp_path):
    from test_color_cpu import read_colored_ply
    from tinysplat_amd.formats import export_mesh_ply
    mesh = _colored(3)
    export_mesh_ply(mesh, tmp_path / "m.ply")
    v, n, c, f = read_colored_ply(tmp_path / "m.ply")
    assert np.array_equal(v, mesh.vertices.cpu().numpy()) and np.array_equal(n, mesh.normals.cpu().numpy())
    assert np.array_equal(f, mesh.faces.cpu().numpy())
    want = np.round(np.clip(mesh.colors.cpu().numpy(), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(c, want) and len(np.unique(c)) > 200
