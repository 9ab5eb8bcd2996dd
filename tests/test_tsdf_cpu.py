"""The depth-map fusion without a GPU: the oracle on analytic surfaces, the NaN rule cell by cell,
the cap on decision-unstable corners of every case, the host build of csrc/tsdf_math.h against the oracle, the new symbols,
their refusals, ``FusionConfig`` and the export tool's flags."""
import ctypes
import importlib.util
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_oracle as MO
import tsdf_cases as TC
import tsdf_oracle as TO

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("ts_tsdf_camera_bytes", "ts_tsdf_mark", "ts_tsdf_chunk_bytes", "ts_tsdf_integrate", "ts_tsdf_field",
           "ts_mesh_count_observed", "ts_mesh_emit_observed")
UNSTABLE_CAP = 0.01


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TC.build_host(tmp_path_factory.mktemp("tsdf_host"))


def _table(c):
    """The camera table as tinysplat_amd.fusion builds it, over host memory -> (ctypes array, what keeps it alive)."""
    from tinysplat_amd import _lib, fusion
    cams, depths = TC.torch_inputs(c, "cpu")
    raw = fusion.camera_table(cams, depths)
    table = (_lib.TsTsdfCamera * len(cams)).from_buffer_copy(raw.tobytes())
    return table, depths


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_puts_the_frontal_planes_vertices_on_the_plane():
    c = TC.case("front")
    m = TO.march_observed(c.F, c.positions)
    _, faces, verts = MO.weld(m["keys"], m["pos"])
    view = c.cams[0]["view"].astype(np.float64)
    residual = np.abs(verts @ view[2, :3] + view[2, 3] - 2.5)
    print(f"\n{verts.shape[0]} vertices, worst distance from the plane {residual.max():.3e}")
    assert verts.shape[0] > 1000 and residual.max() <= 1e-12
    # the normal points outwards: towards the camera, against its axis
    tri = verts[faces]
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    big = np.linalg.norm(normals, axis=1) > 1e-6
    assert big.sum() > 1000 and bool(np.all(normals[big] @ view[2, :3] < 0))


def test_oracle_sphere_is_closed_and_near_the_sphere():
    c = TC.case("sphere")
    m = TO.march_observed(c.F, c.positions)
    _, faces, verts = MO.weld(m["keys"], m["pos"])
    closed, edges = MO.edge_census(faces)
    assert closed and edges > 10000
    r = np.linalg.norm(verts - TC.SPHERE_C, axis=1)
    assert abs(MO.enclosed_volume(verts, faces) / (4 / 3 * math.pi * TC.SPHERE_R ** 3) - 1) < 0.1
    assert r.min() > TC.SPHERE_R - 2 * float(c.h) and r.max() < TC.SPHERE_R + 2 * float(c.h)


@pytest.mark.parametrize("name", ["plane1", "plane7_thin", "slab3"])
def test_nan_rule_cell_by_cell(name):
    c = TC.case(name)
    F = c.F
    nz, ny, nx = (s - 1 for s in F.shape)
    emitted = np.zeros(nz * ny * nx, dtype=bool)
    emitted[TO.march_observed(F)["cell"]] = True
    emitted = emitted.reshape(nz, ny, nx)
    dropped = 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                corners = F[k:k + 2, j:j + 2, i:i + 2].reshape(-1)
                inside = corners > 0
                crossed = bool(inside.any()) and not bool(inside.all())
                unseen = bool(np.isnan(corners).any())
                assert emitted[k, j, i] == (crossed and not unseen), (k, j, i)
                dropped += crossed and unseen
    print(f"\n{name}: {int(emitted.sum())} cells emit, {dropped} crossed cells have a NaN corner and emit nothing")
    assert emitted.sum() > 500 and dropped > 0
    assert bool(np.isnan(F).any()) and bool((c.count[np.isnan(F)] < c.min_observations).all())


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_case_inputs_keep_the_unstable_corners_under_the_cap(name):
    c = TC.case(name)
    active = TC.active_bricks(c)
    g, inside = TO.brick_corner_index(active, c.cells)
    gi, gj, gk = (np.minimum(g[..., a], c.cells[a]) for a in range(3))
    share = float(c.unstable[gk, gj, gi][inside].mean())
    print(f"\n{name}: {active.size} active bricks, unstable corners {100 * share:.3f} %")
    assert 0 < active.size and share <= UNSTABLE_CAP
    assert tuple(c.cells) == ((20, 17, 9) if name == "slab3" else (24, 24, 24))


def test_cases_cover_what_the_issue_lists():
    cams = TC.plane_cameras()
    assert len(cams) == 7 and [k["depth"].shape for k in cams].count((32, 32)) == 1
    assert sum(k["depth"].shape == (40, 48) for k in cams) == 6
    d = cams[0]["depth"]
    assert bool(np.isnan(d).any()) and bool((d[17:20] == 0).all()) and bool((d < 0).any())
    # the fifth camera sits inside the volume and has part of the grid behind it
    c = TC.case("plane7")
    view = cams[4]["view"].astype(np.float64)
    centre = -view[:3, :3].T @ view[:3, 3]
    assert bool(np.all(np.abs(centre) < 1.2))
    z = c.positions.astype(np.float64) @ view[2, :3] + view[2, 3]
    assert 0.05 < float((z <= TC.ZNEAR).mean()) < 0.95
    assert {TC.CASES[n][3] for n in TC.CASES} == {2.0, 4.0} and {TC.CASES[n][4] for n in TC.CASES} == {1, 2}
    assert {len(TC.CASES[n][2]()) for n in TC.CASES} >= {1, 2, 7}
    assert len(TC.sphere_cameras()) == 6


# -------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("name", ["plane7", "slab3"])
def test_host_pixel_and_observation_against_the_oracle(host, name):
    from tinysplat_amd import _lib
    c = TC.case(name)
    table, depths = _table(c)
    assert host.th_camera_bytes() == ctypes.sizeof(_lib.TsTsdfCamera)
    pts = c.positions.reshape(-1, 3)
    z_out, t_out = ctypes.c_float(), ctypes.c_float()
    worst = 0.0
    for ci, cam in enumerate(c.cams):
        o = {k: v.reshape(-1) for k, v in TO.observe(cam, c.positions, c.trunc, TC.ZNEAR).items()}
        depth = cam["depth"]
        width = depth.shape[1]
        rec = ctypes.addressof(table) + ci * ctypes.sizeof(_lib.TsTsdfCamera)
        checked = 0
        for e in np.flatnonzero(~o["unstable"]):
            pixel = host.th_pixel(rec, pts[e, 0], pts[e, 1], pts[e, 2], TC.ZNEAR, ctypes.byref(z_out))
            if not o["in_image"][e]:
                assert pixel == -1, (ci, e)
                continue
            assert pixel == int(o["py"][e]) * width + int(o["px"][e]), (ci, e)
            seen = host.th_observe(float(depth.reshape(-1)[pixel]), z_out.value, float(c.trunc), math.inf, ctypes.byref(t_out))
            assert bool(seen) == bool(o["seen"][e]), (ci, e)
            if seen:
                err = abs(float(t_out.value) - float(o["t"][e]))
                # the bound of one observation, and the float32 rounding of the stored t itself
                assert err <= o["e_t"][e] + TO.U * abs(o["t"][e]), (ci, e, err, o["e_t"][e])
                worst = max(worst, err / o["e_t"][e])
                checked += 1
        assert checked > 500
    print(f"\n{name}: worst |t - oracle| / bound {worst:.3f}")


def test_host_observation_rules(host):
    t = ctypes.c_float()
    inf = math.inf
    for d in (0.0, -1.0, math.nan, inf, -inf):
        assert host.th_observe(d, 1.0, 0.4, inf, ctypes.byref(t)) == 0                # no depth
    assert host.th_observe(2.0, 1.0, 0.4, 1.5, ctypes.byref(t)) == 0                  # beyond depth_max
    assert host.th_observe(2.0, 1.0, 0.4, 2.0, ctypes.byref(t)) == 1 and t.value == 1.0
    assert host.th_observe(1.0, 1.5, 0.4, inf, ctypes.byref(t)) == 0                  # occluded: s < -trunc
    assert host.th_observe(1.0, 1.25, 0.5, inf, ctypes.byref(t)) == 1 and t.value == -0.5
    assert host.th_observe(1.0, 1.5, 0.5, inf, ctypes.byref(t)) == 1 and t.value == -1.0    # s == -trunc stays


@pytest.mark.parametrize("name", ["plane7", "slab3", "narrow2"])
def test_host_cull_never_skips_a_corner_the_rule_accepts(host, name):
    """The sphere test of every (brick, camera) pair against the oracle's per-corner steps 1 and 2, unstable corners
    included: a culled brick has no corner inside the image."""
    from tinysplat_amd import _lib
    c = TC.case(name)
    table, depths = _table(c)
    nb = [-(-n // 8) for n in c.cells]
    bricks = np.arange(nb[0] * nb[1] * nb[2])
    g, inside = TO.brick_corner_index(bricks, c.cells)
    gi, gj, gk = (np.minimum(g[..., a], c.cells[a]) for a in range(3))
    pos = c.positions[gk, gj, gi].astype(np.float64)                                    # [B,729,3]
    culled = 0
    for ci, cam in enumerate(c.cams):
        o = TO.observe(cam, c.positions, c.trunc, TC.ZNEAR)
        accepted = (o["in_image"] | (o["unstable"] & (o["z"] > 0)))[gk, gj, gi] & inside
        rec = ctypes.addressof(table) + ci * ctypes.sizeof(_lib.TsTsdfCamera)
        for b in bricks:
            p = pos[b][inside[b]]
            lo, hi = p.min(0), p.max(0)
            centre = (0.5 * (lo.astype(np.float32) + hi.astype(np.float32))).astype(np.float32)
            radius = float(np.float32(np.linalg.norm(np.maximum(hi - centre, centre - lo)) + 0.0625 * float(c.h)))
            if host.th_cull(rec, centre[0], centre[1], centre[2], radius, TC.ZNEAR):
                culled += 1
                assert not accepted[b].any(), (ci, b)
    print(f"\n{name}: {culled} of {len(c.cams) * bricks.size} (brick, camera) pairs culled")
    assert culled > 20 or name != "narrow2"             # bricks this large are rarely outside a frustum that sees the scene


def test_host_unprojection_inverts_the_pixel(host):
    from tinysplat_amd import _lib
    c = TC.case("plane2")
    table, depths = _table(c)
    out = (ctypes.c_double * 3)()
    pts = c.positions.reshape(-1, 3)
    for ci, cam in enumerate(c.cams):
        o = {k: v.reshape(-1) for k, v in TO.observe(cam, c.positions, c.trunc, TC.ZNEAR).items()}
        rec = ctypes.addressof(table) + ci * ctypes.sizeof(_lib.TsTsdfCamera)
        for e in np.flatnonzero(o["in_image"])[::37]:
            assert host.th_unproject(rec, float(o["u"][e]), float(o["v"][e]), float(o["z"][e]), out) == 1
            assert np.abs(np.array(out[:]) - pts[e].astype(np.float64)).max() < 1e-9


# ----------------------------------------------------------------------------------------------- the symbols, the wrappers
def test_new_symbols_are_declared_exported_and_bound():
    from tinysplat_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tinysplat_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 9 and lib.ts_abi_version() == 9
    assert lib.ts_tsdf_camera_bytes() == ctypes.sizeof(_lib.TsTsdfCamera)
    import tinysplat_amd
    for name in ("FusionConfig", "fuse_depth_maps", "render_depth_alpha", "extract_mesh_tsdf"):
        assert name in tinysplat_amd.__all__ and hasattr(tinysplat_amd, name)
    src = (ROOT / "tinysplat_amd" / "fusion.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(oracle|scipy)", src, flags=re.M)
    build = (ROOT / "tinysplat_amd" / "_build.py").read_text()
    assert re.search(r'\("tsdf\.hip", \["-ffp-contract=off"\]\)', build)


def test_entries_refuse_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    grid = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.1)
    cells = (ctypes.c_int32 * 3)(24, 24, 24)
    bad_grid = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    inf = math.inf
    assert lib.ts_tsdf_chunk_bytes(0) == -1 and lib.ts_tsdf_chunk_bytes((2 ** 31 - 1) // 729 + 1) == -1
    a = lambda b: (b + 255) // 256 * 256
    for b in (1, 7, 1000):
        assert lib.ts_tsdf_chunk_bytes(b) == a(b * 729 * 8) + 2 * a(b * 729 * 4) + a(b * 4) + a(b * 8)
    mark = lambda **kw: lib.ts_tsdf_mark(*{**dict(c=2, t=p, m=1920, g=grid, n=cells, tr=0.4, dm=inf, f=p, s=None), **kw}.values())
    for kw in (dict(c=0), dict(c=65536), dict(t=None), dict(m=0), dict(m=2 ** 31), dict(g=bad_grid), dict(g=None), dict(n=None),
               dict(tr=0.0), dict(tr=inf), dict(tr=math.nan), dict(dm=0.0), dict(dm=math.nan), dict(f=None)):
        assert mark(**kw) == -1, kw
    integ = lambda **kw: lib.ts_tsdf_integrate(*{**dict(b=1, i=p, g=grid, n=cells, t=p, c0=0, c1=1, tr=0.4, zn=0.001, dm=inf,
                                                        fl=0, s=p, c=p, st=None), **kw}.values())
    for kw in (dict(b=0), dict(i=None), dict(g=bad_grid), dict(n=None), dict(t=None), dict(c0=-1), dict(c0=2), dict(tr=-1.0),
               dict(zn=math.nan), dict(dm=-1.0), dict(fl=2), dict(s=None), dict(s=p + 4), dict(c=None)):
        assert integ(**kw) == -1, kw
    assert integ(c0=1, c1=1) == 0                                                      # no camera: nothing to launch
    assert lib.ts_tsdf_field(0, p, p, 1, p, None) == -1 and lib.ts_tsdf_field(1, p, p, 0, p, None) == -1
    for missing in (1, 2, 4):
        args = [1, p, p, 1, p, None]
        args[missing] = None
        assert lib.ts_tsdf_field(*args) == -1
    assert lib.ts_mesh_count_observed(0, p, grid, cells, 0.0, p, p, None) == -1
    assert lib.ts_mesh_count_observed(1, p, grid, cells, math.nan, p, p, None) == -1
    assert lib.ts_mesh_count_observed(1, p, bad_grid, cells, 0.0, p, p, None) == -1
    assert lib.ts_mesh_count_observed(1, p, grid, cells, 0.0, None, p, None) == -1
    assert lib.ts_mesh_emit_observed(1, p, grid, cells, 0.0, p, None, p, p, None, None) == -1
    assert lib.ts_mesh_emit_observed(1, p, grid, cells, 0.0, p, p, None, p, None, None) == -1
    assert lib.ts_mesh_emit_observed(0, p, grid, cells, 0.0, p, p, p, p, None, None) == -1


def test_fusion_config_validation_and_cpu_refusal():
    from tinysplat_amd import CleanConfig, FusionConfig, fuse_depth_maps
    cfg = FusionConfig()
    assert (cfg.resolution, cfg.bounds, cfg.trunc_voxels, cfg.znear, cfg.depth_max, cfg.min_alpha, cfg.min_observations,
            cfg.sparse, cfg.max_workspace_bytes, cfg.camera_batch, cfg.target_faces, cfg.clean) == (
                256, None, 4.0, 0.001, math.inf, 0.5, 1, True, 256 << 20, None, None, None)
    FusionConfig(clean=CleanConfig(), target_faces=10, camera_batch=1, bounds=((0, 0, 0), (1, 1, 1)), resolution=4)
    for bad in (dict(resolution=0), dict(trunc_voxels=0.0), dict(trunc_voxels=math.inf), dict(znear=math.nan),
                dict(depth_max=0.0), dict(depth_max=math.nan), dict(min_alpha=0.0), dict(min_alpha=1.5),
                dict(min_observations=0), dict(max_workspace_bytes=0), dict(camera_batch=0), dict(target_faces=0),
                dict(clean="yes"), dict(bounds=((0, 0, 0), (1, 0, 1))), dict(resolution=8, trunc_voxels=4.0)):
        with pytest.raises(ValueError):
            FusionConfig(**bad)
    c = TC.case("plane1")
    cams, depths = TC.torch_inputs(c, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_depth_maps(cams, depths, FusionConfig(bounds=c.bounds, resolution=24))
    with pytest.raises(ValueError, match="one depth map per camera"):
        fuse_depth_maps(cams, [], FusionConfig(bounds=c.bounds, resolution=24))


def test_projview_and_planes_match_the_oracle():
    from tinysplat_amd import fusion
    c = TC.case("plane2")
    cams, _ = TC.torch_inputs(c, "cpu")
    for cam, k in zip(cams, c.cams):
        pv = fusion.projview(cam)
        assert pv.dtype == np.float32 and pv.tobytes() == TO.projview(k["view"], k["proj"]).tobytes()
        planes = fusion.cull_planes(k["view"], pv)
        assert planes.shape == (6, 5) and planes[0, :4].tobytes() == k["view"][2].tobytes()
        assert planes[1, :4].tobytes() == pv[3].tobytes()
        assert bool(np.all(planes[:, 4] >= np.linalg.norm(planes[:, :3].astype(np.float64), axis=1) * (1 - 1e-6)))


# ------------------------------------------------------------------------------------------------------------ the tool
def test_export_tool_mesher_flags():
    spec = importlib.util.spec_from_file_location("tool_export", str(ROOT / "tools" / "export.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse(["in.ply", "out.obj", "--filetype", "OBJ"])
    assert a.mesher == "density" and a.dataset_dir is None
    a = tool.parse(["in.ply", "out.ply", "--filetype", "MESH_PLY", "--mesher", "tsdf", "--dataset-dir", "scene"])
    assert a.mesher == "tsdf" and a.dataset_dir == "scene"
    for bad in (["in.ply", "o.obj", "--filetype", "OBJ", "--mesher", "tsdf"],                       # no cameras
                ["in.ply", "o.obj", "--filetype", "OBJ", "--dataset-dir", "scene"],                  # cameras, density mesher
                ["in.ply", "o.splat", "--filetype", "SPLAT", "--mesher", "tsdf", "--dataset-dir", "scene"],
                ["in.ply", "o.obj", "--filetype", "OBJ", "--mesher", "tsdf", "--dataset-dir", "s", "--colors"],
                ["in.ply", "o.obj", "--filetype", "OBJ", "--mesher", "poisson"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    assert "--mesher" in tool.__doc__ and "--dataset-dir" in tool.__doc__
