"""The level-set surface extraction on the GPU (tinysplat_amd.extract, csrc/extract.hip) against the float64 oracle
(tests/extract_oracle.py) on the reference's fixture (tests/golden/extract_points.npz).

The oracle judges stage by stage (see its docstring): the back-projection against the float64 back-projection, and
everything downstream - neighbours, densities, keep / first, t, points - in float64 on the GPU's own float32
``p_world`` and sample positions.  The bars are 4 x the deviations of the reference's own float32 run from the same
oracle, read from the fixture (``E_pw``, ``E_d``, ``E_pts``; ``E_n``, for the normals, is the float32 restatement of
the oracle against its float64 evaluation).  "``t`` is held to ``E_pts``" is read as: ``t``, for which the reference
records no value of its own, shares the points' allowance and factor (``|d point| = |d t|`` along a unit direction),
so it is asserted against 4 x ``E_pts`` too.  The sample positions are held to two float32 ulps of the largest
coordinate (three roundings: ``lin * p_std``, ``* dir``, ``+ p_world``).  Every figure is printed before it is asserted.

These tests are for the default build of the library (``TS_PIX_OFF`` = 0, the only build ``_lib.load`` accepts in
this process): the oracle's ``pix_off`` stays 0."""
import math

import numpy as np
import pytest
import torch

import extract_oracle as EO
from helpers import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def _z():
    return np.load(GOLD / "extract_points.npz")


def _model(params, dev=DEV):
    from tinysplat_amd.synthetic import SplatModel
    p = {k: torch.as_tensor(v, dtype=torch.float32).to(dev) for k, v in params.items()}
    n = p["means"].shape[0]
    return SplatModel(p["means"], torch.full((n, 3), 0.5, device=dev), torch.zeros((n, 0, 3), device=dev), p["scales"],
                      p["quats"], p["opacities"], 0, background=torch.zeros(3, device=dev))


def _camera(z, c):
    from tinysplat_amd.synthetic import PinholeCamera
    cam = PinholeCamera(torch.from_numpy(z[c + "view_matrix"]), torch.from_numpy(z[c + "proj_matrix"]),
                        float(z[c + "f"]), float(z[c + "f"]), int(z[c + "width"]), int(z[c + "height"]))
    cam.position = z[c + "position"]
    return cam


def _run(z, case, **cfg):
    from tinysplat_amd.extract import ExtractConfig, level_set_points
    c = case + "_"
    model = _model({k: z[k] for k in EO.PARAMS})
    ids = torch.from_numpy(z[c + "idxs"].astype(np.int64))
    depth = torch.from_numpy(z[c + "depth"]).to(DEV)
    res, dbg = level_set_points(model, _camera(z, c), depth, ids, ExtractConfig(**cfg), return_debug=True)
    torch.cuda.synchronize()
    return res, dbg, ids


def _check_against_oracle(params, depth, view, proj, position, ids, res, dbg, convention, bars, label, cap=True):
    """The staged comparison; ``bars`` = (E_pw, E_d, E_pts, E_n) already multiplied by the factor."""
    b_pw, b_d, b_pts, b_n = bars
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in dbg.items()}
    for k, v in cpu.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
    args = (params, depth, view, proj, position, ids)
    e2e = EO.backproject(ids, depth, view, proj, convention)
    assert torch.equal(cpu["valid"], e2e[1])
    err_pw = (cpu["p_world"].double() - e2e[0])[e2e[1]].abs().max().item()
    o = EO.level_set_oracle(*args, convention=convention, given={"p_world": cpu["p_world"], "samples": cpu["samples"]},
                            with_normals=False)
    valid, stable = o["valid"], o["stable"]
    same_knn = (o["knn"] == cpu["knn"].long()).all(-1).all(-1)
    err_nearest = int((o["nearest"] != cpu["nearest"].long())[valid].sum())
    # the sample positions themselves: float32 rounding of p_world + (lin * p_std) * dir
    rebuilt = EO.level_set_oracle(*args, convention=convention, given={"p_world": cpu["p_world"]}, with_normals=False)
    err_samples = (cpu["samples"].double() - rebuilt["samples"])[valid].abs().max().item()
    b_samples = 2.0 * float(np.spacing(np.float32(cpu["samples"][valid].abs().max().item())))
    err_d = (cpu["density"].double() - o["density"])[valid & stable].abs().max().item()
    keep, first = cpu["keep"], cpu["first"].long()
    unstable = 1.0 - stable.double().mean().item()
    kept = keep.double().mean().item()
    both = stable & keep & o["keep"] & (first == o["first"])
    m = ids.shape[0]
    pts, t = torch.zeros(m, 3), torch.zeros(m)
    pts[keep], t[keep] = res.points.cpu(), res.t.cpu()
    err_pts = (pts.double() - o["points"])[both].abs().max().item()
    err_t = (t.double() - o["t"])[both].abs().max().item()
    p = {k: torch.as_tensor(params[k]).double() for k in EO.PARAMS}
    gp = res.points.cpu()
    n64 = EO.normals(gp.double(), EO.exact_knn(gp, p["means"]), p)
    sel = both[keep]
    err_n = (res.normals.cpu().double() - n64)[sel].abs().max().item()
    print(f"\n[{label}] rays {m} kept {kept:.4f} unstable {unstable:.4f} | p_world {err_pw:.3e} (bar {b_pw:.3e}) "
          f"samples {err_samples:.3e} (bar {b_samples:.3e}) density {err_d:.3e} (bar {b_d:.3e}) points {err_pts:.3e} t {err_t:.3e} "
          f"(bar {b_pts:.3e}) normals {err_n:.3e} (bar {b_n:.3e}) | knn rows differing "
          f"{int((~same_knn & valid).sum())} nearest differing {err_nearest}")
    assert not cap or (unstable <= 0.02 and kept >= 0.5)      # the cap on a fixture case
    assert err_pw <= b_pw
    assert err_nearest == 0 and bool(same_knn[valid].all())
    assert err_samples <= b_samples
    assert err_d <= b_d
    assert torch.equal(keep[stable], o["keep"][stable])
    assert torch.equal(first[stable & keep], o["first"][stable & keep])
    assert not keep[~valid].any()
    assert err_pts <= b_pts and err_t <= b_pts
    assert err_n <= b_n
    nl = res.normals.norm(dim=-1).cpu()
    assert bool(((nl - 1).abs() < 1e-5).logical_or(nl == 0).all())
    # the result is the survivors in ray order
    assert torch.equal(res.pixel.cpu(), ids[keep]) and res.points.shape == (int(keep.sum()), 3)
    for v in (res.points, res.normals, res.t):
        assert torch.isfinite(v).all()
    return o


def _bars(z, cases):
    return tuple(FACTOR * max(float(z[c + "_" + k]) for c in cases) for k in ("E_pw", "E_d", "E_pts", "E_n"))


@pytest.mark.parametrize("case,convention", [("square", "reference"), ("wide", "reference"), ("posed", "reference"),
                                             ("wide", "screen"), ("square", "screen")])
def test_level_set_points_match_the_oracle(case, convention):
    z = _z()
    c = case + "_"
    res, dbg, ids = _run(z, case, pixel_convention=convention)
    o = _check_against_oracle({k: z[k] for k in EO.PARAMS}, z[c + "depth"], z[c + "view_matrix"], z[c + "proj_matrix"],
                              z[c + "position"], ids, res, dbg, convention, _bars(z, (case,)), f"{case}/{convention}")
    if convention == "reference":
        # against the reference's own run: identical decisions on rays both call stable
        keep_ref, first_ref = torch.from_numpy(z[c + "keep"]), torch.from_numpy(z[c + "first"]).long()
        pw_ref = torch.from_numpy(z[c + "p_world"])
        ref = EO.level_set_oracle({k: z[k] for k in EO.PARAMS}, z[c + "depth"], z[c + "view_matrix"],
                                  z[c + "proj_matrix"], z[c + "position"], ids, given={"p_world": pw_ref},
                                  with_normals=False)
        both = ref["stable"] & o["stable"] & (ref["margin"] > 1e-2) & (o["margin"] > 1e-2)
        agree = (dbg["keep"].cpu() == keep_ref) & (~keep_ref | (dbg["first"].cpu().long() == first_ref))
        print(f"[{case}] decisions differing from the reference on rays with margin > 1e-2: {int((~agree & both).sum())}"
              f" of {int(both.sum())}")
        # zero-depth pixels: no points, here and there
        zero = torch.from_numpy(z[c + "depth"]).reshape(-1)[ids] <= 0
        assert int(zero.sum()) == 60 and not dbg["keep"].cpu()[zero].any() and not keep_ref[zero].any()
        assert not torch.isin(res.pixel.cpu(), ids[zero]).any()
    if case == "square" and convention == "screen":
        ref_run, _, _ = _run(z, case, pixel_convention="reference")
        assert torch.equal(ref_run.points, res.points) and torch.equal(ref_run.normals, res.normals)


def test_conventions_differ_on_a_non_square_image():
    z = _z()
    a, da, _ = _run(z, "wide", pixel_convention="reference")
    b, db, _ = _run(z, "wide", pixel_convention="screen")
    assert not torch.equal(da["p_world"], db["p_world"])
    assert a.points.shape[0] > 0 and b.points.shape[0] > 0


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("points", "normals", "camera", "pixel", "t"))


def test_runs_are_bit_identical_and_independent_of_the_chunk_size():
    from tinysplat_amd import _lib
    z = _z()
    one, d1, _ = _run(z, "square")
    two, d2, _ = _run(z, "square")
    assert d1["chunks"] == 1 and _same(one, two)
    for k in ("samples", "knn", "density", "p_world", "first", "keep"):
        assert torch.equal(d1[k], d2[k]), k
    cap = int(_lib.load().ts_extract_chunk_bytes(int(z["means"].shape[0]), 900, 21))
    small, d3, _ = _run(z, "square", max_workspace_bytes=cap)
    print(f"\nchunks with a {cap} byte cap: {d3['chunks']}")
    assert d3["chunks"] >= 4 and _same(one, small)
    for k in ("samples", "knn", "density", "p_world", "first", "keep"):
        assert torch.equal(d1[k], d3[k]), k
    with pytest.raises(ValueError):
        _run(z, "square", max_workspace_bytes=1024)
    plain, _, _ = _run(z, "square", normals=False)
    assert plain.normals is None and torch.equal(plain.points, one.points)


def _sphere_scene(n=6000, radius=0.9, centre=(0.0, 0.0, 3.0), seed=5):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    means = torch.tensor(centre) + radius * d
    # the rotation that takes the local z axis to the radial direction: q = (1 + z.d, z x d) normalised
    zc = torch.tensor([0.0, 0.0, 1.0]).expand(n, 3)
    quats = torch.cat(((1 + d[:, 2:3]), torch.cross(zc, d, dim=-1)), 1)
    quats = torch.where(quats.norm(dim=-1, keepdim=True) < 1e-4, torch.tensor([0.0, 1.0, 0.0, 0.0]).expand(n, 4), quats)
    scales = torch.log(torch.cat((0.04 + 0.02 * torch.rand(n, 2, generator=g), 0.012 + 0.004 * torch.rand(n, 1, generator=g)), 1))
    opac = 2.0 + 0.5 * torch.randn(n, 1, generator=g)
    return {"means": means, "scales": scales, "quats": quats, "opacities": opac}, torch.tensor(centre), radius


def test_extract_surface_points_end_to_end_on_a_sphere():
    from tinysplat_amd import GaussianRasterizer
    from tinysplat_amd.extract import ExtractConfig, extract_surface_points, level_set_points
    from tinysplat_amd.synthetic import PinholeCamera
    z = _z()
    params, centre, radius = _sphere_scene()
    model = _model(params)
    model.background = torch.tensor([0.3, 0.2, 0.1], device=DEV)
    background = model.background
    q = np.array([0.99, 0.05, -0.12, 0.03])
    poses = [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)), ((0.4, -0.2, 0.1), tuple(q / np.linalg.norm(q)))]
    cams = []
    for pos, quat in poses:
        cam = PinholeCamera.look_at_origin_plus_z(128, 128, 40.0, position=pos, quat=quat, znear=0.2, zfar=20.0)
        cam.position = np.asarray(pos, dtype=np.float64)
        cams.append(cam)
    cfg = ExtractConfig(num_total_points=6000)
    res = extract_surface_points(model, cams, cfg, device=DEV, generator=torch.Generator().manual_seed(9))
    torch.cuda.synchronize()
    assert model.background is background               # restored
    for v in (res.points, res.normals, res.t):
        assert torch.isfinite(v).all()
    assert res.points.shape[0] > 1000 and set(res.camera.cpu().tolist()) == {0, 1}
    assert bool((res.camera[1:] >= res.camera[:-1]).all())
    # the same rendered depth, the same pixels: the core reproduces the public entry, and the oracle the core
    g = torch.Generator().manual_seed(9)
    model.background = torch.zeros(3, device=DEV)
    with torch.no_grad():
        render = GaussianRasterizer(model, cams, device=torch.device(DEV))
        bars = _bars(z, ("square", "wide", "posed"))    # the same binade of coordinates (|x| < 4) as the fixture's
        for ci, cam in enumerate(cams):
            depth = render(cam)[1]["depth"]
            ids = torch.randperm(128 * 128, generator=g)[:3000]
            part, dbg = level_set_points(model, cam, depth, ids, cfg, return_debug=True, camera_index=ci)
            mine = res.camera == ci
            assert torch.equal(res.points[mine], part.points) and torch.equal(res.pixel[mine], part.pixel)
            assert torch.equal(res.normals[mine], part.normals) and torch.equal(res.t[mine], part.t)
            _check_against_oracle(params, depth.cpu().numpy(), cam.view_matrix.numpy(), cam.proj_matrix.numpy(),
                                  cam.position, ids, part, dbg, "reference", bars, f"sphere camera {ci}", cap=False)
    model.background = background
    # recorded, not asserted: how well the level set follows the analytic sphere
    rel = res.points.cpu().double() - centre.double()
    dist = rel.norm(dim=-1) - radius
    nl = res.normals.cpu().double()
    cosang = (nl * rel / rel.norm(dim=-1, keepdim=True)).sum(-1).clamp(-1, 1)
    ang = torch.rad2deg(torch.acos(cosang[nl.norm(dim=-1) > 0]))
    print(f"\nsphere: {res.points.shape[0]} points; distance to the sphere mean {dist.mean().item():+.4f} "
          f"|max| {dist.abs().max().item():.4f}; angle normal / radius median {ang.median().item():.2f} deg "
          f"p95 {ang.quantile(0.95).item():.2f} deg")


def test_full_size_run_respects_the_workspace_cap():
    from tinysplat_amd import GaussianRasterizer
    from tinysplat_amd.extract import ExtractConfig, extract_surface_points, level_set_points, pack_model
    from tinysplat_amd.synthetic import PinholeCamera, make_scene
    n, w, h = 1_000_000, 1920, 1080
    model, _ = make_scene(n, 0, w, h, seed=0, scale_mult=4.0, opacity_logit_mean=2.0)
    model = model.to(DEV)
    cams = []
    for i in range(4):
        pos = (0.05 * i, -0.03 * i, 0.0)
        cam = PinholeCamera.look_at_origin_plus_z(w, h, position=pos)
        cam.position = np.asarray(pos, dtype=np.float64)
        cams.append(cam)
    cfg = ExtractConfig()
    mib = 2.0 ** 20
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    # the frame's own buffers: a rasterizer keeps one frame's buffers while it allocates the next one's
    frame = 0
    with torch.no_grad():
        render = GaussianRasterizer(model, cams, device=torch.device(DEV))
        for cam in cams + cams[:1]:
            torch.cuda.reset_peak_memory_stats()
            out = render(cam)
            torch.cuda.synchronize()
            frame = max(frame, torch.cuda.max_memory_allocated() - base)
        # the core on one camera's depth: everything it allocates beyond what it returns stays under the cap
        rays = cfg.num_total_points // 4
        ids = torch.randperm(h * w, generator=torch.Generator().manual_seed(1))[:rays]
        pk = pack_model(model)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        one = level_set_points(model, cams[0], out[1]["depth"], ids, cfg, packed=pk)
        torch.cuda.synchronize()
        core = torch.cuda.max_memory_allocated() - before
    got = one.points.shape[0] * (12 + 12 + 4 + 8 + 4)
    # beyond the workspace: the pixel indices on the device, the returned tensors and their per-chunk parts
    # before the final concatenation, the per-chunk survivor indices
    core_bound = cfg.max_workspace_bytes + rays * 8 + 2 * got + (8 << 20)
    print(f"\nfull size, one camera: {one.points.shape[0]} points of {rays} rays; peak {core / mib:.1f} MiB over the "
          f"state before the call (bound {core_bound / mib:.1f}: cap {cfg.max_workspace_bytes / mib:.0f} MiB)")
    assert core <= core_bound
    del out, one, pk, render
    torch.cuda.reset_peak_memory_stats()
    res = extract_surface_points(model, cams, cfg, device=DEV, generator=torch.Generator().manual_seed(1))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    p = res.points.shape[0]
    result = p * (12 + 12 + 4 + 8 + 4)
    pack = n * 44                                       # records and p_std (the model's means are contiguous: no copy)
    # term by term, as for one camera: the frame, the workspace, the packed records, the returned tensors twice
    # (every camera's parts, then their concatenation), one camera's pixel indices on the device, and the same 8 MiB
    # for the per-chunk survivor indices
    bound = frame + cfg.max_workspace_bytes + pack + 2 * result + rays * 8 + (8 << 20)
    print(f"full size: {p} points of {cfg.num_total_points} rays; peak {peak / mib:.1f} MiB over the model; frame "
          f"{frame / mib:.1f} MiB, cap {cfg.max_workspace_bytes / mib:.0f} MiB, packed {pack / mib:.1f} MiB, "
          f"result {result / mib:.1f} MiB; bound {bound / mib:.1f} MiB")
    assert res.pixel.shape == (p,) and torch.isfinite(res.points).all() and torch.isfinite(res.normals).all()
    assert math.isfinite(peak) and peak <= bound
