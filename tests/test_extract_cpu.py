"""The level-set surface extraction without a GPU: the float64 restatement (tests/extract_oracle.py) against the
reference's own run (tests/golden/extract_points.npz), the analytic normal against autograd, the camera's
back-projection and projection, the PLY round trip, the configuration defaults and the C-ABI argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import extract_oracle as EO
from helpers import GOLD

CASES = ("square", "wide", "posed")


def _z():
    return np.load(GOLD / "extract_points.npz")


def _params(z):
    return {k: z[k] for k in EO.PARAMS}


def _args(z, c):
    return (_params(z), z[c + "depth"], z[c + "view_matrix"], z[c + "proj_matrix"], z[c + "position"],
            z[c + "idxs"].astype(np.int64))


@pytest.mark.parametrize("case", CASES)
def test_pixels_are_the_seeded_permutation(case):
    z = _z()
    c = case + "_"
    g = torch.Generator().manual_seed(int(z[c + "seed"]))
    hw = int(z[c + "height"]) * int(z[c + "width"])
    assert np.array_equal(torch.randperm(hw, generator=g).numpy(), z[c + "idxs"])


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_reference(case):
    """Back-projection end to end; decisions, points and densities stage by stage on the reference's float32 values."""
    z = _z()
    c = case + "_"
    e2e = EO.level_set_oracle(*_args(z, c), with_normals=False)
    pw = torch.from_numpy(z[c + "p_world"])
    valid = e2e["valid"]
    assert torch.equal(valid, torch.isfinite(pw).all(-1)) and int((~valid).sum()) == 60     # the zero-depth patch
    assert (pw.double() - e2e["p_world"])[valid].abs().max().item() <= float(z[c + "E_pw"]) * (1 + 1e-9)
    o = EO.level_set_oracle(*_args(z, c), given={"p_world": pw}, with_normals=False)
    stable = o["stable"]
    keep, first = torch.from_numpy(z[c + "keep"]), torch.from_numpy(z[c + "first"]).long()
    m = keep.shape[0]
    assert 1.0 - stable.double().mean().item() <= 0.02 and keep.double().mean().item() >= 0.5
    assert torch.equal(o["keep"][stable], keep[stable])
    assert torch.equal(o["first"][stable & keep], first[stable & keep])
    assert not keep[~valid].any()
    both = stable & keep
    p_full = torch.zeros(m, 3, dtype=torch.float64)
    p_full[keep] = torch.from_numpy(z[c + "p_intersects"])
    # (the points are compared below, where the reference's own float32 samples are stored: rebuilt float64 samples
    # differ from them by float32 rounding, which the level crossing amplifies by an unbounded 1 / (d_a - d_b))
    # on the stored subset, exactly the reference's samples and neighbours
    s, k = int(z["sample_stride"]), int(z["knn_stride"])
    a = list(_args(z, c))
    a[5] = a[5][::s]
    sub = EO.level_set_oracle(*a, given={"p_world": pw[::s], "samples": z[c + "samples"]}, with_normals=False)
    vk = sub["valid"][::k // s].numpy()               # the neighbours of a NaN sample mean nothing
    assert np.array_equal(sub["knn"][::k // s].numpy()[vk], z[c + "knn"].astype(np.int64)[vk])
    rows = sub["stable"] & sub["valid"]
    assert (torch.from_numpy(z[c + "density"]).double() - sub["density"])[rows].abs().max().item() <= float(z[c + "E_d"])
    sb = rows & keep[::s] & (sub["first"] == first[::s])
    assert (p_full[::s] - sub["points"])[sb].abs().max().item() <= float(z[c + "E_pts"]) * (1 + 1e-9)
    assert torch.equal(sub["keep"][rows], keep[::s][rows])


@pytest.mark.parametrize("case", CASES)
def test_float32_restatement_takes_the_same_decisions(case):
    z = _z()
    c = case + "_"
    pw = torch.from_numpy(z[c + "p_world"])
    o64 = EO.level_set_oracle(*_args(z, c), given={"p_world": pw}, with_normals=False)
    o32 = EO.level_set_oracle(*_args(z, c), given={"p_world": pw, "knn": o64["knn"]}, dtype=torch.float32,
                              with_normals=False)
    st = o64["stable"]
    assert torch.equal(o32["keep"][st], o64["keep"][st])
    assert torch.equal(o32["first"][st & o64["keep"]], o64["first"][st & o64["keep"]])


def test_pixel_conventions():
    """The reference pairs x = f % H, y = f // H with the depth of (row f // W, column f % W); the two conventions
    agree on square images of even size and differ elsewhere.  ``extract.pixel_ndc`` (the package's statement of
    what csrc/extract.hip computes) equals the oracle's."""
    from tinysplat_amd.extract import pixel_ndc
    for hh, ww in ((64, 64), (48, 64), (5, 7)):
        f = torch.arange(hh * ww)
        for conv in ("reference", "screen"):
            for a, b in zip(pixel_ndc(f, hh, ww, conv), EO.pixel_ndc(f, hh, ww, conv, torch.float64)):
                assert a.dtype == torch.float64 and torch.equal(a, b)
    with pytest.raises(ValueError):
        pixel_ndc(torch.arange(4), 2, 2, "ndc")
    ids = torch.arange(64 * 64)
    for a, b in zip(EO.pixel_ndc(ids, 64, 64, "reference", torch.float64), EO.pixel_ndc(ids, 64, 64, "screen", torch.float64)):
        assert torch.allclose(a, b, rtol=0, atol=1e-15)
    ids = torch.arange(48 * 64)
    rx, ry = EO.pixel_ndc(ids, 48, 64, "reference", torch.float64)
    sx, _ = EO.pixel_ndc(ids, 48, 64, "screen", torch.float64)
    assert not torch.allclose(rx, sx)
    f = 100                                             # H = 48, W = 64: x = 100 % 48 = 4, y = 100 // 48 = 2
    assert rx[f].item() == (4 + 0.5 - 32) / 48 * 2 and ry[f].item() == (2 + 0.5 - 24) / 64 * 2
    assert sx[f].item() == (100 % 64 + 0.5 - 32) * 2 / 64


def test_analytic_normal_is_autograd_of_the_density():
    z = _z()
    p = {k: torch.from_numpy(z[k]).double() for k in EO.PARAMS}
    pts = torch.from_numpy(z["square_p_intersects"])[::7].clone().requires_grad_(True)
    knn = EO.exact_knn(pts.detach(), p["means"])
    d, raw = EO.density(pts, knn, p)
    (g,) = torch.autograd.grad(raw.sum(), pts)
    n = EO.normals(pts.detach(), knn, p)
    want = -g / g.norm(dim=-1, keepdim=True)
    assert (raw <= 1).all()
    assert (n - want).abs().max().item() < 1e-12
    assert (n.norm(dim=-1) - 1).abs().max().item() < 1e-12
    # central differences of the density itself
    eps = 1e-6
    fd = torch.stack([(EO.density(pts.detach() + eps * e, knn, p)[1] - EO.density(pts.detach() - eps * e, knn, p)[1])
                      / (2 * eps) for e in torch.eye(3, dtype=torch.float64)], -1)
    assert (fd - g).abs().max().item() < 1e-6 * g.abs().max().item()
    # a clamped point (on a mean of an opaque cluster) gets a zero normal
    dense = dict(p, opacities=torch.full_like(p["opacities"], 8.0))
    at = p["means"][:5].clone()
    assert (EO.density(at, EO.exact_knn(at, p["means"]), dense)[1] > 1).all()
    assert torch.equal(EO.normals(at, EO.exact_knn(at, p["means"]), dense), torch.zeros(5, 3, dtype=torch.float64))


def _camera(z, c):
    from tinysplat_amd.synthetic import PinholeCamera
    cam = PinholeCamera(torch.from_numpy(z[c + "view_matrix"]), torch.from_numpy(z[c + "proj_matrix"]),
                        float(z[c + "f"]), float(z[c + "f"]), int(z[c + "width"]), int(z[c + "height"]))
    cam.position = z[c + "position"]
    return cam


@pytest.mark.parametrize("case", CASES)
def test_camera_backprojection_and_projection_match_the_reference(case):
    z = _z()
    c = case + "_"
    cam = _camera(z, c)
    h, w = cam.height, cam.width
    ids = torch.from_numpy(z[c + "idxs"].astype(np.int64))
    depth = torch.from_numpy(z[c + "depth"]).reshape(-1)[ids]
    p3 = torch.stack([(ids % h).float(), (ids // h).float(), depth], dim=-1)
    got, want = cam.backproject_points(p3), torch.from_numpy(z[c + "p_world"])
    ok = torch.isfinite(want).all(-1)
    assert torch.equal(torch.isfinite(got).all(-1), ok)
    assert (got - want)[ok].abs().max().item() <= 4e-6 * want[ok].abs().max().item()     # a few float32 ulps
    pts = torch.from_numpy(z[c + "p_intersects"]).float()[::4]
    assert torch.allclose(cam.project_points(pts), torch.from_numpy(z[c + "projected"]), rtol=1e-5, atol=1e-4)
    assert torch.allclose(cam.project_points(pts, screen_coordinates=False, return_depth=True),
                          torch.from_numpy(z[c + "projected_ndc_depth"]), rtol=1e-5, atol=1e-6)
    from tinysplat_amd.extract import camera_position
    derived = _camera(z, c)
    del derived.position
    assert np.abs(camera_position(derived) - z[c + "position"]).max() < 1e-6
    assert np.array_equal(camera_position(cam), z[c + "position"])


def test_points_ply_round_trip(tmp_path):
    from tinysplat_amd.extract import SurfacePoints
    from tinysplat_amd.formats import export_points_ply, read_points_ply
    from tinysplat_amd.init import read_point_cloud_ply
    g = torch.Generator().manual_seed(3)
    pts, nrm = torch.randn(37, 3, generator=g), torch.nn.functional.normalize(torch.randn(37, 3, generator=g), dim=-1)
    sp = SurfacePoints(pts, nrm, torch.zeros(37, dtype=torch.int32), torch.arange(37), torch.zeros(37))
    export_points_ply(sp, tmp_path / "s.ply")
    blob = (tmp_path / "s.ply").read_bytes()
    assert blob.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n")
    assert len(blob) == blob.find(b"end_header\n") + 11 + 37 * 24
    p2, n2 = read_points_ply(tmp_path / "s.ply")
    assert torch.equal(p2, pts) and torch.equal(n2, nrm)
    export_points_ply(SurfacePoints(pts, None, sp.camera, sp.pixel, sp.t), tmp_path / "z.ply")
    assert torch.equal(read_points_ply(tmp_path / "z.ply")[1], torch.zeros(37, 3))
    export_points_ply(SurfacePoints(pts[:0], nrm[:0], sp.camera[:0], sp.pixel[:0], sp.t[:0]), tmp_path / "e.ply")
    assert read_points_ply(tmp_path / "e.ply")[0].shape == (0, 3)
    with pytest.raises(ValueError):                     # the SfM reader still insists on colours
        read_point_cloud_ply(tmp_path / "s.ply")
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        read_points_ply(tmp_path / "bad.ply")


def test_config_defaults_are_the_reference_literals():
    from tinysplat_amd.extract import EXTRACT_K, ExtractConfig
    z = _z()
    c = ExtractConfig()
    assert c.surface_level == float(z["default_surface_level"]) == 0.3
    assert c.num_total_points == int(z["default_num_total_points"]) == 2_000_000
    assert c.num_steps == int(z["default_num_steps"]) == 21
    assert c.extent_sigmas == float(z["default_extent_sigmas"]) == 3.0
    assert EXTRACT_K == int(z["default_neighbours"]) == 16
    assert (c.pixel_convention, c.normals, c.max_workspace_bytes) == ("reference", True, 256 << 20)
    assert float(z["delta"]) == EO.DELTA
    for bad in (dict(pixel_convention="ndc"), dict(num_steps=1), dict(num_steps=65), dict(extent_sigmas=0.0),
                dict(num_total_points=0), dict(max_workspace_bytes=0)):
        with pytest.raises(ValueError):
            ExtractConfig(**bad)


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    bad = -1
    p = ctypes.c_void_p(16)
    cam = (ctypes.c_float * 21)(*([1.0] * 21))
    nan_cam = (ctypes.c_float * 21)(*([1.0] * 20 + [float("nan")]))

    def each(fn, args, cases):
        for i, v in cases:
            a = list(args)
            a[i] = v
            assert fn(*a) == bad, (fn.__name__, i, v)

    each(lib.ts_extract_pack, [20, p, p, p, p, p, p, None], [(0, 0)] + [(i, None) for i in range(1, 7)])
    each(lib.ts_extract_rays, [8, p, 48, 64, p, 0, cam, p, p, p, p, None],
         [(0, 0), (2, 0), (3, 0), (5, 2), (5, -1), (6, nan_cam)] + [(i, None) for i in (1, 4, 6, 7, 8, 9, 10)])
    a = [8, p, 65536, 65536, p, 0, cam, p, p, p, p, None]                  # H * W >= 2^31
    assert lib.ts_extract_rays(*a) == bad
    each(lib.ts_extract_samples, [20, 8, 21, 3.0, p, p, p, p, p, p, None],
         [(0, 0), (1, 0), (2, 1), (2, 65), (3, 0.0), (3, float("inf")), (1, 2 ** 31 // 21 + 1)]
         + [(i, None) for i in range(4, 10)])
    each(lib.ts_extract_march, [20, 8, 21, 3.0, 0.3, p, p, p, p, p, p, p, p, p, p, p, None, None],
         [(0, 0), (1, 0), (2, 1), (2, 65), (3, -1.0), (4, float("nan")), (1, 2 ** 31 // 21 + 1)]
         + [(i, None) for i in range(5, 16)])
    each(lib.ts_extract_normals, [20, 8, p, p, p, p, None], [(0, 0), (1, 0)] + [(i, None) for i in range(2, 6)])
    for n, rays, steps in ((15, 8, 21), (20, 0, 21), (20, 8, 1), (20, 8, 65), (20, 2 ** 31 // 21 + 1, 21)):
        assert lib.ts_extract_chunk_bytes(n, rays, steps) == bad
    one, two = lib.ts_extract_chunk_bytes(2000, 1000, 21), lib.ts_extract_chunk_bytes(2000, 2000, 21)
    assert 0 < one < two and one >= lib.ts_knn_ws_bytes(2000, 21000, 16) + 1000 * 21 * (12 + 128)
    assert lib.ts_abi_version() == 9


def test_extraction_refuses_cpu_tensors_and_small_models():
    from tinysplat_amd.extract import extract_surface_points, level_set_points, pack_model
    from tinysplat_amd.synthetic import make_scene
    model, cam = make_scene(40, 0, 32, 32, seed=1)
    with pytest.raises(RuntimeError):
        pack_model(model)
    with pytest.raises(RuntimeError):
        level_set_points(model, cam, torch.ones(32, 32), torch.arange(8))
    with pytest.raises(ValueError):
        extract_surface_points(model, [])
