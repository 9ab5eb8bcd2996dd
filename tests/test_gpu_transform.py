"""Scene editing on the GPU (csrc/transform.hip): ts_transform_gaussians against the float64 oracle
under the bounds of tests/transform_cases.py and bit for bit against the g++ build of csrc/transform_math.h, at partial
and exact waves, several workgroups and every k_rest instantiation, in place, masked and twice; the box mask against numpy's
float32 expression; the merge; the render invariance through GaussianRasterizer; the guards."""
import ctypes

import numpy as np
import pytest
import torch

import transform_cases as TC
from helpers import scene_args
from tinysplat_amd import GaussianRasterizer, _lib, edit
from tinysplat_amd.semantic import select_gaussians
from tinysplat_amd.synthetic import SplatModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32P = ctypes.POINTER(ctypes.c_float)
SIZES = [(n, 3) for n in (0, 1, 63, 64, 65, 257, 2000)] + [(257, d) for d in (0, 1, 2, 4)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TC.build_host(tmp_path_factory.mktemp("transform"))


def scene_of(n, degree):
    """The edge rows ride along wherever the scene has room for them (n = 257: at both ends and across row 64)."""
    return TC.with_edges(n, degree, seed=n + degree) if n >= 3 * TC.EDGE_ROWS else TC.random_scene(n, degree, seed=n + degree)


def launch(scene, args, mask=None, in_place=False):
    """ts_transform_gaussians on device copies of a scene's arrays -> dict of float32 numpy arrays."""
    xform, quat, log_scale, sh = args[:4]
    src = {f: torch.from_numpy(scene[f]).to(DEV) for f in TC.FIELDS}
    out = src if in_place else {f: torch.full_like(src[f], 7.0) for f in TC.FIELDS}
    n, kr = scene["means"].shape[0], scene["rest"].shape[1]
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    sh = np.ascontiguousarray(sh, dtype=np.float32)
    code = _lib.load().ts_transform_gaussians(
        n, kr, xform.ctypes.data_as(F32P), quat.ctypes.data_as(F32P), log_scale, sh.ctypes.data_as(F32P) if sh.size else None,
        None if m is None or n == 0 else m.data_ptr(), *[ptr(src[f]) for f in TC.FIELDS], *[ptr(out[f]) for f in TC.FIELDS],
        torch.cuda.current_stream(DEV).cuda_stream)
    assert code == 0
    torch.cuda.synchronize()
    return {f: out[f].cpu().numpy() for f in TC.FIELDS}


@pytest.mark.parametrize("n,degree", SIZES)
def test_transform_is_the_host_builds_bits_and_within_the_oracles_bounds(host, n, degree):
    scene = scene_of(n, degree)
    args = TC.arguments(TC.sim3(2.5), degree)
    want = TC.host_transform(host, scene, *args[:4])
    got = launch(scene, args)
    for f in TC.FIELDS:
        assert TC.same_bits(got[f], want[f]), f
    worst = TC.check_against_oracle(got, scene, args[0], args[1], args[2], args[4])
    print(f"n = {n}, degree {degree}: worst error / bound {worst}")
    again, inplace = launch(scene, args), launch(scene, args, in_place=True)
    for f in TC.FIELDS:
        assert np.array_equal(TC.bits(again[f]), TC.bits(got[f])), f             # the same bits on every run
        assert np.array_equal(TC.bits(inplace[f]), TC.bits(got[f])), f           # out == in


@pytest.mark.parametrize("n,degree", [(2000, 3), (257, 4), (65, 0)])
def test_masks(host, n, degree):
    scene = scene_of(n, degree)
    args = TC.arguments(TC.sim3(0.4), degree)
    full = launch(scene, args)
    mask = np.random.default_rng(n).random(n) < 0.5
    part = launch(scene, args, mask)
    want = TC.host_transform(host, scene, *args[:4], mask)
    none, every = launch(scene, args, np.zeros(n, bool)), launch(scene, args, np.ones(n, bool), in_place=True)
    for f in TC.FIELDS:
        assert TC.same_bits(part[f], want[f]), f
        assert np.array_equal(TC.bits(part[f][~mask]), TC.bits(scene[f][~mask])), f   # masked-out rows: the input's bits
        assert np.array_equal(TC.bits(part[f][mask]), TC.bits(full[f][mask])), f
        assert np.array_equal(TC.bits(none[f]), TC.bits(scene[f])), f
        assert np.array_equal(TC.bits(every[f]), TC.bits(full[f])), f


def model_of(scene, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = scene["means"].shape[0]
    t = {f: torch.from_numpy(scene[f]).to(DEV) for f in TC.FIELDS}
    return SplatModel(t["means"], torch.randn((n, 3), generator=g).to(DEV), t["rest"], t["scales"], t["quats"],
                      torch.randn((n, 1), generator=g).to(DEV), active_sh_degree=min(degree, 2),
                      background=torch.tensor([0.1, 0.2, 0.3], device=DEV))


def test_transform_gaussians_builds_a_new_model(host):
    scene = scene_of(257, 3)
    model = model_of(scene, 3)
    t = TC.sim3(2.5)
    mask = torch.from_numpy(np.random.default_rng(5).random(257) < 0.3).to(DEV)
    for m in (None, mask):
        new = edit.transform_gaussians(model, t, m)
        want = TC.host_transform(host, scene, *TC.arguments(t, 3)[:4], None if m is None else m.cpu().numpy())
        for f, name in zip(TC.FIELDS, ("means", "scales", "quats", "colors_rest")):
            assert TC.same_bits(getattr(new, name).cpu().numpy(), want[f]), name
            assert getattr(new, name) is not getattr(model, name)
            assert np.array_equal(TC.bits(getattr(model, name).cpu().numpy()), TC.bits(scene[f])), name   # input not written
        assert new.colors_dc is model.colors_dc and new.opacities is model.opacities
        assert new.background is model.background and new.active_sh_degree == model.active_sh_degree == 2
    empty = edit.transform_gaussians(select_gaussians(model, torch.zeros(257, dtype=torch.bool, device=DEV)), t)
    assert empty.num_points == 0 and empty.colors_rest.shape == (0, 15, 3)
    with pytest.raises(ValueError, match="bool"):
        edit.transform_gaussians(model, t, mask.to(torch.uint8))
    with pytest.raises(ValueError, match="bool"):
        edit.transform_gaussians(model, t, mask[:-1])


def test_guards():
    model = model_of(scene_of(64, 1), 1)
    model.held_by = {"TrainStep"}
    with pytest.raises(RuntimeError, match="held by"):
        edit.transform_gaussians(model, TC.sim3())
    cpu = scene_args(10, 1, 16, 16)[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit.transform_gaussians(cpu, TC.sim3())
    model.held_by = set()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit.transform_gaussians(model, TC.sim3(), torch.ones(64, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ box, crop, merge
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_box_mask_is_numpys_float32_expression(host, n):
    scene = scene_of(n, 0)
    centre, half = np.array([0.5, -1.0, 0.25]), np.array([2.0, 4.0, 0.5])      # powers of two: A and b are exact
    rot = TC.sim3().rotation
    if n >= 12:
        local = np.array([[2.0, 0, 0], [-2.0, 4.0, 0.5], [0, 4.0, 0], [0, 0, -0.5], [2.000001, 0, 0], [0, 0, 0]])
        scene["means"][:6] = (centre + local).astype(np.float32)          # on a face, on a corner, just outside, the centre
        scene["means"][6] = (np.nan, 0, 0)
        scene["means"][7] = (0, np.inf, 0)
    model = model_of(scene, 0)
    for r in (None, rot):
        got = edit.box_mask(model, centre, half, r)
        assert got.dtype == torch.bool and got.shape == (n,)
        a = (np.eye(3) if r is None else r).T / half[:, None]
        box = np.concatenate([a.reshape(-1), -(a @ centre)]).astype(np.float32)
        a32, b32, m = box[:9].reshape(3, 3), box[9:], scene["means"]
        with np.errstate(all="ignore"):
            v = ((a32[None, :, 0] * m[:, None, 0] + a32[None, :, 1] * m[:, None, 1]) + a32[None, :, 2] * m[:, None, 2]) + b32
        want = (np.abs(v) <= 1).all(1)
        assert v.dtype == np.float32 and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(TC.host_box_mask(host, box, m), want)
        if n >= 12 and r is None:
            assert want[:4].all() and want[5] and not want[4] and not want[6] and not want[7]
        kept = edit.crop_gaussians(model, centre, half, r)
        idx = torch.from_numpy(np.flatnonzero(want)).to(DEV)
        for p, q in zip(kept.parameters(), model.parameters()):
            assert torch.equal(p.view(torch.int32), q[idx].view(torch.int32))   # the rows inside, in order (bits: NaN rows)
    if n == 2000:
        assert 0 < int(want.sum()) < n


def test_merge_mixed_degrees_and_render_of_two_halves():
    parts = [scene_args(n, d, 64, 48, seed=s, device=DEV)[0] for n, d, s in ((50, 0, 1), (70, 2, 2), (30, 3, 3))]
    m = edit.merge_models(parts)
    assert m.num_points == 150 and m.colors_rest.shape == (150, 15, 3) and m.active_sh_degree == 3
    assert torch.equal(m.colors_rest[50:120, :8], parts[1].colors_rest) and not m.colors_rest[50:120, 8:].any()
    assert not m.colors_rest[:50].any() and torch.equal(m.colors_rest[120:], parts[2].colors_rest)
    assert torch.equal(m.means, torch.cat([p.means for p in parts])) and m.background is parts[0].background
    with pytest.raises(ValueError, match="devices"):
        edit.merge_models([parts[0], scene_args(5, 0, 16, 16)[0]])
    # two disjoint halves of a scene, concatenated in the original order, render the scene's bits
    model, cam = scene_args(3000, 2, 160, 96, seed=4, scale_mult=3.0, device=DEV)
    first = torch.arange(3000, device=DEV) < 1400
    whole = edit.merge_models([select_gaussians(model, first), select_gaussians(model, ~first)])
    with torch.no_grad():
        rgb0, ex0 = GaussianRasterizer(model, [cam])(cam, (160, 96), 2)
        rgb1, ex1 = GaussianRasterizer(whole, [cam])(cam, (160, 96), 2)
    assert torch.equal(rgb0, rgb1) and torch.equal(ex0["depth"], ex1["depth"]) and rgb0.max() > 0.5


# ------------------------------------------------------------------------------------------------ render invariance
def _render(model, cam, **kw):
    with torch.no_grad():
        rgb, extras = GaussianRasterizer(model, [cam], **kw)(cam, (cam.width, cam.height), model.active_sh_degree)
    return rgb.cpu(), extras["depth"].cpu()


@pytest.fixture(scope="module")
def reference_render():
    model, cam = scene_args(400, 3, 64, 48, seed=3, scale_mult=4.0, device=DEV)
    return model, cam, _render(model, cam, correct_viewdirs=True)


@pytest.mark.parametrize("s", TC.SCALES)
def test_render_is_invariant(reference_render, s):
    """The scene and the three transforms of tests/test_transform_cpu.py's oracle check through the kernels: rgb to 1e-3,
    depth' = s depth to 1e-3 max(1, s), with correct_viewdirs=True.  Measured on the MI355X: rgb 4.1e-6 / 6.4e-6 / 2.1e-5
    and depth 4.1e-5 / 9.9e-5 / 3.0e-5 for s = 1 / 2.5 / 0.4; the SH left unrotated: 0.39."""
    model, cam, (rgb0, depth0) = reference_render
    t = TC.sim3(s)
    moved, moved_cam = edit.transform_gaussians(model, t), edit.transform_camera(cam, t)
    rgb, depth = _render(moved, moved_cam, correct_viewdirs=True)
    plain = SplatModel(moved.means, moved.colors_dc, model.colors_rest, moved.scales, moved.quats, moved.opacities,
                       active_sh_degree=3, background=model.background)
    unrotated = (_render(plain, moved_cam, correct_viewdirs=True)[0] - rgb0).abs().max().item()
    e_rgb, e_depth = (rgb - rgb0).abs().max().item(), (depth - s * depth0).abs().max().item()
    print(f"s = {s}: rgb {e_rgb:.2e}, depth {e_depth:.2e}, with the SH left unrotated {unrotated:.2f}")
    assert e_rgb <= 1e-3 and e_depth <= 1e-3 * max(1.0, s)
    assert unrotated > 0.05


def test_degree_zero_is_invariant_through_the_default_rasterizer():
    model, cam = scene_args(400, 0, 64, 48, seed=3, scale_mult=4.0, device=DEV)
    rgb0, depth0 = _render(model, cam)
    for s in TC.SCALES:
        t = TC.sim3(s)
        rgb, depth = _render(edit.transform_gaussians(model, t), edit.transform_camera(cam, t))
        e_rgb, e_depth = (rgb - rgb0).abs().max().item(), (depth - s * depth0).abs().max().item()
        print(f"degree 0, s = {s}: rgb {e_rgb:.2e}, depth {e_depth:.2e}")
        assert e_rgb <= 1e-3 and e_depth <= 1e-3 * max(1.0, s)
    assert rgb0.max() > 0.5
