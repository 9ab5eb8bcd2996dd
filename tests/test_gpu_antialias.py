"""Antialiased rendering on the GPU: the three launches of csrc/antialias.hip against the host build
of their header bit for bit, the antialiased frame against the classic frame of the baked model and against the oracle,
training in the mode, the down-sampling case the mode exists for, and the PLY round trip."""
import numpy as np
import pytest
import torch

import antialias_cases as AC
import pose_cases as PC
from helpers import assert_close_masked, check_grad, scene_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-4           # threshold-stable pixels, as tests/test_gpu_parity.py takes them


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("antialias_gpu"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} entries differ, first at {bad[:5]}: "
                           f"{g[bad[:5]].view(np.float32)} against {w[bad[:5]].view(np.float32)}")


# ---- 4. the kernels against the host build
@pytest.mark.parametrize("logit", (True, False), ids=("logit", "opacity"))
@pytest.mark.parametrize("raw", (False, True), ids=("plain", "raw"))
@pytest.mark.parametrize("n", AC.KERNEL_SIZES)
def test_kernels_equal_the_host_build_bit_for_bit(host, n, raw, logit):
    """ts_antialias_fwd, ts_antialias_bwd and ts_compensation_bwd on a 50 x 35 image seen by a rotated camera: Gaussians
    behind the clip plane, off screen, beyond the fov clamp, of 0.05 px and with log-scales of -40 among ordinary ones,
    as prepared inputs or as log-scales and raw quaternions, with a logit or a plain opacity."""
    from tinysplat_amd import _lib, ops
    from tinysplat_amd.rasterizer import tile_bounds
    g = AC.kernel_gaussians(n, seed=n)
    view = AC.kernel_view().astype(np.float32)
    fx, fy, proj = PC.intrinsics(AC.KW, AC.KH)
    cam10 = AC.cam10(fx, fy, AC.KW, AC.KH)
    pflags = 3 if raw else 0
    rflags = _lib.RASTER_LOGIT_OPACITY if logit else 0
    scales, quats = (g["log_scales"], g["raw_quats"]) if raw else (g["scales"], g["quats"])
    opacity = g["logits"] if logit else (1.0 / (1.0 + np.exp(-g["logits"].astype(np.float64)))).astype(np.float32)
    means_d, scales_d, quats_d, op_d, view_d = (_dev(a) for a in (g["means"], scales, quats, opacity, view[:3, :]))
    cam = ops._camera(float(np.float32(fx)), float(np.float32(fy)), AC.KW / 2, AC.KH / 2, AC.KH, AC.KW,
                      tile_bounds((AC.KW, AC.KH)))
    lib = _lib.load()
    s = ops._stream(torch.device(DEV))
    f32 = dict(dtype=torch.float32, device=DEV)
    comp, o_eff, rows = torch.full((n,), 7.0, **f32), torch.full((n,), 7.0, **f32), torch.full((n, 4), 7.0, **f32)
    with torch.cuda.device(DEV):
        _lib.check(lib.ts_antialias_fwd(n, means_d.data_ptr(), scales_d.data_ptr(), quats_d.data_ptr(), view_d.data_ptr(),
                                        cam, pflags, op_d.data_ptr(), rflags, comp.data_ptr(), o_eff.data_ptr(),
                                        rows.data_ptr(), s), "ts_antialias_fwd")
    h_comp, h_oeff, h_rows = AC.host_fwd(host, g["means"], scales, quats, view, cam10, pflags, opacity, rflags)
    _same_bits(rows, h_rows, "rows")
    _same_bits(comp, h_comp, "comp")
    _same_bits(o_eff, h_oeff, "o_eff")
    assert ((h_comp >= 0) & (h_comp <= 1)).all()

    # the kinds are what they claim to be (every kind occurs from n = 63 on)
    projview = _dev((proj @ AC.kernel_view()).astype(np.float32))
    radii = ops.project_gaussians(means_d, scales_d, 1., quats_d, view_d, projview, float(np.float32(fx)), float(np.float32(fy)),
                                  AC.KW / 2, AC.KH / 2, AC.KH, AC.KW, tile_bounds((AC.KW, AC.KH)), log_scales=raw,
                                  raw_quats=raw)[2].cpu().numpy()
    p = g["means"].astype(np.float64) @ view[:3, :3].T.astype(np.float64) + view[:3, 3]
    kind = g["kind"]
    k = AC.KINDS.index
    if n >= 63:
        assert all((kind == j).sum() >= 8 for j in range(len(AC.KINDS)))
    assert (p[kind == k("behind"), 2] <= 0.01).all() and (h_comp[kind == k("behind")] == 0).all()
    assert (h_rows[kind == k("behind")] == 0).all()
    off = kind == k("off_screen")
    assert (radii[off] == 0).all() and (p[off, 2] > 0.01).all() and (h_comp[off] > 0).all()
    far = kind == k("beyond_fov")
    assert (np.abs(p[far, 0] / p[far, 2]) > 1.3 * 0.5 * AC.KW / fx).all() and (h_comp[far] > 0).all()
    sub = kind == k("sub_pixel")
    sig = np.sqrt(0.5 * (h_rows[sub, 0] + h_rows[sub, 2]))
    assert ((sig > 0.03) & (sig < 0.08)).all() and (h_comp[sub] > 0).all() and (h_comp[sub] < 0.05).all()
    under = kind == k("underflow")
    assert (h_comp[under] == 0).all() and (p[under, 2] > 0.01).all()
    if raw and n >= 63:
        assert (radii[under] > 0).any()          # drawn by the classic mode at the blur's size, invisible in this one

    # backward, in place: rows of culled Gaussians keep what they held
    rng = np.random.default_rng(n + 17)
    v_op = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 1, size=n)).astype(np.float32)
    v_conic = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 1, size=(n, 1))).astype(np.float32)
    v_op_d, v_conic_d, radii_d = _dev(v_op), _dev(v_conic), _dev(radii.astype(np.int32))
    with torch.cuda.device(DEV):
        _lib.check(lib.ts_antialias_bwd(n, radii_d.data_ptr(), rows.data_ptr(), op_d.data_ptr(), rflags,
                                        v_op_d.data_ptr(), v_conic_d.data_ptr(), s), "ts_antialias_bwd")
    h_vop, h_vconic = AC.host_bwd(host, radii, h_rows, opacity, rflags, v_op, v_conic)
    _same_bits(v_op_d, h_vop, "v_opacity")
    _same_bits(v_conic_d, h_vconic, "v_conic")
    culled = radii <= 0
    _same_bits(v_op_d.cpu().numpy()[culled], v_op[culled], "v_opacity of culled rows")
    _same_bits(v_conic_d.cpu().numpy()[culled], v_conic[culled], "v_conic of culled rows")
    assert np.isfinite(h_vop).all() and np.isfinite(h_vconic).all()
    clamped = (~culled) & (h_comp == 0)
    _same_bits(h_vconic[clamped], v_conic[clamped], "v_conic at the clamp")        # G = 0 exactly
    assert (h_vop[clamped] == 0).all()

    # the stand-alone op's backward launch
    v_comp = (rng.normal(size=n) * 10.0 ** rng.uniform(-2, 1, size=n)).astype(np.float32)
    outs = [torch.full((n, 3), 7.0, **f32), torch.full((n, 3), 7.0, **f32), torch.full((n, 4), 7.0, **f32)]
    v_comp_d = _dev(v_comp)
    with torch.cuda.device(DEV):
        _lib.check(lib.ts_compensation_bwd(n, means_d.data_ptr(), scales_d.data_ptr(), quats_d.data_ptr(),
                                           view_d.data_ptr(), cam, pflags, v_comp_d.data_ptr(),
                                           *[o.data_ptr() for o in outs], s), "ts_compensation_bwd")
    wants = AC.host_comp_bwd(host, g["means"], scales, quats, view, cam10, pflags, v_comp)
    for got, want, name in zip(outs, wants, ("v_means", "v_scales", "v_quats")):
        _same_bits(got, want, name)
        assert np.isfinite(want).all()
        assert (want[h_comp == 0] == 0).all()                  # the clamp and the clip plane: exact zeros
    if n >= 63:
        assert np.abs(wants[1]).max() > 0


def test_entries_refuse_bad_arguments():
    from tinysplat_amd import _lib
    lib = _lib.load()
    from tinysplat_amd import ops
    cam = ops._camera(10.0, 10.0, 8, 8, 16, 16, (1, 1, 1))
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = t.data_ptr()
    assert lib.ts_antialias_fwd(-1, p, p, p, p, cam, 0, p, 0, p, p, p, None) == -1
    assert lib.ts_antialias_fwd(0, None, None, None, None, cam, 0, None, 0, None, None, None, None) == 0
    assert lib.ts_antialias_fwd(4, p, p, p, p, cam, 4, p, 0, p, p, p, None) == -1          # unknown flag bits
    assert lib.ts_antialias_fwd(4, p, p, p, p, cam, 0, None, 0, None, p, None, None) == -1  # o_eff without an opacity
    assert lib.ts_antialias_fwd(4, p, p, p, p, cam, 0, p, 0, p, p, p + 4, None) == -1      # rows off 16 bytes
    assert lib.ts_antialias_fwd(4, p, p, p, p, cam, 0, None, 0, None, None, None, None) == -1
    assert lib.ts_antialias_bwd(4, p, p + 8, p, 0, p, p, None) == -1 and lib.ts_antialias_bwd(0, *([None] * 3), 0, None, None, None) == 0
    assert lib.ts_compensation_bwd(4, p, p, p + 4, p, cam, 0, p, p, p, p, None) == -1
    assert lib.ts_compensation_bwd(4, p, p, p, p, None, 0, p, p, p, p, None) == -1


# ---- 5. baked equivalence
def _baked_scene():
    """300 Gaussians seen at 64 x 48, degree 1: make_scene (scale_mult 3) shrunk to a tenth about the camera, so that depths
    lie in 0.2 .. 1 and an absolute bar means the same on the depth image as on the colours."""
    model, cam = scene_args(300, 1, 64, 48, seed=41, scale_mult=3.0)
    model.means = model.means * 0.1
    model.scales = model.scales + float(np.log(0.1))
    model.background = torch.tensor([0.1, 0.2, 0.3])
    return model, cam


def _bake(model, cam):
    """M' of M: the same model with opacities = logit(o_eff(M)) for ``cam`` (formed in double; o_eff = 0 -> -100, whose
    sigmoid is 0 in float32), classic mode."""
    from tinysplat_amd import ops
    view = cam.view_matrix.to(DEV)
    with torch.no_grad():
        o = ops.compensated_opacity(model, view[:3, :], cam.f_x, cam.f_y, cam.width, cam.height).double()
    logit = torch.where(o > 0, torch.log(o.clamp_min(1e-300) / (1.0 - o)), torch.full_like(o, -100.0))
    baked = model.to(DEV)
    baked.opacities = logit.to(torch.float32)
    baked.rasterize_mode = "classic"
    return baked, o


def test_antialiased_frame_is_the_classic_frame_of_the_baked_model():
    """For a fixed camera the antialiased frame of M equals the classic frame of M' with opacities = logit(o_eff(M)):
    identical radii and xys, image and depth within 1e-6 absolute - the sigmoid / logit round trip moves an opacity by a
    few ulps (<= 2e-7), and a pixel of this scene blends at most a few dozen Gaussians (the longest tile list is
    printed), few of them with a weight near 1.  Through render_frame_planes and render_view; the same 1e-6 for
    fusion.render_depth_alpha on alpha and on the composited depth sum over all pixels (and on the depth quotient the bar
    that follows from it, per pixel); semantic.gaussian_contributions within the relative bound derived below."""
    from tinysplat_amd import frame, fusion
    from tinysplat_amd.rasterizer import camera_on_device
    from tinysplat_amd.semantic import gaussian_contributions
    model, cam = _baked_scene()
    m = model.to(DEV)
    m.rasterize_mode = "antialiased"
    baked, o_eff = _bake(m, cam)
    assert ((o_eff > 0) & (o_eff < 1)).float().mean() > 0.7
    view, projview, origin = camera_on_device(cam, torch.device(DEV))
    args = (view[:3, :], projview, origin, cam.f_x, cam.f_y, cam.width, cam.height)
    with torch.no_grad():
        got = frame.render_frame_planes(m, *args)
        lists = frame.last_binning[0]
        longest = int((lists.tile_bins[:, 1] - lists.tile_bins[:, 0]).max())
        want = frame.render_frame_planes(baked, *args)
        got_v = frame.render_view(m, *args, True, planes=True)
        want_v = frame.render_view(baked, *args, True, planes=True)
        plain = frame.render_frame_planes(model.to(DEV), *args)
    print(f"longest tile list {longest}")
    assert longest <= 100
    for (rgb, depth, xys, radii), (rgb_w, depth_w, xys_w, radii_w), what in ((got, want, "planes"), (got_v, want_v, "view")):
        assert torch.equal(radii, radii_w) and torch.equal(xys, xys_w)
        e_rgb, e_d = (rgb - rgb_w).abs().max().item(), (depth - depth_w).abs().max().item()
        print(f"{what}: largest difference rgb {e_rgb:.3g}, depth {e_d:.3g}")
        assert e_rgb <= 1e-6 and e_d <= 1e-6
    assert torch.equal(got[0], got_v[0]) and torch.equal(got[1], got_v[1])
    assert (got[0] - plain[0]).abs().max().item() > 0.05            # the mode does something on this scene
    d, a = fusion.render_depth_alpha(m, cam)
    d_w, a_w = fusion.render_depth_alpha(baked, cam)
    # the same bar on what the pass composites, over ALL pixels: alpha, and the depth sum S = depth * alpha (depths <= 1)
    e_a = (a - a_w).abs().max().item()
    e_s = (d * a - d_w * a_w).abs().max().item()
    # ... and on the quotient it hands out, per pixel and without a cut-off: depth = S / alpha with S and alpha each within
    # 1e-6 moves by at most (1 + depth) 1e-6 / alpha; where alpha is 0 both depths are the 0 the function writes there
    seen = a_w > 0
    excess = ((d - d_w).abs() - (1.0 + d_w) * 1e-6 / a_w.clamp_min(1e-30))[seen].max().item()
    e_d = (d - d_w).abs().max().item()
    print(f"render_depth_alpha: largest difference alpha {e_a:.3g}, depth * alpha {e_s:.3g}, depth {e_d:.3g} "
          f"(smallest positive alpha {a_w[seen].min().item():.3g})")
    assert e_a <= 1e-6 and e_s <= 1e-6 and excess <= 0.0 and seen.any()
    assert torch.equal(a == 0, a_w == 0) and (d[~seen] == 0).all() and (d_w[~seen] == 0).all()
    votes, votes_w = gaussian_contributions(m, [cam]), gaussian_contributions(baked, [cam])
    # A vote is rint(2^24 w) of the weight w = alpha_g T_g a pixel blends Gaussian g with.  The vote walk of M packs the
    # torch product sigmoid(opacities) comp as a plain opacity, the very number M' is baked from; M' reproduces one that
    # votes (o_eff >= 1/255, so |logit| <= 5.6) to (1 - o) |logit| u <= 5.6 u for the float32 logit plus 4 u for the packing
    # stage's sigmoid, u = 2^-24: under 10 u = 6e-7, taken as 1e-6 RELATIVE.  alpha_g inherits that, T_g = prod (1 - alpha_j) over the blends in front moves by sum alpha_j / (1 - alpha_j)
    # times it, and 1 + sum alpha_j / (1 - alpha_j) <= prod 1 / (1 - alpha_j) <= K = 1 / (1 - largest alpha of the image).
    # So a Gaussian's votes move by at most 1e-6 K of themselves, plus one unit of 2^-24 for each of the at most
    # (2 r + 1)^2 pixels whose vote is rounded.
    K = 1.0 / (1.0 - a.max().item())
    pixels = (2.0 * got[3].double() + 1.0) ** 2
    bound = 1e-6 * K * votes_w + 2.0 ** -24 * pixels.to(votes.device)
    e_v = (votes - votes_w).abs()
    worst = (e_v / bound).max().item()
    print(f"gaussian_contributions: largest votes {votes_w.max().item():.3g}, largest difference {e_v.max().item():.3g}, "
          f"largest bound {bound.max().item():.3g} (K = {K:.3g}), worst difference / bound {worst:.3g}")
    assert votes.sum() > 1 and a.max().item() < 0.99 and (e_v <= bound).all()


# ---- 6. the frame and its gradients, three ways
_PARITY = {}


def _parity_reference():
    """The small parity scene of tests/test_gpu_parity.py (5000 Gaussians, degree 1, 200 x 120, scale_mult 4, seed 21; its
    per-axis scales span a factor 5 at most, so no Gaussian's axis ratio exceeds 10 and the conic's conditioning does not
    decide the outcome) through the oracle in the antialiased mode, once per session."""
    if not _PARITY:
        n, sh, w, h, mult = 5000, 1, 200, 120, 4.0
        model, cam = scene_args(n, sh, w, h, seed=21, scale_mult=mult)
        model.background = torch.tensor([0.2, 0.3, 0.1])
        ratio = torch.exp(model.scales.max(dim=1).values - model.scales.min(dim=1).values).max().item()
        assert ratio <= 10.0
        m_ref, _ = scene_args(n, sh, w, h, seed=21, scale_mult=mult)
        m_ref.background = model.background.clone()
        m_ref.requires_grad_(True)
        f = AC.oracle_render(m_ref, cam, (w, h), True)
        stable = f["aux"]["margin"] > MARGIN
        g = torch.Generator().manual_seed(1)
        w_rgb = torch.rand(h, w, 3, generator=g) * stable[..., None]
        w_d = torch.rand(h, w, generator=g) * stable
        ((f["rgb"] * w_rgb).sum() + (f["depth"] * w_d).sum()).backward()
        f = {k: (v.detach() if isinstance(v, torch.Tensor) and k != "xys" else v) for k, v in f.items()}
        _PARITY.update(model=model, cam=cam, ref=m_ref, frame=f, stable=stable, w_rgb=w_rgb, w_d=w_d, dims=(w, h), sh=sh)
    return _PARITY


def _run_adapter(P, fused, single_node):
    from tinysplat_amd.rasterizer import GaussianRasterizer
    md = P["model"].to(DEV).requires_grad_(True)
    md.rasterize_mode = "antialiased"
    r = GaussianRasterizer(md, None, device=torch.device(DEV), fused_colors=fused)
    r.single_node = single_node
    rgb, extras = r(P["cam"], P["dims"], P["sh"])
    ((rgb * P["w_rgb"].to(DEV)).sum() + (extras["depth"] * P["w_d"].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return md, rgb.detach(), extras


_NAMES = ("means", "scales", "quats", "opacities", "colors_dc", "colors_rest")


def test_antialiased_frame_and_gradients_match_the_oracle():
    """The one-node antialiased frame and its six gradients against the oracle with o_eff in place of the opacity, at the
    bars of tests/helpers.py as tests/test_gpu_parity.py applies them (1e-5 at threshold-stable pixels, check_grad)."""
    P = _parity_reference()
    f, stable = P["frame"], P["stable"]
    md, rgb, extras = _run_adapter(P, True, True)
    assert torch.equal(extras["radii"].cpu(), f["radii"])
    assert_close_masked(rgb, f["rgb"], 1e-5, stable, what="rgb")
    assert_close_masked(extras["depth"], f["depth"], 1e-5 * 10.0, stable, what="depth")     # depth values reach 10
    assert extras["xys"].grad is not None
    for nm in _NAMES:
        check_grad(nm, getattr(md, nm).grad, getattr(P["ref"], nm).grad, rel=2e-5)
    check_grad("xys", extras["xys"].grad, f["xys"].grad, rel=2e-5)
    # the compensation's share of the gradient is far above the bars: leaving it out would fail them
    classic = P["model"].to(DEV).requires_grad_(True)
    from tinysplat_amd.rasterizer import GaussianRasterizer
    rgb_c, ex_c = GaussianRasterizer(classic, None, device=torch.device(DEV))(P["cam"], P["dims"], P["sh"])
    assert (rgb_c.detach() - rgb).abs().max().item() > 1e-2


@pytest.mark.parametrize("path", ("op_by_op", "prep"))
def test_op_by_op_adapter_paths_match_the_one_node_path(path):
    """GaussianRasterizer's op-by-op recipe (fused_colors=False) and its fused-preparation recipe (one node off) compute
    o_eff with ops.opacity_compensation and hand it over as a plain opacity: image and gradients against the one-node
    path at the same bars."""
    P = _parity_reference()
    one, rgb_one, ex_one = _run_adapter(P, True, True)
    md, rgb, extras = _run_adapter(P, path == "prep", False)
    # (the op-by-op recipe takes exp and the norm from torch, the one-node frame inside its kernels: a radius may flip)
    assert (extras["radii"] == ex_one["radii"]).float().mean().item() > 0.999
    assert_close_masked(rgb, rgb_one, 1e-5, P["stable"], what="rgb")
    assert_close_masked(extras["depth"].detach(), ex_one["depth"].detach(), 1e-5 * 10.0, P["stable"], what="depth")
    for nm in _NAMES:
        check_grad(nm, getattr(md, nm).grad, getattr(one, nm).grad, rel=2e-5)
    check_grad("xys", extras["xys"].grad, ex_one["xys"].grad, rel=2e-5)


def test_opacity_compensation_op_matches_the_oracle():
    """ops.opacity_compensation forward and backward (log-scales and raw quaternions, and prepared inputs) against the
    float64 restatement on the parity scene: comp within 1e-5, the gradients of a random weighted sum at check_grad's bars."""
    import antialias_oracle as AO
    from tinysplat_amd import ops
    from tinysplat_amd.rasterizer import project_args
    P = _parity_reference()
    model, cam, (w, h) = P["model"], P["cam"], P["dims"]
    g = torch.Generator().manual_seed(3)
    weights = torch.randn(model.means.shape[0], generator=g)
    ref = {k: getattr(model, k).detach().double().requires_grad_(True) for k in ("means", "scales", "quats")}
    unit = ref["quats"] / ref["quats"].norm(dim=-1, keepdim=True)
    want, _ = AO.scene_compensation(ref["means"], torch.exp(ref["scales"]), unit, cam.view_matrix.double()[:3, :], cam.f_x,
                                    cam.f_y, w, h)
    (want * weights.double()).sum().backward()
    md = model.to(DEV).requires_grad_(True)
    view = cam.view_matrix.to(DEV)[:3, :]
    got = ops.opacity_compensation(md.means, md.scales, 1., md.quats, view, cam.f_x, cam.f_y, w / 2, h / 2, h, w,
                                   log_scales=True, raw_quats=True)
    (got * weights.to(DEV)).sum().backward()
    assert got.shape == (model.means.shape[0],) and ((got >= 0) & (got <= 1)).all()
    assert (got.detach().cpu().double() - want.detach()).abs().max().item() <= 1e-5
    for nm in ("means", "scales", "quats"):
        check_grad(f"comp:{nm}", getattr(md, nm).grad, ref[nm].grad, rel=2e-5)
    # prepared inputs: the same values to rounding
    pa = project_args(model.to(DEV), cam, (w, h), DEV)
    plain = ops.opacity_compensation(pa[0], pa[1], 1., pa[3], view, cam.f_x, cam.f_y, w / 2, h / 2, h, w)
    assert (plain - got.detach()).abs().max().item() <= 1e-5


# ---- 7. training
def _training_case():
    from tinysplat_amd.rasterizer import GaussianRasterizer
    from tinysplat_amd.synthetic import make_scene
    n, sh, w, h = 3000, 0, 160, 112
    truth, cam = make_scene(n, sh, w, h, seed=11, scale_mult=3.0)
    truth = truth.to(DEV)
    truth.rasterize_mode = "antialiased"
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(truth, None, device=torch.device(DEV))(cam, None, sh)
    gen = torch.Generator(device="cpu").manual_seed(12)
    start, _ = make_scene(n, sh, w, h, seed=11, scale_mult=3.0)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(n, 3, generator=gen)
    start.means = start.means + 0.02 * torch.randn(n, 3, generator=gen)
    return start, cam, tgt.clone(), extras["depth"].clone()


def _fresh(start, mode):
    model = start.to(DEV)
    for nm in _NAMES:
        setattr(model, nm, getattr(model, nm).detach().clone())
    if mode is None:
        del model.rasterize_mode
    else:
        model.rasterize_mode = mode
    return model


def test_fused_adam_step_in_the_mode_is_bitwise_the_two_launch_step():
    """TrainStep on an antialiased model, fused against backward + ts_adam_step: the six tensors and both moment sets bit
    for bit after two steps; the fused update ran (the logits are the tensor it updates), and the step differs from the
    classic one."""
    from tinysplat_amd.training import TrainStep
    start, cam, tgt, tgt_d = _training_case()
    runs = {}
    for fused in (False, True):
        model = _fresh(start, "antialiased")
        step = TrainStep(model, DEV, fused_adam=fused)
        outs = [step(cam, tgt, tgt_d) for _ in range(2)]
        assert step.optimizer.fused_steps == (2 if fused else 0)
        runs[fused] = (model, step.optimizer, outs)
    (m0, o0, r0), (m1, o1, r1) = runs[False], runs[True]
    for a, b in zip(r0, r1):
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["xys_grad"], b["xys_grad"])
    for nm in _NAMES:
        assert torch.equal(getattr(m0, nm), getattr(m1, nm)), nm
        assert torch.equal(o0.exp_avg[nm], o1.exp_avg[nm]) and torch.equal(o0.exp_avg_sq[nm], o1.exp_avg_sq[nm]), nm
    assert not torch.equal(m1.opacities, start.opacities.to(DEV)) and torch.isfinite(m1.scales).all()
    classic = _fresh(start, "classic")
    step = TrainStep(classic, DEV)
    step(cam, tgt, tgt_d)
    step(cam, tgt, tgt_d)
    assert not torch.equal(classic.scales, m1.scales)


def test_explicit_classic_mode_is_the_model_without_the_attribute():
    from tinysplat_amd.training import TrainStep
    start, cam, tgt, tgt_d = _training_case()
    models = []
    for mode in ("classic", None):
        model = _fresh(start, mode)
        assert hasattr(model, "rasterize_mode") == (mode is not None)
        out = TrainStep(model, DEV)(cam, tgt, tgt_d)
        models.append((model, out))
    (a, oa), (b, ob) = models
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["xys_grad"], ob["xys_grad"])
    for nm in _NAMES:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm


def test_fit_with_the_reference_densifier_keeps_the_mode():
    from tinysplat_amd.densify import DensifyConfig, Densifier
    from tinysplat_amd.training import fit
    start, cam, tgt, tgt_d = _training_case()
    model = _fresh(start, "antialiased")
    dens = Densifier(model, DensifyConfig(warmup_densify=4, warmup_grad=2, interval_densify=4, tau_means=1e-7))
    losses = []
    fit(model, [cam], [tgt], DEV, 10, max_sh_degree=0, densifier=dens, rng=np.random.default_rng(0),
        generator=torch.Generator().manual_seed(0), on_step=lambda s, o: losses.append(float(o["loss"])))
    assert len(losses) == 10 and np.isfinite(losses).all()
    assert model.rasterize_mode == "antialiased" and model.means.shape[0] != start.means.shape[0]
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_sharded_entry_points_refuse_the_mode():
    from tinysplat_amd import frame, sharded, sharding
    from tinysplat_amd.rasterizer import camera_on_device
    start, cam, _, _ = _training_case()
    model = _fresh(start, "antialiased")
    dims = (cam.width, cam.height)
    layout = sharded.ShardLayout(model.means.shape[0], 1, 0, dims)
    with pytest.raises(NotImplementedError, match="antialiased"):
        sharded.render_sharded(model, cam, DEV, layout, sharded._LocalCounts())
    with pytest.raises(NotImplementedError, match="antialiased"):
        sharded.simulate_frame(model, cam, dims, DEV, 2, lambda *a: None)
    with pytest.raises(NotImplementedError, match="antialiased"):
        sharded.export_records(model, cam, DEV, layout)
    with pytest.raises(NotImplementedError, match="antialiased"):
        sharding.render_stripe(model, cam, dims, torch.device(DEV))
    with pytest.raises(NotImplementedError, match="antialiased"):
        sharding.render_rgb_stripe(model, cam, dims, None, torch.device(DEV))
    view, projview, origin = camera_on_device(cam, torch.device(DEV))
    with pytest.raises(NotImplementedError, match="process group"):
        frame.render_frame(model, view[:3, :], projview, origin, cam.f_x, cam.f_y, dims[0], dims[1], group=object())


# ---- 8. the point of it
def test_antialiased_render_is_closer_to_the_downsampled_truth():
    """300 sparse, semi-transparent Gaussians of about 1 px at 128 x 96 (antialias_cases.downsample_scene), rendered at
    32 x 24 by the same camera and compared with the 4 x 4 box mean of the classic 128 x 96 render: the antialiased
    render's mean squared error is the smaller one.  The oracle alone (CPU, float32) gives 2.38e-2 for the classic and
    1.26e-3 for the antialiased render (against the antialiased 128 x 96 render: 2.91e-2 and 4.08e-4); measured on the
    GPU: the same figures to three digits (printed)."""
    from tinysplat_amd.rasterizer import GaussianRasterizer
    model, cam_hi, cam_lo = AC.downsample_scene()
    mse = {}
    with torch.no_grad():
        for mode in ("classic", "antialiased"):
            md = model.to(DEV)
            md.rasterize_mode = mode
            r = GaussianRasterizer(md, None, device=torch.device(DEV))
            hi = AC.box_mean(r(cam_hi)[0])
            lo = r(cam_lo)[0]
            if mode == "classic":
                truth = hi
            mse[mode] = float(((lo - truth) ** 2).mean())
            mse[mode + " own"] = float(((lo - hi) ** 2).mean())
    print(f"mean squared error against the box mean of the classic 128 x 96 render: classic {mse['classic']:.4g}, "
          f"antialiased {mse['antialiased']:.4g}; antialiased against its own 128 x 96 render {mse['antialiased own']:.4g}")
    assert mse["antialiased"] < mse["classic"]


# ---- 9. round trip
def test_ply_round_trip_keeps_the_mode_and_a_classic_file_is_unchanged(tmp_path):
    from tinysplat_amd import formats
    from tinysplat_amd.rasterizer import GaussianRasterizer
    model, cam = _baked_scene()
    aa = model.to(DEV)
    aa.rasterize_mode = "antialiased"
    formats.export_ply(aa, tmp_path / "aa.ply")
    head = (tmp_path / "aa.ply").read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head.count("comment rasterize_mode antialiased") == 1
    back = formats.load_ply(tmp_path / "aa.ply", DEV)
    assert back.rasterize_mode == "antialiased"
    back.background = aa.background
    back.active_sh_degree = aa.active_sh_degree
    with torch.no_grad():
        a, ea = GaussianRasterizer(aa, None, device=torch.device(DEV))(cam)
        b, eb = GaussianRasterizer(back, None, device=torch.device(DEV))(cam)
    assert torch.equal(a, b) and torch.equal(ea["depth"], eb["depth"])
    assert formats.load_ply(tmp_path / "aa.ply", DEV, rasterize_mode="classic").rasterize_mode == "classic"
    # a classic model: the bytes written for a model without the attribute
    classic, bare = model.to(DEV), model.to(DEV)
    del bare.rasterize_mode
    formats.export_ply(classic, tmp_path / "classic.ply")
    formats.export_ply(bare, tmp_path / "bare.ply")
    data = (tmp_path / "classic.ply").read_bytes()
    assert data == (tmp_path / "bare.ply").read_bytes() and b"comment" not in data.split(b"end_header\n")[0]
    assert formats.load_ply(tmp_path / "classic.ply", DEV).rasterize_mode == "classic"
    # .pth carries nothing: the six tensors and no other key
    formats.save_checkpoint(aa, tmp_path / "aa.pth")
    assert sorted(torch.load(tmp_path / "aa.pth")) == sorted(formats.FIELDS)
    assert formats.load_checkpoint(tmp_path / "aa.pth", DEV).rasterize_mode == "classic"
    assert formats.load_checkpoint(tmp_path / "aa.pth", DEV, rasterize_mode="antialiased").rasterize_mode == "antialiased"
