"""Training-step ops through the C ABI: photometric loss + gradient against
autograd of the oracle restatement, Adam against torch.optim.Adam itself, and a short optimisation
run that must reduce the loss."""
import pytest
import torch

from oracle import train_oracle as TO
from tinysplat_amd.training import Adam, TrainStep, frame_loss, photometric_loss, planes_loss
from tinysplat_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("h,w,lam", [(64, 96, 0.2), (77, 131, 0.5), (200, 333, 0.0), (40, 40, 1.0)])
def test_photometric_loss_and_gradient(h, w, lam):
    g = torch.Generator().manual_seed(h * w)
    img = torch.rand(h, w, 3, generator=g)
    tgt = (img + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    x64 = img.double().requires_grad_(True)
    ref, ref_l1, ref_s = TO.photometric_loss(x64, tgt.double(), lam)
    ref.backward()
    xd = img.to(DEV).requires_grad_(True)
    loss, l1, s = photometric_loss(xd, tgt.to(DEV), lam)
    (3.0 * loss).backward()
    assert abs(loss.item() - ref.item()) < 2e-6 and abs(l1.item() - ref_l1.item()) < 2e-6
    assert abs(s.item() - ref_s.item()) < 2e-6
    err = (xd.grad.cpu().double() / 3.0 - x64.grad).abs().max().item()
    assert err < 1e-5 * max(1.0, x64.grad.abs().max().item() * 1e3), err
    assert err < 2e-8 + 1e-4 * x64.grad.abs().max().item()


@pytest.mark.parametrize("h,w,with_depth", [(64, 96, True), (77, 131, False), (120, 50, True)])
def test_frame_loss_on_rgbd_output_equals_the_separate_losses(h, w, with_depth):
    """The fused loss on the adapter's [H, W, 4] output (train.py:58-69) vs autograd of the oracle's
    photometric loss + a float64 depth L1."""
    g = torch.Generator().manual_seed(h + w)
    frame = torch.rand(h, w, 4, generator=g)
    frame[:, :, 3] = 2.0 + 8.0 * frame[:, :, 3]
    tgt = (frame[:, :, :3] + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    dtgt = 2.0 + 8.0 * torch.rand(h, w, generator=g)
    lam, lamd = 0.2, 0.3
    x64 = frame.double().requires_grad_(True)
    ref, ref_l1, ref_s = TO.photometric_loss(x64[:, :, :3], tgt.double(), lam)
    ref_d = (x64[:, :, 3] - dtgt.double()).abs().mean()
    total = ref + lamd * ref_d if with_depth else ref
    total.backward()
    xd = frame.to(DEV).requires_grad_(True)
    loss, l1, s, ld = frame_loss(xd * 1.0, tgt.to(DEV), dtgt.to(DEV) if with_depth else None, lam, lamd)
    (2.0 * loss).backward()
    assert abs(loss.item() - total.item()) < 3e-6 and abs(l1.item() - ref_l1.item()) < 2e-6
    assert abs(s.item() - ref_s.item()) < 2e-6
    assert abs(ld.item() - (ref_d.item() if with_depth else 0.0)) < 2e-6
    err = (xd.grad.cpu().double() / 2.0 - x64.grad).abs().max().item()
    assert err < 2e-8 + 1e-4 * x64.grad.abs().max().item(), err
    if not with_depth:
        assert torch.all(xd.grad[:, :, 3] == 0)


@pytest.mark.parametrize("h,w,with_depth", [(64, 96, True), (77, 131, False), (120, 50, True)])
def test_planes_loss_is_the_frame_loss_bit_for_bit(h, w, with_depth):
    """ABI 5: the fused loss on rgb[H,W,3] + depth[H,W] (ts_loss with a depth plane) against the same loss on the
    interleaved [H,W,4] frame: values and both gradient planes identical; no depth gradient without a target."""
    g = torch.Generator().manual_seed(h * w)
    frame = torch.rand(h, w, 4, generator=g)
    frame[:, :, 3] = 2.0 + 8.0 * frame[:, :, 3]
    tgt = (frame[:, :, :3] + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1).to(DEV)
    dtgt = (2.0 + 8.0 * torch.rand(h, w, generator=g)).to(DEV) if with_depth else None
    xd = frame.to(DEV).requires_grad_(True)
    ref = frame_loss(xd * 1.0, tgt, dtgt, 0.2, 0.3)
    (2.0 * ref[0]).backward()
    rgb = frame[:, :, :3].contiguous().to(DEV).requires_grad_(True)
    dep = frame[:, :, 3].contiguous().to(DEV).requires_grad_(True)
    out = planes_loss(rgb * 1.0, dep * 1.0, tgt, dtgt, 0.2, 0.3)
    (2.0 * out[0]).backward()
    for a, b in zip(ref, out):
        assert torch.equal(a, b)
    assert torch.equal(rgb.grad, xd.grad[:, :, :3])
    if with_depth:
        assert torch.equal(dep.grad, xd.grad[:, :, 3])
    else:
        assert dep.grad is None or torch.all(dep.grad == 0)


@pytest.mark.parametrize("h,w", [(11, 11), (21, 75)])
def test_photometric_loss_is_the_planes_loss_without_a_depth_target_bit_for_bit(h, w):
    """The three-channel loss and the two-plane loss are one implementation: without a depth target the depth plane is
    never compared with anything, so loss, l1, ssim and the image gradient are the same bytes whatever the plane holds.
    The smallest image, and the smallest with a second column block's worth of halo."""
    g = torch.Generator().manual_seed(h * w)
    img = torch.rand(h, w, 3, generator=g)
    tgt = (img + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1).to(DEV)
    dep = (2.0 + 8.0 * torch.rand(h, w, generator=g)).to(DEV).requires_grad_(True)
    x = img.to(DEV).requires_grad_(True)
    one = photometric_loss(x * 1.0, tgt, 0.2)
    (2.0 * one[0]).backward()
    y = img.to(DEV).requires_grad_(True)
    two = planes_loss(y * 1.0, dep * 1.0, tgt, None, 0.2, 0.3)
    (2.0 * two[0]).backward()
    assert len(one) == 3 and len(two) == 4
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert torch.equal(x.grad, y.grad) and x.grad.abs().max().item() > 0.0
    assert dep.grad is None or torch.all(dep.grad == 0)


@pytest.mark.parametrize("h,w", [(11, 11), (11, 75), (12, 11), (55, 139), (57, 74), (99, 75), (100, 203)])
def test_frame_loss_on_sizes_around_the_sliding_windows_edges(h, w):
    """The sliding-window SSIM pass (64 map columns x 44 map rows per wave, 10 halo columns / rows): one map pixel, one
    more column than a wave's main part, exactly 64 map columns (W = 74), one map row more than two segments - the
    loss, its three parts and the gradient of all four channels against autograd of the oracle in float64."""
    g = torch.Generator().manual_seed(7 * h + w)
    frame = torch.rand(h, w, 4, generator=g)
    frame[:, :, 3] = 2.0 + 8.0 * frame[:, :, 3]
    tgt = (frame[:, :, :3] + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    dtgt = 2.0 + 8.0 * torch.rand(h, w, generator=g)
    lam, lamd = 0.2, 0.3
    x64 = frame.double().requires_grad_(True)
    ref, ref_l1, ref_s = TO.photometric_loss(x64[:, :, :3], tgt.double(), lam)
    ref_d = (x64[:, :, 3] - dtgt.double()).abs().mean()
    (ref + lamd * ref_d).backward()
    xd = frame.to(DEV).requires_grad_(True)
    loss, l1, s, ld = frame_loss(xd * 1.0, tgt.to(DEV), dtgt.to(DEV), lam, lamd)
    loss.backward()
    assert abs(loss.item() - (ref + lamd * ref_d).item()) < 3e-6
    assert abs(l1.item() - ref_l1.item()) < 2e-6 and abs(s.item() - ref_s.item()) < 2e-6 and abs(ld.item() - ref_d.item()) < 2e-6
    err = (xd.grad.cpu().double() - x64.grad).abs().max().item()
    assert err < 2e-8 + 1e-4 * x64.grad.abs().max().item(), err


def test_ssim_of_identical_images_is_one():
    img = torch.rand(50, 70, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    loss, l1, s = photometric_loss(img, img.clone(), 0.2)
    assert abs(s.item() - 1.0) < 1e-6 and l1.item() == 0.0 and abs(loss.item()) < 1e-6


def test_adam_matches_torch_optim():
    g = torch.Generator().manual_seed(0)
    shapes = {"means": (1001, 3), "colors_dc": (1001, 3), "colors_rest": (1001, 15, 3),
              "scales": (1001, 3), "quats": (1001, 4), "opacities": (1001, 1)}
    lrs = {"means": 0.00016, "colors_dc": 0.0025, "colors_rest": 0.000125, "scales": 0.005,
           "quats": 0.001, "opacities": 0.05}
    mine = {n: torch.randn(s, generator=g).to(DEV).requires_grad_(True) for n, s in shapes.items()}
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in mine.items()}
    opt = Adam(mine, lrs)
    topt = torch.optim.Adam([{"params": [ref[n]], "lr": lrs[n]} for n in shapes])
    for step in range(5):
        for n in shapes:
            gr = torch.randn(shapes[n], generator=g).to(DEV) * (10.0 ** (step - 2))
            mine[n].grad = gr.clone()
            ref[n].grad = gr.clone()
        if step == 3:
            mine["quats"].grad = None
            ref["quats"].grad = None          # a tensor without gradient is skipped, as in torch
        opt.step()
        topt.step()
    for n in shapes:
        assert torch.allclose(mine[n], ref[n], rtol=2e-6, atol=2e-7), n


def test_adam_step_on_an_sh0_model_with_a_non_contiguous_gradient():
    """64 Gaussians at SH degree 0: colors_rest is [64, 0, 3], so nothing of it is launched, but its step count advances
    as torch.optim.Adam's does; the means' gradient is a transposed view, copied once into row order.  One step against
    torch.optim.Adam on CPU copies, at the tolerance of test_adam_matches_torch_optim."""
    g = torch.Generator().manual_seed(5)
    shapes = {"means": (64, 3), "colors_dc": (64, 3), "colors_rest": (64, 0, 3), "scales": (64, 3), "quats": (64, 4),
              "opacities": (64, 1)}
    ref = {n: torch.randn(s, generator=g).requires_grad_(True) for n, s in shapes.items()}
    mine = {n: p.detach().clone().to(DEV).requires_grad_(True) for n, p in ref.items()}
    for n, s in shapes.items():
        gr = torch.randn(3, 64, generator=g).to(DEV).t() if n == "means" else torch.randn(s, generator=g).to(DEV)
        mine[n].grad, ref[n].grad = gr, gr.cpu().contiguous()
    assert not mine["means"].grad.is_contiguous() and mine["colors_rest"].grad is not None
    opt = Adam(mine)
    topt = torch.optim.Adam([{"params": [ref[n]], "lr": opt.lrs[n]} for n in shapes])
    opt.step()
    topt.step()
    assert opt.steps == {n: 1 for n in shapes}
    for n in shapes:
        assert mine[n].shape == shapes[n] and torch.allclose(mine[n].detach().cpu(), ref[n].detach(), rtol=2e-6, atol=2e-7), n

def test_train_step_reduces_the_loss():
    w, h, n = 160, 112, 4000
    target_model, cam = make_scene(n, 1, w, h, seed=5, scale_mult=4.0)
    from tinysplat_amd.rasterizer import GaussianRasterizer
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(target_model.to(DEV), None, device=torch.device(DEV))(cam, None, 1)
    model = target_model.to(DEV)
    gen = torch.Generator(device="cpu").manual_seed(9)
    model.colors_dc = (model.colors_dc + 0.5 * torch.randn(n, 3, generator=gen).to(DEV))
    model.means = model.means + 0.02 * torch.randn(n, 3, generator=gen).to(DEV)
    step = TrainStep(model, DEV)
    losses = [step(cam, tgt, extras["depth"])["loss"].item() for _ in range(30)]
    assert losses[-1] < 0.7 * losses[0], losses[::5]
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_fit_loop_follows_the_reference_schedule():
    """training.fit = scripts/train.py:45-106: SH degree schedule, random background, camera pick,
    step, densification, on a two-camera toy problem."""
    import numpy as np
    from tinysplat_amd.densify import DensifyConfig, Densifier
    from tinysplat_amd.rasterizer import GaussianRasterizer
    from tinysplat_amd.synthetic import PinholeCamera
    from tinysplat_amd.training import CameraSampler, Scheduler, fit
    w, h = 160, 120
    truth, cam0 = make_scene(3000, 1, w, h, seed=11, scale_mult=4.0)
    cam1 = PinholeCamera.look_at_origin_plus_z(w, h, position=(0.3, 0.0, 0.0))
    truth = truth.to(DEV)
    truth.background = torch.zeros(3, device=DEV)
    with torch.no_grad():
        r = GaussianRasterizer(truth, None, device=torch.device(DEV))
        tg = [r(c, None, 1)[0].clone() for c in (cam0, cam1)]
    model, _ = make_scene(3000, 1, w, h, seed=12, scale_mult=4.0)
    model = model.to(DEV)
    model.active_sh_degree = 0
    losses, degrees = [], []
    dens = Densifier(model, DensifyConfig(warmup_densify=10, warmup_grad=5, interval_densify=10, tau_means=1e-7))
    fit(model, [cam0, cam1], tg, DEV, 30, sh_increment_interval=8, max_sh_degree=1, densifier=dens,
        rng=np.random.default_rng(0), generator=torch.Generator().manual_seed(0),
        on_step=lambda s, o: (losses.append(float(o["loss"])), degrees.append(model.active_sh_degree)))
    assert degrees[6] == 0 and degrees[7] == 1 and degrees[-1] == 1          # step 8 raises the degree, capped at 1
    assert model.means.shape[0] != 3000                                         # densification fired (steps 10, 20, 30)
    assert len(losses) == 30 and all(np.isfinite(losses))    # (that the loss falls is test_train_step_reduces_the_loss's job:
                                                             #  here the background is random per step, train.py:51)
    assert Scheduler(True, 3, 5)(3) and not Scheduler(True, 3, 5)(5) and not Scheduler(False, 0, 9)(1)
    pick = CameraSampler(4, np.random.default_rng(1))
    seq = [pick(s) for s in range(1, 10)]
    assert all(0 <= i < 4 for i in seq)


@pytest.mark.parametrize("sh,n,w,h", [(3, 20000, 320, 208), (0, 3000, 160, 112)])
def test_fused_adam_step_is_bitwise_the_two_launch_step(sh, n, w, h):
    """SURVEY 8(f) F1 (train.py:93-97): TrainStep(fused_adam=True) - the frame's backward pass applies the Adam update to
    the gradients its parameter-stage kernels hold in registers, no gradient tensor is written - against backward +
    ts_adam_step: parameters and both moments bit for bit after three steps, xys.grad too; the fused path really ran."""
    from tinysplat_amd.rasterizer import GaussianRasterizer
    target_model, cam = make_scene(n, sh, w, h, seed=11, scale_mult=3.0)
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(target_model.to(DEV), None, device=torch.device(DEV))(cam, None, sh)
    tgt, tgt_d = tgt.clone(), extras["depth"].clone()
    gen = torch.Generator(device="cpu").manual_seed(12)
    start, _ = make_scene(n, sh, w, h, seed=11, scale_mult=3.0)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(n, 3, generator=gen)
    start.means = start.means + 0.02 * torch.randn(n, 3, generator=gen)
    runs = {}
    for fused in (False, True):
        model = start.to(DEV)
        for nm in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
            setattr(model, nm, getattr(model, nm).detach().clone())
        step = TrainStep(model, DEV, fused_adam=fused)
        outs = [step(cam, tgt, tgt_d) for _ in range(3)]
        assert step.optimizer.fused_steps == (3 if fused else 0)
        if fused:
            assert all(p.grad is None for p in model.parameters())
        runs[fused] = (model, step.optimizer, outs)
    (m0, o0, r0), (m1, o1, r1) = runs[False], runs[True]
    for a, b in zip(r0, r1):
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["xys_grad"], b["xys_grad"])
    for nm in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
        assert torch.equal(getattr(m0, nm), getattr(m1, nm)), nm
        assert torch.equal(o0.exp_avg[nm], o1.exp_avg[nm]) and torch.equal(o0.exp_avg_sq[nm], o1.exp_avg_sq[nm]), nm
        assert o0.steps[nm] == o1.steps[nm] == 3
    assert not torch.equal(m1.means, start.means.to(DEV))
