"""The opacity-entropy regulariser on the GPU (tinysplat_amd.surface): against the reference's own training-script
block (tests/golden/surface_opacity.npz) and the float64 oracle at 1 M Gaussians, run to run, inside TrainStep (no
change on steps where it is inactive; one backward for the whole loss where it is active) and inside fit."""
import numpy as np
import pytest
import torch

from helpers import GOLD
from surface_oracle import opacity_entropy_oracle
from tinysplat_amd.surface import SurfaceConfig, SurfaceRegularizer, opacity_entropy
from tinysplat_amd.synthetic import make_scene
from tinysplat_amd.training import TrainStep, planes_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")


def _entropy(x, weight=1.0):
    x = x.to(DEV).requires_grad_(True)
    lo = opacity_entropy(x)
    (weight * lo).backward()
    return lo.detach().cpu().double(), x.grad.cpu().double()


@pytest.mark.parametrize("case", ["random", "extreme"])
def test_opacity_entropy_matches_the_reference(case):
    z = np.load(GOLD / "surface_opacity.npz")
    lam = float(z["default_lambda_opacity"])
    lo, grad = _entropy(torch.from_numpy(z[f"{case}_opacities"]), lam)
    assert grad.shape == z[f"{case}_grad"].shape
    assert abs(lo.item() - float(z[f"{case}_loss_opacity"])) <= 1e-6 * max(1.0, abs(lo.item()))
    ref = torch.from_numpy(z[f"{case}_grad"]).double()
    assert (grad - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    lo64, g64 = opacity_entropy_oracle(z[f"{case}_opacities"], weight=lam)
    assert abs(lo.item() - lo64.item()) <= 1e-6 * max(1.0, abs(lo64.item()))
    assert (grad - g64).abs().max().item() <= 1e-5 * g64.abs().max().item()


def test_opacity_entropy_at_1m_against_the_float64_oracle_and_bitwise_run_to_run():
    g = torch.Generator().manual_seed(3)
    x = 4.0 * torch.randn(1_000_000, 1, generator=g)
    x[::1000] = 30.0 * torch.sign(torch.randn(1000, 1, generator=g))      # saturated sigmoids
    lo, grad = _entropy(x)
    lo64, g64 = opacity_entropy_oracle(x)
    assert abs(lo.item() - lo64.item()) <= 1e-6 * abs(lo64.item()), (lo.item(), lo64.item())
    err = (grad - g64).abs()
    assert err.max().item() <= 1e-5 * g64.abs().max().item(), err.max().item()
    lo2, grad2 = _entropy(x)
    assert torch.equal(lo, lo2) and torch.equal(grad, grad2)
    xd = x.to(DEV)
    assert torch.equal(opacity_entropy(xd), opacity_entropy(xd.view(-1)))       # any shape: the same memory


def test_a_step_against_the_gradient_lowers_the_entropy():
    g = torch.Generator().manual_seed(4)
    x = (2.0 * torch.randn(5000, 1, generator=g)).to(DEV).requires_grad_(True)
    lo = opacity_entropy(x)
    lo.backward()
    step = 0.05 * x.grad / x.grad.norm()
    with torch.no_grad():
        assert opacity_entropy(x - step).item() < lo.item() < opacity_entropy(x + step).item()


def _scene(n=3000, w=160, h=112, seed=5):
    from tinysplat_amd.rasterizer import GaussianRasterizer
    truth, cam = make_scene(n, 1, w, h, seed=seed, scale_mult=4.0)
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(truth.to(DEV), None, device=torch.device(DEV))(cam, None, 1)
    gen = torch.Generator().manual_seed(seed + 1)
    start, _ = make_scene(n, 1, w, h, seed=seed, scale_mult=4.0)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(n, 3, generator=gen)
    start.opacities = start.opacities + 0.5 * torch.randn(n, 1, generator=gen)
    return start, cam, tgt.clone(), extras["depth"].clone()


def _fresh(start):
    model = start.to(DEV)
    for nm in PARAMS:
        setattr(model, nm, getattr(model, nm).detach().clone())
    return model


def test_train_step_with_an_inactive_regulariser_is_bitwise_the_plain_step():
    start, cam, tgt, tgt_d = _scene()
    surface = SurfaceRegularizer(SurfaceConfig(regularize_opacity=True, regularize_opacity_start=100,
                                               regularize_opacity_end=200))
    runs = []
    for with_surface in (False, True):
        model = _fresh(start)
        step = TrainStep(model, DEV)
        outs = [step(cam, tgt, tgt_d, step=s, surface=surface if with_surface else None) for s in (1, 2, 3)]
        assert step.optimizer.fused_steps == 3
        runs.append((model, step.optimizer, outs))
    (m0, o0, r0), (m1, o1, r1) = runs
    for a, b in zip(r0, r1):
        assert torch.equal(a["loss"], b["loss"]) and "loss_opacity" not in b
    for nm in PARAMS:
        assert torch.equal(getattr(m0, nm), getattr(m1, nm)), nm
        assert torch.equal(o0.exp_avg[nm], o1.exp_avg[nm]) and torch.equal(o0.exp_avg_sq[nm], o1.exp_avg_sq[nm]), nm


def test_train_step_with_the_active_regulariser_matches_a_torch_composition():
    """train.py:58-75, :93-97 on one step: the planes loss + lambda * entropy (torch's float32 expression) in one
    backward, then Adam.  The first Adam moment is 0.1 * gradient: compared there (the update itself is about
    lr * sign(gradient), which near-zero gradients make meaningless to compare)."""
    start, cam, tgt, tgt_d = _scene()
    lam = 0.3
    surface = SurfaceRegularizer(SurfaceConfig(regularize_opacity=True, lambda_opacity=lam,
                                               regularize_opacity_start=1, regularize_opacity_end=2))
    model = _fresh(start)
    before = model.opacities.detach().clone()
    step = TrainStep(model, DEV)
    out = step(cam, tgt, tgt_d, step=1, surface=surface)
    assert step.optimizer.fused_steps == 0 and all(v == 1 for v in step.optimizer.steps.values())

    ref_model = _fresh(start)
    ref_step = TrainStep(ref_model, DEV, fused_adam=False)
    rgb, extras = ref_step.scene.render(cam)
    loss = planes_loss(rgb, extras["depth"], tgt, tgt_d, 0.2, 0.2)[0]
    o = torch.sigmoid(ref_model.opacities)
    lo = -(o * torch.log(o + 1e-10) + (1 - o) * torch.log(1 - o + 1e-10)).mean()
    loss = loss + lam * lo
    loss.backward()
    ref_step.optimizer.step()

    lo64, _ = opacity_entropy_oracle(before.cpu())
    assert abs(out["loss_opacity"].item() - lo64.item()) <= 1e-6 * abs(lo64.item())
    assert abs(out["loss"].item() - loss.item()) <= 1e-6 * abs(loss.item())
    for nm in PARAMS:
        a, b = step.optimizer.exp_avg[nm], ref_step.optimizer.exp_avg[nm]
        if nm == "opacities":
            assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), nm
        else:
            assert torch.equal(a, b), nm            # the frame's own gradients: the same kernels on the same inputs
    assert not torch.equal(step.optimizer.exp_avg["opacities"], _plain_opacity_moment(start, cam, tgt, tgt_d))


def _plain_opacity_moment(start, cam, tgt, tgt_d):
    model = _fresh(start)
    step = TrainStep(model, DEV, fused_adam=False)
    step(cam, tgt, tgt_d)
    return step.optimizer.exp_avg["opacities"]


def test_fit_reports_the_opacity_term_inside_its_window():
    from tinysplat_amd.training import fit
    start, cam, tgt, tgt_d = _scene(n=2000, seed=8)
    model = _fresh(start)
    outs = {}
    cfg = SurfaceConfig(regularize_opacity=True, regularize_opacity_start=4, regularize_opacity_end=9)
    fit(model, [cam], [tgt], DEV, 12, generator=torch.Generator().manual_seed(0), surface=cfg,
        on_step=lambda s, o: outs.__setitem__(s, o))
    assert sorted(s for s, o in outs.items() if "loss_opacity" in o) == list(range(4, 9))
    assert all(np.isfinite(float(o["loss"])) for o in outs.values())
    assert all(np.isfinite(float(o["loss_opacity"])) for o in outs.values() if "loss_opacity" in o)
    assert all(torch.isfinite(p).all() for p in model.parameters())
