"""The per-view appearance model on the GPU (tinysplat_amd.appearance, csrc/appearance.hip): the
kernels against the host build of csrc/appearance_math.h (bit for bit where the definition fixes the bits) and against the
float64 oracle of tests/appearance_oracle.py at the bounds tests/appearance_cases.py derives, the optimiser step, and the
model inside ``fit`` and ``evaluate``."""
import numpy as np
import pytest
import torch

import appearance_cases as AC
from tinysplat_amd import metrics as M
from tinysplat_amd.appearance import AppearanceConfig, AppearanceModel, apply_grid, grid_backward, grid_tv
from tinysplat_amd.synthetic import PinholeCamera, make_scene
from tinysplat_amd.training import Adam, TrainStep, fit

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARAMS = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("appearance_host"))


def _gpu(a):
    return torch.tensor(np.array(a)).to(DEV)                          # (a copy: the shared inputs are read-only)


# --------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("h,w,grid", AC.CASES, ids=AC.IDS)
def test_forward_and_backward_against_host_build_and_oracle(host, h, w, grid):
    image, G, v_out = AC.inputs(h, w, grid)
    ref = AC.reference(h, w, grid)
    out = apply_grid(_gpu(image), _gpu(G)).cpu().numpy()
    assert out.tobytes() == AC.host_forward(host, image, G).tobytes()
    v_image, v_grid = grid_backward(_gpu(image), _gpu(G), _gpu(v_out))
    host_v_image, _ = AC.host_backward(host, image, G, v_out)
    assert v_image.cpu().numpy().tobytes() == host_v_image.tobytes()
    AC.check_against_oracle(ref, v_grid=v_grid.cpu().numpy())
    again = grid_backward(_gpu(image), _gpu(G), _gpu(v_out))[1]
    assert torch.equal(v_grid, again) and v_grid.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    # an image whose storage is not 16-byte aligned takes the scalar accesses: the same bits
    shifted = torch.empty(image.size + 1, device=DEV)[1:].view(h, w, 3)
    shifted.copy_(_gpu(image))
    assert shifted.data_ptr() % 16 != 0 and apply_grid(shifted, _gpu(G)).cpu().numpy().tobytes() == out.tobytes()


@pytest.mark.parametrize("h,w,grid", AC.CASES[:1] + AC.CASES[2:], ids=AC.IDS[:1] + AC.IDS[2:])
def test_identity_grid_returns_the_image(h, w, grid):
    image, _, v_out = AC.inputs(h, w, grid)
    eye = _gpu(AC.identity(grid))
    assert apply_grid(_gpu(image), eye).cpu().numpy().tobytes() == image.tobytes()
    assert np.array_equal(grid_backward(_gpu(image), eye, _gpu(v_out))[0].cpu().numpy(), v_out)


@pytest.mark.parametrize("grid", [AC.DEFAULT, (1, 1, 1), (2, 1, 3), (3, 2, 1)], ids=str)
def test_total_variation_is_the_host_builds(host, grid):
    G = AC.inputs(37, 53, grid)[1]
    base = np.random.default_rng(4).standard_normal(G.shape).astype(np.float32)
    for weight, v_in in ((1.0, None), (10.0, base)):
        want_value, want_grad = AC.host_tv(host, G, weight, v_in)
        value, grad = grid_tv(_gpu(G), weight, None if v_in is None else _gpu(v_in))
        assert np.float64(value.item()).tobytes() == np.float64(want_value).tobytes()
        assert grad.cpu().numpy().tobytes() == want_grad.tobytes()


def test_fit_sums_are_the_host_builds(host):
    image, target, u8 = AC.fit_inputs()
    for tgt in (target, u8):
        got = M.affine_fit_sums(_gpu(image), _gpu(tgt)).cpu().numpy()
        assert got.tobytes() == AC.host_fit_sums(host, image, tgt).tobytes()
    fit_map = M.affine_color_fit(_gpu(image), _gpu(target))
    assert fit_map.shape == (3, 4) and fit_map.dtype == np.float64
    assert np.abs(fit_map - np.hstack([0.8 * np.eye(3), np.full((3, 1), 0.1)])).max() < 0.02      # the planted map, roughly


# ---------------------------------------------------------------------------------------------------- the optimiser step
def _trained_model(views=3, seed=8):
    model = AppearanceModel(views, AppearanceConfig(), DEV)
    g = torch.Generator().manual_seed(seed)
    model.grids += (0.05 * torch.randn(model.grids.shape, generator=g)).to(DEV)
    model.exp_avg.copy_((0.01 * torch.randn(model.grids.shape, generator=g)).to(DEV))
    model.exp_avg_sq.copy_((1e-4 * torch.rand(model.grids.shape, generator=g)).to(DEV))
    model.steps = [5, 9, 2]
    return model


def test_step_touches_one_view_and_equals_adam_on_its_slice():
    image, _, v_out = AC.inputs(37, 53, AC.DEFAULT)
    model = _trained_model()
    before = {n: getattr(model, n).clone() for n in ("grids", "exp_avg", "exp_avg_sq")}
    x = _gpu(image).requires_grad_(True)
    y = model.apply(x, 1)
    y.backward(_gpu(v_out))
    v_image, v_grid = grid_backward(_gpu(image), before["grids"][1], _gpu(v_out))
    assert torch.equal(x.grad, v_image) and torch.equal(model.grad, v_grid)
    with pytest.raises(RuntimeError):
        model.apply(x, 0)                                             # view 1's gradient is waiting for its step
    assert model.step(0) is None and model.steps == [5, 9, 2]         # nothing pending for view 0
    tv = model.step(1)
    assert model.steps == [5, 10, 2] and torch.equal(tv, grid_tv(before["grids"][1])[0])
    for n in before:
        now = getattr(model, n)
        for view in (0, 2):
            assert now[view].cpu().numpy().tobytes() == before[n][view].cpu().numpy().tobytes(), (n, view)
        assert not torch.equal(now[1], before[n][1]), n
    # the same update through training.Adam (ts_adam_step) on a copy of the slice
    cfg = model.config
    param = before["grids"][1].clone()
    optim = Adam({"grid": param}, {"grid": cfg.lr}, cfg.betas, cfg.eps)
    optim.exp_avg["grid"], optim.exp_avg_sq["grid"] = before["exp_avg"][1].clone(), before["exp_avg_sq"][1].clone()
    optim.steps["grid"] = 9
    param.grad = grid_tv(before["grids"][1], cfg.tv_weight, v_grid)[1]
    optim.step()
    assert torch.equal(param, model.grids[1]) and torch.equal(optim.exp_avg["grid"], model.exp_avg[1])
    assert torch.equal(optim.exp_avg_sq["grid"], model.exp_avg_sq[1])


def test_state_round_trip(tmp_path):
    model = _trained_model()
    model.save(tmp_path / "appearance.pt")
    loaded = AppearanceModel.load(tmp_path / "appearance.pt", DEV)
    assert loaded.config == model.config and loaded.steps == model.steps
    for n in ("grids", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(loaded, n), getattr(model, n))


# ------------------------------------------------------------------------------------------------------- fit, evaluate
def _scene(n=500, w=160, h=112, seed=5):
    """tests/test_gpu_mcmc.py's small teacher scene, cut to its first ``n`` rows, seen by two cameras"""
    from tinysplat_amd.rasterizer import GaussianRasterizer
    truth, cam = make_scene(3000, 1, w, h, seed=seed, scale_mult=4.0)
    gen = torch.Generator().manual_seed(seed + 1)
    start, _ = make_scene(3000, 1, w, h, seed=seed, scale_mult=4.0)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(3000, 3, generator=gen)
    start.opacities = start.opacities + 0.5 * torch.randn(3000, 1, generator=gen)
    for model in (truth, start):
        for nm in PARAMS:
            setattr(model, nm, getattr(model, nm)[:n].clone())
    cams = [cam, PinholeCamera.look_at_origin_plus_z(w, h, position=(0.25, 0.05, 0.0))]
    teacher = truth.to(DEV)
    with torch.no_grad():
        render = GaussianRasterizer(teacher, None, device=torch.device(DEV))
        targets = [render(c, None, 1)[0].clone() for c in cams]
    return start, teacher, cams, targets


def _fresh(start):
    model = start.to(DEV)
    for nm in PARAMS:
        setattr(model, nm, getattr(model, nm).detach().clone().contiguous())
    return model


def _run(start, cams, targets, steps, appearance):
    model, losses = _fresh(start), []
    fit(model, cams, targets, DEV, steps, generator=torch.Generator().manual_seed(0), rng=np.random.default_rng(0),
        on_step=lambda step, out: losses.append(out["loss"]), appearance=appearance)
    return model, [float(v) for v in losses]


def test_fit_with_a_frozen_identity_model_is_fit_without():
    start, _teacher, cams, targets = _scene()
    plain, plain_losses = _run(start, cams[:1], targets[:1], 20, None)
    frozen, frozen_losses = _run(start, cams[:1], targets[:1], 20, AppearanceConfig(lr=0.0, tv_weight=0.0))
    assert np.array(plain_losses).tobytes() == np.array(frozen_losses).tobytes()
    for nm in PARAMS:
        assert torch.equal(getattr(plain, nm), getattr(frozen, nm)), nm


def _alternate(start, cams, targets, steps, appearance):
    """``steps`` training steps on the views in turn, on the black background the targets were rendered on (``fit`` draws a
    random background per step, as the reference does: where the few hundred Gaussians leave the frame open, a target
    rendered on black then asks every view's matrix to darken, whatever its gain) -> the losses"""
    model = _fresh(start)
    step_fn, losses = TrainStep(model, DEV), []
    for step in range(1, steps + 1):
        view = (step - 1) % len(cams)
        extra = {} if appearance is None else dict(appearance=appearance, view=view)
        out = step_fn(cams[view], targets[view], **extra)
        assert ("appearance_tv" in out) == (appearance is not None)
        losses.append(out["loss"])
    return [float(v) for v in losses]


def test_appearance_explains_per_view_gains():
    start, _teacher, cams, targets = _scene()
    gains = (0.7, 1.3)
    scaled = [t * g for t, g in zip(targets, gains)]
    plain_losses = _alternate(start, cams, scaled, 200, None)
    appearance = AppearanceModel(2, AppearanceConfig(grid=(1, 1, 1)), DEV)
    losses = _alternate(start, cams, scaled, 200, appearance)
    diag = appearance.grids[:, 0, 0, 0, [0, 5, 10]].cpu().numpy()
    print(f"final loss {plain_losses[-1]:.5f} without, {losses[-1]:.5f} with appearance; diagonals {diag.tolist()}; "
          f"steps per view {appearance.steps}")
    assert losses[-1] < plain_losses[-1]                              # (the same view in both runs)
    assert np.all(diag[0] < 1.0) and np.all(diag[0] > 0.7 - 0.05)     # from 1 towards 0.7 (and not far beyond it)
    assert np.all(diag[1] > 1.0) and np.all(diag[1] < 1.3 + 0.05)
    assert appearance.steps == [100, 100]


def test_color_corrected_evaluation():
    _start, teacher, cams, targets = _scene()
    scaled = [(t * g).contiguous() for t, g in zip(targets, (0.7, 1.3))]
    today = M.evaluate(teacher, cams, scaled, DEV)
    off = M.evaluate(teacher, cams, scaled, DEV, color_correct=False)
    on = M.evaluate(teacher, cams, scaled, DEV, color_correct=True)
    assert off.table.tobytes() == today.table.tobytes()
    rows = torch.stack([M.image_metrics(r, s) for r, s in zip(targets, scaled)]).cpu().numpy()
    assert today.table.tobytes() == rows.tobytes()                    # the table the evaluation has always given
    print(f"PSNR per view: {today.table[:, 3].tolist()} as rendered, {on.table[:, 3].tolist()} colour-corrected")
    assert np.all(on.table[:, 3] > today.table[:, 3])
