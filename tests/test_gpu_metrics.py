"""The evaluation metrics on the GPU: ts_image_metrics against the float64 oracle, ``evaluate`` on a
small synthetic scene, and a training run with an ``Evaluator`` attached that must not change what is trained."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as MC
from tinysplat_amd import Evaluator, Scene, evaluate, image_metrics
from tinysplat_amd.dataset import Targets
from tinysplat_amd.synthetic import PinholeCamera, make_scene
from tinysplat_amd.training import DEFAULT_LRS, PARAM_ORDER, fit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, N = 128, 96, 2000


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("h,w", MC.SHAPES)
def test_image_metrics_against_the_oracle(h, w):
    """Both target types and both pixel strides against the float64 oracle; a uint8 target and its float32 quotients give
    the same 32 bytes; so do two runs, and two frames that differ in their (garbage) depth channel."""
    img, tgt, u8 = MC.inputs(h, w)
    img3, img4, other4 = img.to(DEV), MC.with_depth(img).to(DEV), MC.with_depth(img, seed=4).to(DEV)
    for byte_target in (False, True):
        target = (u8 if byte_target else tgt).to(DEV)
        ref = MC.reference(h, w, byte_target)
        got3, got4 = image_metrics(img3, target), image_metrics(img4, target)
        print(f"{h}x{w} {'uint8' if byte_target else 'float'}: gpu {got3.tolist()} oracle {ref.tolist()}")
        assert got3.dtype == torch.float64 and got3.shape == (4,)
        MC.check(got3.cpu().numpy(), ref)
        MC.check(got4.cpu().numpy(), ref)
        assert _bits(image_metrics(img3, target)) == _bits(got3)
        assert _bits(image_metrics(other4, target)) == _bits(got4) == _bits(got3)
    as_float = MC.bytes_as_float(u8).to(DEV)
    for image in (img3, img4):
        assert _bits(image_metrics(image, u8.to(DEV))) == _bits(image_metrics(image, as_float))


def test_image_metrics_fills_a_row_of_a_table_and_checks_its_arguments():
    img, tgt, u8 = MC.inputs(40, 40)
    table = torch.full((3, 4), -1.0, dtype=torch.float64, device=DEV)
    out = image_metrics(img.to(DEV), u8.to(DEV), out=table[1])
    assert out.data_ptr() == table[1].data_ptr() and _bits(table[1]) == _bits(image_metrics(img.to(DEV), u8.to(DEV)))
    assert torch.all(table[0] == -1.0) and torch.all(table[2] == -1.0)
    with pytest.raises(ValueError):
        image_metrics(img.to(DEV), tgt[:, :39].to(DEV))
    with pytest.raises(ValueError):
        image_metrics(img.to(DEV), tgt.double().to(DEV))
    with pytest.raises(ValueError):
        image_metrics(img[:10].to(DEV), tgt[:10].to(DEV))
    with pytest.raises(ValueError):
        image_metrics(img.to(DEV), tgt.to(DEV), out=torch.zeros(4, device=DEV))


def test_identical_images():
    img = torch.rand(50, 70, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    mse, l1, ssim, psnr = image_metrics(img, img.clone()).tolist()
    assert mse == 0.0 and l1 == 0.0 and psnr == math.inf and abs(ssim - 1.0) < 1e-6
    # a byte image against its float32 quotients (taken on the host: IEEE division; on the device torch divides by a
    # host scalar as a multiplication by its reciprocal, one ulp off for 126 of the 256 bytes)
    u8 = torch.randint(0, 256, (50, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    mse, l1, ssim, psnr = image_metrics(MC.bytes_as_float(u8).to(DEV), u8.to(DEV)).tolist()
    assert mse == 0.0 and l1 == 0.0 and psnr == math.inf and abs(ssim - 1.0) < 1e-6


def _cameras():
    cams = [PinholeCamera.look_at_origin_plus_z(W, H, position=p)
            for p in ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (-0.3, 0.1, 0.0), (0.0, -0.2, 0.3), (0.15, 0.1, 0.0), (-0.1, -0.1, 0.1))]
    for i, c in enumerate(cams):
        c.name = f"view_{i:02d}.png"
    return cams


def _renders(model, cams, background):
    found = model.background
    model.background = background
    try:
        with torch.no_grad():
            scene = Scene(cams, model, device=DEV)
            return [scene.render(c)[0].clone() for c in cams]
    finally:
        model.background = found


def test_evaluate_on_a_small_scene():
    model, _ = make_scene(N, 1, W, H)
    model = model.to(DEV).requires_grad_(True)
    cams = _cameras()[:4]
    black = torch.zeros(3, device=DEV)
    own = _renders(model, cams, black)
    g = torch.Generator().manual_seed(3)
    noisy = [(r + 0.1 * torch.randn(H, W, 3, generator=g).to(DEV)).clamp(0, 1) for r in own]
    targets = [noisy[0], (noisy[1] * 255.0).round().to(torch.uint8), noisy[2], (noisy[3] * 255.0).round().to(torch.uint8)]

    # what evaluate must leave as it found it
    found_bg = model.background = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    result = evaluate(model, cams, targets, DEV)
    assert model.background is found_bg and model.active_sh_degree == 1
    assert all(p.requires_grad and p.grad is None for p in model.parameters())
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(DEV), dev_rng)
    assert result.table.shape == (4, 4) and result.table.dtype == np.float64
    assert result.names == [c.name for c in cams]

    # row i is the entry on the training forward's image of view i (grad mode on: Scene.render builds the autograd node)
    for background in (None, (0.2, 0.5, 0.7)):
        res = evaluate(model, cams, targets, DEV, background=background)
        model.background = black if background is None else torch.tensor(background, device=DEV)
        scene = Scene(cams, model, device=DEV)
        for i, cam in enumerate(cams):
            image = scene.render(cam)[0]
            assert image.requires_grad
            assert res.table[i].tobytes() == _bits(image_metrics(image.detach(), targets[i])), (background, i)
        model.background = found_bg
    assert result.psnr == pytest.approx(result.table[:, 3].mean()) and 10.0 < result.psnr < 40.0
    assert result.l1 == pytest.approx(result.table[:, 1].mean()) and result.ssim == pytest.approx(result.table[:, 2].mean())

    # the model's own renders: no error at all; rounded to bytes: the rounding's bound
    exact = evaluate(model, cams, own, DEV)
    assert np.all(exact.table[:, 0] == 0.0) and np.all(np.isposinf(exact.table[:, 3])) and exact.psnr == math.inf
    assert np.all(np.abs(exact.table[:, 2] - 1.0) < 1e-6)
    as_bytes = [(r * 255.0).round().to(torch.uint8) for r in own]
    rounded = evaluate(model, cams, Targets(as_bytes), DEV)
    print("psnr of the renders against themselves rounded to uint8:", rounded.table[:, 3].tolist())
    assert np.all(rounded.table[:, 3] >= MC.PSNR_OF_BYTE_ROUNDING) and np.all(np.isfinite(rounded.table[:, 3]))
    # a Targets is read as its bytes: the same table as the byte tensors, and as their float32 quotients (host division)
    assert rounded.table.tobytes() == evaluate(model, cams, as_bytes, DEV).table.tobytes()
    quotients = [MC.bytes_as_float(b.cpu()).to(DEV) for b in as_bytes]
    assert rounded.table.tobytes() == evaluate(model, cams, quotients, DEV).table.tobytes()
    # the floats a Targets hands out on the device are torch's b * (1 / 255): within an ulp (6e-8) of the quotient, which
    # moves an mse of 1.3e-6 made of errors of 1e-3 by at most 2 x 1e-3 x 6e-8, 1e-4 relative, 4e-4 dB
    on_device = evaluate(model, cams, Targets(as_bytes)[:], DEV)
    assert np.all(np.abs(on_device.table[:, 3] - rounded.table[:, 3]) < 1e-3)
    with pytest.raises(ValueError):
        evaluate(model, cams, own[:3], DEV)


def _student(teacher):
    """The teacher with its colours jittered and its opacities lowered and jittered; geometry kept."""
    g = torch.Generator().manual_seed(21)
    s, _ = make_scene(N, 1, W, H)
    assert torch.equal(s.means, teacher.means)
    s.colors_dc = s.colors_dc + 0.3 * torch.randn(N, 3, generator=g)
    s.opacities = s.opacities - 2.0 + 0.5 * torch.randn(N, 1, generator=g)
    return s.to(DEV)


def test_training_with_an_evaluator_is_training_without_it():
    """fit for 60 steps with Evaluator(every=20) and without: the six parameter tensors bit-equal; rows 20, 40, 60; the
    held-out PSNR after step 60 above the one before step 1.  The student is too transparent by 2 logits and the
    opacities' rate is 0.02, so that 60 steps (at most 1.2 logits) move it towards the teacher and cannot pass it."""
    teacher, _ = make_scene(N, 1, W, H)
    cams = _cameras()
    train, held = cams[:4], cams[4:]
    black = torch.zeros(3, device=DEV)
    truth = _renders(teacher.to(DEV), cams, black)
    targets, held_targets = truth[:4], Targets([(t * 255.0).round().to(torch.uint8) for t in truth[4:]])
    lrs = dict(DEFAULT_LRS, opacities=0.02)
    runs = {}
    for attached in (True, False):
        model = _student(teacher)
        before = evaluate(model, held, held_targets, DEV).psnr if attached else None
        ev = Evaluator(model, held, held_targets, DEV, 20) if attached else None
        fit(model, train, targets, DEV, 60, max_sh_degree=1, lrs=lrs, rng=np.random.default_rng(0),
            generator=torch.Generator().manual_seed(0), on_step=ev)
        runs[attached] = (model, ev, before)
    (with_ev, ev, before), (without, _, _) = runs[True], runs[False]
    for name in PARAM_ORDER:
        assert torch.equal(getattr(with_ev, name), getattr(without, name)), name
    assert [r[0] for r in ev.rows] == [20, 40, 60] and all(r[1] == N for r in ev.rows)
    assert ev.final(60) == ev.rows[-1] and len(ev.rows) == 3
    after = ev.rows[-1][2]
    print(f"held-out PSNR before step 1: {before:.4f} dB; rows: {[Evaluator.format(r) for r in ev.rows]}")
    assert math.isfinite(before) and math.isfinite(after) and after > before, (before, after)
    assert after == evaluate(with_ev, held, held_targets, DEV).psnr
