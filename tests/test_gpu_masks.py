"""The masked loss and the masked metrics on the GPU: an all-255 mask is the unmasked entry bit
for bit; every mask ties the masked kernels to the unmasked ones through the substituted image of ts_mask_blend; the
float64 oracle at the unmasked tests' bars; what is masked cannot steer training; masks through evaluate and the
dataset's undistortion."""
import math

import numpy as np
import pytest
import torch

import mask_cases as KC
from tinysplat_amd import Evaluator, Scene, TrainingMasks, dilate_ignored, evaluate, image_metrics
from tinysplat_amd.masks import mask_weights, substituted_image
from tinysplat_amd.synthetic import PinholeCamera, make_scene
from tinysplat_amd.training import (PARAM_ORDER, TrainStep, fit, frame_loss, photometric_loss, planes_loss,
                                    planes_loss_and_gradient)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = ("rgb", "frame", "planes")


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _run(path, rgb, depth, tgt, dtgt, mask):
    """One of the three loss paths on host tensors -> (values [4] on the host: loss, l1, ssim, depth l1; the gradient
    w.r.t. rgb; the gradient w.r.t. depth or None).  path "rgb": 3 floats per pixel, no depth term."""
    kw = {} if mask is None else {"mask": mask.to(DEV)}
    dt = None if dtgt is None else dtgt.to(DEV)
    if path == "rgb":
        x = rgb.to(DEV).requires_grad_(True)
        loss, l1, s = photometric_loss(x, tgt.to(DEV), KC.LAMBDA, **kw)
        loss.backward()
        return torch.stack([loss.detach(), l1, s, torch.zeros_like(l1)]).cpu(), x.grad, None
    if path == "frame":
        x = torch.cat([rgb, depth[..., None]], dim=2).contiguous().to(DEV).requires_grad_(True)
        out = frame_loss(x, tgt.to(DEV), dt, KC.LAMBDA, KC.LAMBDA_DEPTH, **kw)
        out[0].backward()
        return torch.stack([o.detach() for o in out]).cpu(), x.grad[:, :, :3].contiguous(), x.grad[:, :, 3].contiguous()
    x, d = rgb.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
    out = planes_loss(x, d, tgt.to(DEV), dt, KC.LAMBDA, KC.LAMBDA_DEPTH, **kw)
    out[0].backward()
    return torch.stack([o.detach() for o in out]).cpu(), x.grad, d.grad


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("h,w", KC.SHAPES)
def test_masked_loss_against_the_unmasked_entry_and_the_oracle(h, w, path):
    """Checks 1, 2, 4 and 5 of the issue for one shape and one loss path, with and without a depth target, under every
    mask of mask_cases.masks.

    Equivalence: with X' = ts_mask_blend(X, Y, mask), the masked entry's l1 and ssim values are the unmasked entry's on X'
    bit for bit, its colour gradient is m times that entry's, and its depth gradient m times the unmasked depth
    gradient.  All four values are compared where the unmasked entry can state them: without a depth target, and with one
    under a binary mask, where the unmasked entry runs on the depth d' = D at ignored pixels (|D - D| = 0 = 0 |d - D|).
    Under a soft mask the depth term m |d - D| is no unmasked loss of any depth image; its value and the total are then
    held to the float64 oracle alone."""
    frame, tgt, dtgt = KC.inputs(h, w)
    rgb, depth = frame[:, :, :3].contiguous(), frame[:, :, 3].contiguous()
    plain = {wd: _run(path, rgb, depth, tgt, dtgt if wd else None, None) for wd in (False, True)}
    for name, mask in KC.masks(h, w).items():
        mw = mask_weights(mask.to(DEV))
        blended = substituted_image(rgb.to(DEV), tgt.to(DEV), mask.to(DEV)).cpu()
        for with_depth in ((False,) if path == "rgb" else (False, True)):
            tag = (h, w, path, name, with_depth)
            dt = dtgt if with_depth else None
            values, g_rgb, g_depth = _run(path, rgb, depth, tgt, dt, mask)
            if name == "all255":                                    # 1: the unmasked entry's bits
                assert _bits(values) == _bits(plain[with_depth][0]), tag
                assert torch.equal(g_rgb, plain[with_depth][1]), tag
                assert g_depth is None or plain[with_depth][2] is None or torch.equal(g_depth, plain[with_depth][2]), tag
            # 2: the unmasked entry on the substituted image
            u_values, u_rgb, u_depth = _run(path, blended, depth, tgt, dt, None)
            assert _bits(values[1:3]) == _bits(u_values[1:3]), tag
            assert torch.equal(g_rgb, mw[..., None] * u_rgb), tag
            if with_depth:
                assert torch.equal(g_depth, mw * u_depth), tag
            elif g_depth is not None:
                assert torch.all(g_depth == 0), tag
            if not with_depth:
                assert _bits(values) == _bits(u_values), tag
            elif KC.is_binary(mask):
                substituted_depth = torch.where(mask == 0, dtgt, depth)
                assert _bits(values) == _bits(_run(path, blended, substituted_depth, tgt, dt, None)[0]), tag
            # 4: the float64 oracle at the unmasked tests' bars
            ref = KC.loss_reference(h, w, name, with_depth)
            got = [float(v) for v in values]
            print(f"{tag}: gpu {got} oracle {[ref['loss'], ref['l1'], ref['ssim'], ref['depth']]}")
            assert abs(got[0] - ref["loss"]) < KC.BAR_LOSS and abs(got[1] - ref["l1"]) < KC.BAR_VALUE, tag
            assert abs(got[2] - ref["ssim"]) < KC.BAR_VALUE and abs(got[3] - ref["depth"]) < KC.BAR_VALUE, tag
            err = (g_rgb.cpu().double() - ref["grad_rgb"]).abs().max().item()
            assert err < KC.gradient_bar(ref["grad_rgb"]), (tag, err)
            if with_depth:
                err = (g_depth.cpu().double() - ref["grad_depth"]).abs().max().item()
                assert err < KC.gradient_bar(ref["grad_depth"]), (tag, err)
            # a pixel with byte 0 gets a gradient of exactly zero
            assert torch.all(g_rgb[mask.to(DEV) == 0] == 0), tag
            if name == "all0":                                      # 5
                assert got[1] == 0.0 and got[3] == 0.0 and abs(got[2] - 1.0) < 1e-6, tag
                assert torch.all(g_rgb == 0) and (g_depth is None or torch.all(g_depth == 0)), tag


@pytest.mark.parametrize("h,w", KC.SHAPES)
def test_mask_blend_is_the_host_build_bit_for_bit(h, w, tmp_path_factory):
    lib = _host(tmp_path_factory)
    frame, tgt, _ = KC.inputs(h, w)
    image = frame[:, :, :3].contiguous()
    for name, mask in KC.masks(h, w).items():
        got = substituted_image(image.to(DEV), tgt.to(DEV), mask.to(DEV)).cpu()
        assert _bits(got) == _bits(KC.host_blend(lib, image, tgt, mask)), (h, w, name)
    keep = KC.masks(h, w)["random"] > 100                            # a bool mask is its 0 / 255 bytes
    assert torch.equal(substituted_image(image.to(DEV), tgt.to(DEV), keep.to(DEV)),
                       substituted_image(image.to(DEV), tgt.to(DEV), (keep.to(torch.uint8) * 255).to(DEV)))


_HOST = []


def _host(tmp_path_factory):
    if not _HOST:
        _HOST.append(KC.build_host(tmp_path_factory.mktemp("maskhost")))
    return _HOST[0]


@pytest.mark.parametrize("h,w", KC.SHAPES)
def test_masked_metrics(h, w):
    """An all-255 mask gives image_metrics' 32 bytes; every mask is held to the float64 restatement of the definitions at
    the unmasked tests' bars, for float and uint8 targets and both pixel strides, and gives the same bytes twice; a mask
    that keeps nothing gives four NaNs."""
    frame, tgt, _ = KC.inputs(h, w)
    img3, img4 = frame[:, :, :3].contiguous().to(DEV), frame.to(DEV)
    u8 = (tgt * 255.0).round().to(torch.uint8)
    as_float = u8.to(torch.float32) / 255.0                          # on the host: IEEE division
    for name, mask in KC.masks(h, w).items():
        md = mask.to(DEV)
        for target, target_host in ((tgt.to(DEV), tgt), (u8.to(DEV), as_float)):
            got = image_metrics(img3, target, mask=md)
            assert got.dtype == torch.float64 and got.shape == (4,)
            ref = KC.metrics_reference(frame, target_host, mask)
            print(f"{h}x{w} {name} {target.dtype}: gpu {got.tolist()} restatement {ref.tolist()}")
            KC.check_metrics(got.cpu().numpy(), ref)
            assert _bits(image_metrics(img3, target, mask=md)) == _bits(got)
            assert _bits(image_metrics(img4, target, mask=md)) == _bits(got)
            if name == "all255":
                assert _bits(got) == _bits(image_metrics(img3, target))
            if name == "all0":
                assert all(math.isnan(v) for v in got.tolist())
        assert _bits(image_metrics(img3, u8.to(DEV), mask=md)) == _bits(image_metrics(img3, as_float.to(DEV), mask=md))
    keep = KC.masks(h, w)["random"] > 100
    assert _bits(image_metrics(img3, tgt.to(DEV), mask=keep.to(DEV))) == \
        _bits(image_metrics(img3, tgt.to(DEV), mask=(keep.to(torch.uint8) * 255).to(DEV)))
    with pytest.raises(ValueError):
        image_metrics(img3, tgt.to(DEV), mask=torch.ones(h, w + 1, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------- training and evaluation
W, H, N = 96, 64, 2000
RECT = (20, 30, 40, 60)                                              # rows 20..29, columns 40..59


def _student():
    g = torch.Generator().manual_seed(21)
    s, cam = make_scene(N, 1, W, H)
    s.colors_dc = s.colors_dc + 0.3 * torch.randn(N, 3, generator=g)
    return s.to(DEV), cam


def _targets_and_mask():
    g = torch.Generator().manual_seed(9)
    a = torch.rand(H, W, 3, generator=g)
    b = a.clone()
    y0, y1, x0, x1 = RECT
    b[y0:y1, x0:x1] = torch.rand(y1 - y0, x1 - x0, 3, generator=g)
    inside = torch.full((H, W), 255, dtype=torch.uint8)
    inside[y0:y1, x0:x1] = 0
    mask = dilate_ignored(inside.to(DEV), 10)                        # R grown by the SSIM window's reach
    assert int((mask == 0).sum()) == (y1 - y0 + 20) * (x1 - x0 + 20)
    return a.to(DEV), b.to(DEV), mask


@pytest.mark.parametrize("fused", [True, False])
def test_what_is_masked_cannot_steer_training(fused):
    """One TrainStep from identical copies of a model towards two targets that differ only inside a rectangle, under a
    mask that ignores the rectangle grown by 10 pixels: the six parameter tensors agree bit for bit.  The same step with
    an all-255 mask is the step without a mask, bit for bit."""
    a, b, mask = _targets_and_mask()
    after = {}
    for key, target, m in (("a", a, mask), ("b", b, mask), ("plain", a, None),
                           ("all255", a, torch.full((H, W), 255, dtype=torch.uint8, device=DEV)),
                           ("unmasked_b", b, None)):
        model, cam = _student()
        model.background = torch.tensor([0.1, 0.2, 0.3], device=DEV)
        step = TrainStep(model, DEV, fused_adam=fused)
        out = step(cam, target) if m is None else step(cam, target, mask=m)
        assert math.isfinite(float(out["loss"]))
        after[key] = {n: getattr(model, n).detach().clone() for n in PARAM_ORDER}
    for n in PARAM_ORDER:
        assert torch.equal(after["a"][n], after["b"][n]), n
        assert torch.equal(after["plain"][n], after["all255"][n]), n
    # the comparison has teeth: without the mask the two targets do move the model differently, and the mask changes the step
    assert any(not torch.equal(after["plain"][n], after["unmasked_b"][n]) for n in PARAM_ORDER)
    assert any(not torch.equal(after["plain"][n], after["a"][n]) for n in PARAM_ORDER)


def test_the_renders_gradient_is_zero_on_masked_pixels():
    a, b, mask = _targets_and_mask()
    model, cam = _student()
    model.background = torch.zeros(3, device=DEV)
    with torch.no_grad():
        rgb, extras = Scene([cam], model, device=DEV).render(cam)
    rgb, depth = rgb.detach().contiguous(), extras["depth"].detach().contiguous()
    dtgt = (depth + 0.5).contiguous()
    grads = []
    for target in (a, b):
        _values, v_rgb, v_depth = planes_loss_and_gradient(rgb, depth, target, dtgt, 0.2, 0.2, mask=mask)
        assert torch.all(v_rgb[mask == 0] == 0) and torch.all(v_depth[mask == 0] == 0)
        assert torch.any(v_rgb[mask == 255] != 0) and torch.all(v_depth[mask == 255] != 0)
        grads.append((v_rgb, v_depth))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def _cameras():
    cams = [PinholeCamera.look_at_origin_plus_z(W, H, position=p)
            for p in ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (-0.3, 0.1, 0.0), (0.0, -0.2, 0.3), (0.15, 0.1, 0.0))]
    for i, c in enumerate(cams):
        c.name = f"view_{i:02d}.png"
    return cams


def _renders(model, cams):
    found = model.background
    model.background = torch.zeros(3, device=DEV)
    try:
        with torch.no_grad():
            scene = Scene(cams, model, device=DEV)
            return [scene.render(c)[0].clone() for c in cams]
    finally:
        model.background = found


def _fit(model, cams, targets, steps, **kw):
    fit(model, cams, targets, DEV, steps, max_sh_degree=1, rng=np.random.default_rng(0),
        generator=torch.Generator().manual_seed(0), **kw)
    return {n: getattr(model, n).detach().clone() for n in PARAM_ORDER}


def test_fit_with_masks_and_an_evaluator_with_masks():
    """fit with masks=[None, ...] is fit without; with real masks it is another run.  evaluate's rows under masks are
    image_metrics(..., mask=) on the same renders, a view whose mask keeps nothing is NaN, named, and left out of the
    means; training with such an Evaluator attached is training without one."""
    teacher, _ = make_scene(N, 1, W, H)
    cams = _cameras()
    train, held = cams[:3], cams[3:]
    truth = _renders(teacher.to(DEV), cams)
    targets, held_targets = truth[:3], [(t * 255.0).round().to(torch.uint8) for t in truth[3:]]
    _a, _b, mask = _targets_and_mask()
    none = _fit(_student()[0], train, targets, 6)
    nones = _fit(_student()[0], train, targets, 6, masks=[None, None, None])
    masked = _fit(_student()[0], train, targets, 6, masks=[mask, None, mask > 0])
    for n in PARAM_ORDER:
        assert torch.equal(none[n], nones[n]), n
    assert any(not torch.equal(none[n], masked[n]) for n in PARAM_ORDER)
    with pytest.raises(ValueError):
        _fit(_student()[0], train, targets, 1, masks=[mask])

    model = _student()[0]
    held_masks = [mask, torch.zeros((H, W), dtype=torch.uint8, device=DEV)]
    result = evaluate(model, held, held_targets, DEV, masks=held_masks)
    renders = _renders(model, held)
    assert result.table[0].tobytes() == _bits(image_metrics(renders[0], held_targets[0], mask=mask))
    assert np.all(np.isnan(result.table[1])) and result.empty == [held[1].name]
    assert result.psnr == result.table[0, 3] and result.l1 == result.table[0, 1] and result.ssim == result.table[0, 2]
    mixed = evaluate(model, held, held_targets, DEV, masks=[None, mask])
    assert mixed.table[0].tobytes() == _bits(image_metrics(renders[0], held_targets[0])) and mixed.empty == []
    assert mixed.table[1].tobytes() == _bits(image_metrics(renders[1], held_targets[1], mask=mask))
    assert evaluate(model, held, held_targets, DEV).empty == []
    with pytest.raises(ValueError):
        evaluate(model, held, held_targets, DEV, masks=[mask])

    runs = {}
    for attached in (True, False):
        m = _student()[0]
        ev = Evaluator(m, held, held_targets, DEV, 3, masks=[mask, mask]) if attached else None
        runs[attached] = (_fit(m, train, targets, 6, masks=[mask, None, mask], on_step=ev), ev, m)
    for n in PARAM_ORDER:
        assert torch.equal(runs[True][0][n], runs[False][0][n]), n
    ev, m = runs[True][1], runs[True][2]
    assert [r[0] for r in ev.rows] == [3, 6]
    assert ev.results[-1].table.tobytes() == evaluate(m, held, held_targets, DEV, masks=[mask, mask]).table.tobytes()


def test_a_source_sized_mask_is_undistorted_like_its_photo(tmp_path):
    """A tiny COLMAP folder with distorted cameras and a half-plane mask per photo: where the dataset resampled the photo
    the loaded mask is undistort_image of the replicated mask with that camera's own intrinsics, soft only along the
    edge; where it did not, the file's bytes."""
    import colmap_cases as CC
    from PIL import Image
    from tinysplat_amd import Dataset
    from tinysplat_amd.dataset import undistort_image
    CC.write(tmp_path / "sparse")
    CC.write_images(tmp_path / "images")
    (tmp_path / "masks").mkdir()
    half = np.zeros((CC.H, CC.W), np.uint8)
    half[:, :CC.W // 2] = 1                                          # nonzero means keep
    dataset = Dataset(tmp_path / "sparse", tmp_path / "images", device=DEV)
    for cam in dataset.cameras:
        Image.fromarray(half).save(tmp_path / "masks" / (cam.name + ".png"))
    masks = TrainingMasks(dataset, tmp_path / "masks", DEV)
    assert len(masks) == len(dataset.cameras) and any(dataset.resampled) and not all(dataset.resampled)
    source = torch.from_numpy(np.repeat((half * 255)[:, :, None], 3, axis=2).copy()).to(DEV)
    for i, cam in enumerate(dataset.cameras):
        got = masks[i]
        assert got.dtype == torch.uint8 and got.shape == (cam.height, cam.width) and got.is_contiguous()
        if not dataset.resampled[i]:
            assert torch.equal(got, source[:, :, 0])
            continue
        s = dataset.setups[i]
        want = undistort_image(source, s.src_k, s.dst_k, s.dist, s.out_size)
        assert torch.equal(got, want[:, :, 0]) and torch.equal(want[:, :, 0], want[:, :, 1])
        rows = got.cpu().numpy().astype(np.int32)
        soft = (rows != 0) & (rows != 255)
        # every row runs from kept through at most a few soft pixels to ignored: bilinear samples of a step edge
        assert np.all(np.diff(rows, axis=1) <= 0), cam.name
        assert soft.any() and soft.sum(axis=1).max() <= 3, (cam.name, soft.sum(axis=1).max())
        assert np.all(rows[:, 0] == 255) and np.all(rows[:, -1] == 0)


# ---- the tools
def _tool(name):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location(f"tool_{name}", Path(__file__).resolve().parent.parent / "tools" / f"{name}.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_training_and_evaluation_tools_with_masks(tmp_path, capsys):
    """tools/train.py --masks-dir --mask-classes --eval-holdout on a six-camera COLMAP folder trains under the combined
    masks and reports the held-out views over their kept pixels; tools/eval.py --masks-dir measures the same views the same
    way, and differently from the unmasked evaluation."""
    import colmap_cases as CC
    from PIL import Image
    base = tmp_path / "scene"
    CC.write(base / "colmap" / "sparse" / "0")
    CC.write_images(base / "images")
    (base / "masks").mkdir()
    (base / "semantic").mkdir()
    half = np.zeros((CC.H, CC.W), np.uint8)
    half[:, :CC.W // 2] = 255
    labels = np.zeros((CC.H, CC.W), np.uint8)
    labels[10:20, 5:15] = 3
    for im in CC.reconstruction()[1]:
        name = im["name"].rsplit("/", 1)[-1]
        Image.fromarray(half).save(base / "masks" / (name + ".png"))
        np.save(base / "semantic" / (name + ".npy"), labels)
    scene_path = tmp_path / "scene.ply"
    _tool("train").main(["--dataset-dir", str(base), "--max-iter", "4", "--sh-degree", "1", "--masks-dir", "masks",
                         "--mask-classes", "3", "--semantic-dir", "semantic", "--semantic-classes", "5", "--mask-dilate", "2",
                         "--eval-holdout", "3", "--output", str(scene_path)])
    out = capsys.readouterr().out
    assert "masks for 6 cameras" in out and "% of the pixels kept" in out and "4 training cameras, 2 held out" in out
    assert "PSNR" in out and scene_path.exists()
    kept = float(out.split("masks for 6 cameras: ")[1].split(" %")[0])
    assert 35.0 < kept < 50.0                                         # half the frame less the labelled block
    tables = []
    for extra in (["--masks-dir", "masks"], []):
        _tool("eval").main([str(scene_path), "--dataset-dir", str(base), "--holdout", "3"] + extra)
        out = capsys.readouterr().out
        assert ("over the masks' kept pixels" in out) == bool(extra) and "mean" in out
        tables.append([line for line in out.splitlines() if line.startswith("mean")][0])
    assert tables[0] != tables[1]
