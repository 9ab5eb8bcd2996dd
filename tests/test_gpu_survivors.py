"""SURVIVOR LISTS (csrc/raster.hip, frame.SURVIVORS): the backward compositing pass replays the entries the forward pass
staged instead of re-culling the lists.  Everything a frame computes must be bitwise what the re-culling replay computes:
image, final_Ts, final_index, the gradient rows (flags and the rows they flag), every parameter gradient - compared in one
process with the flag on and off, on the full-size frame (RGB, RGB + depth), config 2, hybrid launches forced into other
(S, W16, C16) shapes, fuzz scenes, and three training steps."""
import sys
from pathlib import Path

import pytest
import torch

from tinysplat_amd import frame
from tinysplat_amd.rasterizer import GaussianRasterizer

from helpers import scene_args

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Capture:
    """keeps the last frame's compositing state alive for inspection (final_Ts / final_index / partials / row flags)"""

    def __init__(self):
        self.frames = []

    def __enter__(self):
        self.orig = frame._forward

        def fwd(*a, **k):
            F = self.orig(*a, **k)
            self.frames.append(F)
            return F
        frame._forward = fwd
        return self

    def __exit__(self, *exc):
        frame._forward = self.orig
        return False


def _render(model, cam, dims, sh, depth, seed=5):
    w, h = dims
    g = torch.Generator().manual_seed(seed)
    w_rgb = torch.rand(h, w, 3, generator=g).to(DEV)
    w_d = torch.rand(h, w, generator=g).to(DEV)
    md = model.to(DEV).requires_grad_(True)
    r = GaussianRasterizer(md, None, device=torch.device(DEV))
    with _Capture() as cap:
        rgb, ex = r(cam, dims, sh)
        F = cap.frames[-1]
        base, px = F.wf.data_ptr(), h * w    # final_Ts / final_index live in the frame's workspace
        fin = torch.cat([F.wf[F.fr.final_Ts - base:][:4 * px].clone(), F.wf[F.fr.final_index - base:][:4 * px].clone()])
        loss = (rgb * w_rgb).sum() + ((ex["depth"] * w_d).sum() if depth else 0.0)
        loss.backward()
    torch.cuda.synchronize()
    out = [rgb.detach(), fin] + ([ex["depth"].detach()] if depth else []) + [ex["xys"].grad]
    return out + [p.grad.clone() for p in md.parameters()], F


def _both(model, cam, dims, sh=3, depth=False):
    saved = (frame.SURVIVORS, frame.WIDE_TILES)
    res = []
    try:
        frame.WIDE_TILES = 0                 # 16x16 lists whatever earlier frames on the device looked like
        for on in (False, True):
            frame.SURVIVORS = on
            out, F = _render(model, cam, dims, sh, depth)
            res.append(out)
            assert bool(F.fr.flags & 512) == on, F.fr.flags          # the survivor path really ran
    finally:
        frame.SURVIVORS, frame.WIDE_TILES = saved
    for a, b in zip(*res):
        assert a.shape == b.shape and torch.equal(a, b)
    return res


@pytest.mark.parametrize("depth", [False, True])
def test_config3_bitwise(depth):
    model, cam = scene_args(1_000_000, 3, 1920, 1080, seed=0)
    _both(model, cam, (1920, 1080), 3, depth)


def test_config2_bitwise():
    model, cam = scene_args(100_000, 3, 1920, 1080, seed=0)
    _both(model, cam, (1920, 1080), 3, True)


def test_partials_and_row_flags_bitwise():
    """the raw gradient rows: same slots flagged, same values in them"""
    from tinysplat_amd import _lib
    model, cam = scene_args(200_000, 3, 1280, 720, seed=3)
    saved, got = frame.SURVIVORS, []
    orig = frame.row_flags_for
    try:
        for on in (False, True):
            frame.SURVIVORS = on
            keep = {}

            def flags_for(dev, rows):
                t, gen = orig(dev, rows)
                keep["flags"], keep["gen"], keep["rows"] = t, gen, rows
                return t, gen
            frame.row_flags_for = flags_for
            orig_empty = torch.empty
            parts = {}

            def empty(*a, **k):
                t = orig_empty(*a, **k)
                if len(a) == 1 and isinstance(a[0], tuple) and len(a[0]) == 2 and a[0][1] == _lib.PARTIAL_ROW_FLOATS:
                    parts["p"] = t
                return t
            torch.empty = empty
            try:
                _render(model, cam, (1280, 720), 3, False)
            finally:
                torch.empty = orig_empty
            rows = keep["rows"]
            flagged = keep["flags"][:rows] == keep["gen"]
            got.append((flagged.clone(), parts["p"][:rows][flagged].clone()))
    finally:
        frame.SURVIVORS, frame.row_flags_for = saved, orig
    assert torch.equal(got[0][0], got[1][0]) and int(got[0][0].sum()) > 0
    assert torch.equal(got[0][1], got[1][1])


@pytest.mark.parametrize("segs,w16,c16", [(8, 13, 3), (4, 0, 0), (2, 15, 15), (8, 6, 6), (3, 10, 0)])
def test_forced_hybrid_shapes_bitwise(segs, w16, c16):
    """W16 = 0: every tile cut into list segments; C16 = W16 = 15: nearly every tile a cooperative workgroup"""
    saved = (frame.HYBRID_SEGS, frame.HYBRID_WHOLE16, frame.HYBRID_COOP16)
    try:
        frame.HYBRID_SEGS, frame.HYBRID_WHOLE16, frame.HYBRID_COOP16 = segs, w16, c16
        model, cam = scene_args(400_000, 3, 1920, 1080, seed=1)
        _both(model, cam, (1920, 1080), 3, True)
        assert frame.last_segments[0] == segs
    finally:
        frame.HYBRID_SEGS, frame.HYBRID_WHOLE16, frame.HYBRID_COOP16 = saved


@pytest.mark.parametrize("seed", [3, 7, 17, 42, 400, 578, 595])
def test_fuzz_scenes_bitwise(seed):
    """fuzz scenes (needles among them), composited one wave per tile with hybrid shapes even on small images"""
    import fuzz_frame
    case = fuzz_frame.draw_case(seed)
    model, cam = fuzz_frame.build(case)
    saved = (frame.SPLIT_BLOCKS_BELOW, frame.HYBRID_FROM, frame.LIST_SEGMENTS_FROM, frame.WIDE_TILES)
    try:
        frame.SPLIT_BLOCKS_BELOW, frame.HYBRID_FROM, frame.LIST_SEGMENTS_FROM, frame.WIDE_TILES = 0, 1, 1, 0
        _both(model, cam, case["dims"], case["sh"], True)
    finally:
        frame.SPLIT_BLOCKS_BELOW, frame.HYBRID_FROM, frame.LIST_SEGMENTS_FROM, frame.WIDE_TILES = saved


def test_training_steps_bitwise():
    """three TrainStep steps (fused Adam, RGB + depth loss) on a full-size frame: parameters and both moments"""
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import TrainStep
    n, sh, w, h = 300_000, 3, 1920, 1080
    target_model, cam = make_scene(n, sh, w, h, seed=11)
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(target_model.to(DEV), None, device=torch.device(DEV))(cam, None, sh)
    tgt, tgt_d = tgt.clone(), extras["depth"].clone()
    gen = torch.Generator(device="cpu").manual_seed(12)
    start, _ = make_scene(n, sh, w, h, seed=11)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(n, 3, generator=gen)
    start.means = start.means + 0.02 * torch.randn(n, 3, generator=gen)
    saved, runs = frame.SURVIVORS, []
    try:
        for on in (False, True):
            frame.SURVIVORS = on
            model = start.to(DEV)
            for nm in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
                setattr(model, nm, getattr(model, nm).detach().clone())
            step = TrainStep(model, DEV)
            outs = [step(cam, tgt, tgt_d) for _ in range(3)]
            runs.append((model, step.optimizer, outs))
    finally:
        frame.SURVIVORS = saved
    (m0, o0, r0), (m1, o1, r1) = runs
    for a, b in zip(r0, r1):
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["xys_grad"], b["xys_grad"])
    for nm in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
        assert torch.equal(getattr(m0, nm), getattr(m1, nm)), nm
        assert torch.equal(o0.exp_avg[nm], o1.exp_avg[nm]) and torch.equal(o0.exp_avg_sq[nm], o1.exp_avg_sq[nm]), nm
