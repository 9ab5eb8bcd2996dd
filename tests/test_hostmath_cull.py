"""The two alpha culls of tinysplat_amd/csrc/splat_math.h - ts::rect_may_contribute (per 8x8 block, raster.hip:
stage_splat) and ts::TightTest (per 16x16 tile, binning.hip) - compiled for the host and held to their written
contract: a rejection is a proof that no sample of the region reaches alpha >= 1/255.

Reference: alpha in float64 at every sample position of the region (tests/cull_cases.py, from the definition in
oracle/gsplat_oracle.py::rasterize_gaussians); the float32 operands are cast exactly.  SOUNDNESS carries no tolerance:
the culls' designed slack (0.02 in the log2 exponent) is orders of magnitude above float32 rounding, so one rejected
region that the reference calls needed is a bug in the header.  TEETH: a cull that rejects nothing fails too.  No GPU.
"""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import cull_cases as C
from oracle import gsplat_oracle as O
from tinysplat_amd.rasterizer import project_args, tile_bounds

from helpers import scene_args

ROOT = Path(__file__).resolve().parent.parent
N_BLOCK = 40000          # regions per block family
N_TILE = 1500            # Gaussians per tile family (each brings the tiles of its bounding box)
W, H = 640, 400


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _block_keep(hm, recs, rects):
    out = np.empty(len(recs), dtype=np.int32)
    hm.hm_rect_may_contribute(len(recs), _p(recs), _p(rects), _p(out))
    return out != 0


def _tile_keep(hm, recs, radii, w, h, tile_rows=None):
    """-> boxes, (gi, tx, ty) of every bounding-box pair, kept[pair]"""
    tbx, tby = tile_bounds((w, h))[:2]
    row0, rows = (0, tby) if tile_rows is None else (tile_rows[0], tile_rows[1] - tile_rows[0])
    n = len(recs)
    xys = np.ascontiguousarray(recs[:, :2])
    boxes = np.empty((n, 4), dtype=np.int32)
    hm.hm_tile_bbox(n, _p(xys), _p(radii.astype(np.float32)), tbx, tby, row0, rows, _p(boxes))
    gi, tx, ty, row_off, nrows = C.tile_pairs(boxes)
    lo = np.full(max(nrows, 1), -1, dtype=np.int32); hi = np.full(max(nrows, 1), -1, dtype=np.int32)
    row_off = np.ascontiguousarray(row_off.astype(np.int64))
    hm.hm_tight_rows(n, _p(recs), _p(np.ascontiguousarray(radii.astype(np.int32))), _p(boxes), _p(row_off), _p(lo), _p(hi))
    k = row_off[gi] + (ty - boxes[gi, 1])
    return boxes, (gi, tx, ty), (tx >= lo[k]) & (tx < hi[k])


def _report(kind, family, keep, amax):
    needed = amax >= C.ALPHA_MIN
    rej = ~keep
    worst = float(amax[rej].max()) * 255.0 if rej.any() else float("nan")
    ratio = keep.sum() / max(int(needed.sum()), 1)
    print(f"[cull] {kind:5s} {family:18s} regions {len(keep):7d}  needed {int(needed.sum()):7d}  kept {int(keep.sum()):7d}  "
          f"kept/needed {ratio:6.3f}  rejected {int(rej.sum()):7d}  largest rejected alpha*255 {worst:.4f}")
    return needed, rej


def _assert_sound(kind, family, recs, keep, amax, extra=None):
    needed, rej = _report(kind, family, keep, amax)
    bad = np.nonzero(rej & needed)[0]
    if len(bad):
        i = bad[np.argmax(amax[bad])]
        raise AssertionError(f"{kind} cull, family {family}: {len(bad)} rejected regions are NEEDED; worst: case {i}, "
                             f"alpha*255 = {amax[i] * 255.0:.6f}, record {recs[i if extra is None else extra[0][i]].tolist()}"
                             + ("" if extra is None else f", tile ({extra[1][i]}, {extra[2][i]})"))
    return needed, rej


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.BLOCK_FAMILIES)
def test_block_cull_rejects_only_what_float64_calls_unneeded(hostmath, family):
    recs, rects = C.block_cases(family, seed=1000 + C.BLOCK_FAMILIES.index(family), n=N_BLOCK)
    keep = _block_keep(hostmath, recs, rects)
    amax = C.block_alpha_max(recs, rects)
    needed, rej = _assert_sound("block", family, recs, keep, amax)
    # teeth: the family decides near the boundary (needed and unneeded both present) and the cull does reject
    assert needed.any() and (~needed).any()
    assert rej.any(), f"{family}: nothing rejected"


def test_block_families_hold_enough_regions():
    assert N_BLOCK * len(C.BLOCK_FAMILIES) >= 100000


def test_block_cull_keeps_everything_for_conics_that_are_not_positive_definite(hostmath):
    """zero / negative diagonal entries: stage_splat has no geometric cull.  |b| >= sqrt(a c) with a positive diagonal
    goes through rect_may_contribute: whatever it returns there must still be sound."""
    recs, rects = C.block_cases("non_psd", seed=77, n=N_BLOCK)
    keep = _block_keep(hostmath, recs, rects)
    diag_bad = (recs[:, 3] <= 0) | (recs[:, 5] <= 0)
    assert diag_bad.sum() > N_BLOCK // 2
    assert keep[diag_bad].all()
    rest = ~diag_bad
    _assert_sound("block", "non_psd", recs[rest], keep[rest], C.block_alpha_max(recs[rest], rects[rest]))


def test_block_cull_opacity_gate(hostmath):
    """opacity <= 0 and opacity below 1/255 * 2^-0.02 reject every block (alpha <= opacity < 1/255 for a PSD conic)"""
    recs, rects = C.block_cases("axis_ratio", seed=5, n=2000)
    recs[:1000, 2] = 0.0
    recs[1000:, 2] = np.float32(C.ALPHA_MIN * 2.0 ** -0.03)
    assert not _block_keep(hostmath, recs, rects).any()
    assert (C.block_alpha_max(recs, rects) < C.ALPHA_MIN).all()


def test_min_form_on_rect_is_a_lower_bound_of_the_form_on_the_samples(hostmath):
    """ts::min_form_on_rect against the smallest value of the form over the rectangle's sample positions in float64:
    never above it by more than float32 rounding of the form's terms (4e-6 mag is what rect_may_contribute allows),
    and equal to it for a one-pixel rectangle."""
    recs, rects = C.block_cases("axis_ratio", seed=11, n=N_BLOCK)
    q = recs.astype(np.float64)
    log2e = 1.4426950408889634
    forms = np.ascontiguousarray(np.stack([0.5 * log2e * q[:, 3], log2e * q[:, 4], 0.5 * log2e * q[:, 5]], 1).astype(np.float32))
    off = np.ascontiguousarray(np.stack([recs[:, 0] - rects[:, 1], recs[:, 0] - rects[:, 0],
                                         recs[:, 1] - rects[:, 3], recs[:, 1] - rects[:, 2]], 1).astype(np.float32))
    got = np.empty(len(recs), dtype=np.float32)
    hostmath.hm_min_form_on_rect(len(recs), _p(forms), _p(off), _p(got))
    # smallest sigma' over the samples = -log2(alpha_max / opacity) with opacity 1
    one = recs.copy(); one[:, 2] = 1.0
    with np.errstate(divide="ignore"):
        ref = -np.log2(C.block_alpha_max(one, rects))
    f = forms.astype(np.float64); o = np.abs(off.astype(np.float64))
    dxm, dym = o[:, :2].max(1), o[:, 2:].max(1)
    mag = f[:, 0] * dxm * dxm + f[:, 2] * dym * dym + np.abs(f[:, 1]) * dxm * dym
    fin = np.isfinite(ref)
    assert fin.mean() > 0.9
    assert (got[fin] <= ref[fin] + 4e-6 * mag[fin] + 1e-6).all()
    single = fin & (rects[:, 0] == rects[:, 1]) & (rects[:, 2] == rects[:, 3])
    assert single.sum() > 100
    assert (np.abs(got[single] - ref[single]) <= 4e-6 * mag[single] + 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------------------------------
def _tile_family_check(hm, family, seed, n, pix_off=0.0, tile_rows=None):
    recs, radii = C.tile_cases(family, seed, n, W, H, pix_off=pix_off)
    boxes, (gi, tx, ty), keep = _tile_keep(hm, recs, radii, W, H, tile_rows)
    amax = C.tile_alpha_max(recs, gi, tx, ty, pix_off=pix_off)
    return _assert_sound("tile", family, recs, keep, amax, extra=(gi, tx, ty)), len(gi)


@pytest.mark.parametrize("family", C.TILE_FAMILIES)
def test_tight_rows_reject_only_what_float64_calls_unneeded(hostmath, family):
    (needed, rej), pairs = _tile_family_check(hostmath, family, 2000 + C.TILE_FAMILIES.index(family), N_TILE)
    assert pairs >= 10000, pairs
    assert needed.any() and (~needed).any()
    assert rej.any(), f"{family}: nothing rejected"


def test_tight_rows_on_a_tile_row_stripe(hostmath):
    """tile_row0 > 0: the box rows are clipped to the stripe, the decisions are those of the full frame"""
    recs, radii = C.tile_cases("axis_ratio", 2100, N_TILE, W, H)
    _, (gi, tx, ty), keep = _tile_keep(hostmath, recs, radii, W, H)
    full = set(zip(gi[keep].tolist(), tx[keep].tolist(), ty[keep].tolist()))
    got = set()
    tby = tile_bounds((W, H))[1]
    for r0, r1 in ((0, 7), (7, 8), (8, tby)):
        _, (g2, x2, y2), k2 = _tile_keep(hostmath, recs, radii, W, H, tile_rows=(r0, r1))
        assert ((y2 >= r0) & (y2 < r1)).all()
        got |= set(zip(g2[k2].tolist(), x2[k2].tolist(), y2[k2].tolist()))
    assert got == full


def test_tight_rows_keep_the_box_for_conics_that_are_not_positive_definite(hostmath):
    recs, radii = C.tile_cases("axis_ratio", 2200, N_TILE, W, H)
    k = np.arange(len(recs)) % 5
    g = np.sqrt(recs[:, 3] * recs[:, 5])
    recs[:, 4] = np.where(k == 0, g * 1.5, recs[:, 4])
    recs[:, 3] = np.where(k == 1, 0.0, np.where(k == 2, -recs[:, 3], recs[:, 3]))
    recs[:, 5] = np.where(k == 3, 0.0, np.where(k == 4, -recs[:, 5], recs[:, 5]))
    _, (gi, _, _), keep = _tile_keep(hostmath, recs, radii, W, H)
    assert len(gi) > 10000 and keep.all()


def test_tight_rows_opacity_gate(hostmath):
    recs, radii = C.tile_cases("axis_ratio", 2300, 500, W, H)
    recs[:250, 2] = 0.0
    recs[250:, 2] = np.float32(C.ALPHA_MIN * 2.0 ** -0.03)
    _, (gi, tx, ty), keep = _tile_keep(hostmath, recs, radii, W, H)
    assert len(gi) > 1000 and not keep.any()
    assert (C.tile_alpha_max(recs, gi, tx, ty) < C.ALPHA_MIN).all()


def test_tile_families_hold_enough_regions(hostmath):
    total = 0
    for family in C.TILE_FAMILIES:
        recs, radii = C.tile_cases(family, 2000 + C.TILE_FAMILIES.index(family), N_TILE, W, H)
        total += len(_tile_keep(hostmath, recs, radii, W, H)[1][0])
    assert total >= 100000, total


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of the two tight-binning GPU tests: the tight lists drop a real share of the bounding-box pairs
# ---------------------------------------------------------------------------------------------------------------------
def _projected(model, cam, w, h):
    xys, _, radii, conics, nth, _ = O.project_gaussians(*project_args(model, cam, (w, h), "cpu"))
    live = (radii > 0).numpy()
    op = torch.sigmoid(model.opacities)[:, 0].numpy()
    recs = C.records_of(xys[:, 0].numpy(), xys[:, 1].numpy(), op, conics[:, 0].numpy(), conics[:, 1].numpy(),
                        conics[:, 2].numpy())
    return recs[live], radii.numpy()[live], int(nth.sum())


def _scene_check(hm, name, model, cam, w, h):
    recs, radii, bbox_pairs = _projected(model, cam, w, h)
    _, (gi, tx, ty), keep = _tile_keep(hm, recs, radii, w, h)
    assert len(gi) == bbox_pairs                        # the pairs walked here are the oracle's num_tiles_hit
    # soundness on a 1/16 sample of the scene's Gaussians (all tiles of every 16th); the share below is of ALL pairs
    sel = gi % 16 == 0
    amax = C.tile_alpha_max(recs, gi[sel], tx[sel], ty[sel])
    _assert_sound("tile", name + " 1/16", recs, keep[sel], amax, extra=(gi[sel], tx[sel], ty[sel]))
    share = keep.sum() / bbox_pairs
    print(f"[cull] scene {name}: bounding-box pairs {bbox_pairs}, tight pairs {int(keep.sum())}, share {share:.4f}")
    assert keep.sum() <= 0.85 * bbox_pairs, (name, int(keep.sum()), bbox_pairs)


@pytest.mark.parametrize("mult,seed", [(2.0, 5), (6.0, 6)])
def test_tight_rows_drop_a_real_share_of_the_random_scene(hostmath, mult, seed):
    """the scene of test_tight_binning_drops_only_pairs_that_contribute_nothing, and its bound"""
    n, w, h = 50000, 480, 270
    model, cam = scene_args(n, 1, w, h, seed=seed, scale_mult=mult)
    _scene_check(hostmath, f"make_scene x{mult:g}", model, cam, w, h)


def test_tight_rows_drop_a_real_share_of_the_stress_scene(hostmath):
    """the scene of test_tight_binning_stress_anisotropic_faint_and_opaque"""
    n, w, h = 60000, 416, 240
    model, cam = scene_args(n, 0, w, h, seed=33, scale_mult=1.0)
    g = torch.Generator().manual_seed(34)
    z = model.means[:, 2:3]
    model.scales = torch.log(z) + torch.empty(n, 3).uniform_(math.log(2e-4), math.log(0.25), generator=g)
    logit = torch.empty(n, 1).uniform_(-5.6, 9.0, generator=g)
    logit[: n // 10] = -5.53 + 0.02 * torch.rand(n // 10, 1, generator=g)
    model.opacities = logit
    _scene_check(hostmath, "stress", model, cam, w, h)


# ---------------------------------------------------------------------------------------------------------------------
# the other sample convention: TS_PIX_OFF = 0.5
# ---------------------------------------------------------------------------------------------------------------------
def test_culls_are_sound_in_the_half_pixel_build(tmp_path):
    so = tmp_path / "_hostmath_pixoff.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-DTS_PIX_OFF=0.5f",
                    str(ROOT / "tests" / "hostmath" / "hostmath.cpp"), "-o", str(so)], check=True)
    hm = ctypes.CDLL(str(so))
    rejected = 0
    for family in C.BLOCK_FAMILIES:
        recs, rects = C.block_cases(family, seed=3000 + C.BLOCK_FAMILIES.index(family), n=N_BLOCK // 4, pix_off=0.5)
        keep = _block_keep(hm, recs, rects)
        _assert_sound("block", family + " +0.5", recs, keep, C.block_alpha_max(recs, rects))
        rejected += int((~keep).sum())
    for family in C.TILE_FAMILIES:
        (_, rej), _ = _tile_family_check(hm, family, 4000 + C.TILE_FAMILIES.index(family), N_TILE // 3, pix_off=0.5)
        assert rej.any(), family
    assert rejected > 0
    # the switch matters: the default build, given the same records, decides some of these tiles differently
    recs, radii = C.tile_cases("axis_ratio", 4100, N_TILE, W, H, pix_off=0.5)
    _, _, keep5 = _tile_keep(hm, recs, radii, W, H)
    so0 = tmp_path / "_hostmath_default.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "hostmath.cpp"), "-o", str(so0)], check=True)
    _, _, keep0 = _tile_keep(ctypes.CDLL(str(so0)), recs, radii, W, H)
    assert (keep5 != keep0).any()


# ---------------------------------------------------------------------------------------------------------------------
# the block cases as compositing inputs (cull_cases.composite_inputs), judged by the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
def test_compositing_inputs_stay_under_the_masked_share_cap():
    """tests/test_gpu_parity.py::_raster_parity masks the pixels whose float64 decision margin is below 1e-4 and caps
    their share at 5e-3: the block cases, rendered as an image, must leave room under that cap (so that they can be
    handed to it), and the image must be neither empty nor saturated."""
    xys, depths, radii, conics, colors, opac, bg = (torch.from_numpy(a) for a in C.composite_inputs())
    w, h = C.COMPOSITE_W, C.COMPOSITE_H
    minx, miny, maxx, maxy = O.tile_bbox(xys, radii, tile_bounds((w, h)))
    nth = ((maxx - minx) * (maxy - miny)).to(torch.int32)
    radii = torch.where(nth > 0, radii, torch.zeros_like(radii))
    img, alpha, aux = O.rasterize_gaussians(xys.double(), depths.double(), radii, conics.double(), nth, colors.double(),
                                            opac.double(), h, w, bg.double(), return_aux=True)
    masked = (aux["margin"] <= 1e-4).double().mean().item()
    lens = (aux["tile_bins"][:, 1] - aux["tile_bins"][:, 0]).double()
    print(f"[cull] compositing inputs: {len(xys)} Gaussians, {int(nth.sum())} pairs, mean list {lens.mean():.1f}, "
          f"masked share {masked:.2e}, mean alpha {alpha.mean():.3f}")
    assert masked < 2.5e-3                              # half the cap of _raster_parity
    assert (alpha > 0.01).double().mean() > 0.3 and (alpha < 0.9).double().mean() > 0.3
