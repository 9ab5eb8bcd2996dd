"""Shared test helpers: scene -> boundary arguments, oracle frame, comparison utilities."""
from pathlib import Path

import numpy as np
import torch

from oracle import gsplat_oracle as O
from tinysplat_amd.rasterizer import project_args, raster_args, sh_args, tile_bounds
from tinysplat_amd.synthetic import make_scene


GOLD = Path(__file__).resolve().parent / "golden"


def load_golden(name):
    """The arrays of tests/golden/<name>.npz, with those of <name>.post.npz (the expected state after the operation)
    merged in where a fixture is stored in two files to keep every committed file below 1 MiB."""
    z = dict(np.load(GOLD / f"{name}.npz"))
    post = GOLD / f"{name}.post.npz"
    if post.exists():
        z.update(np.load(post))
    return z


def scene_args(n, sh_degree, width, height, seed=0, scale_mult=1.0, device="cpu", dtype=None):
    model, cam = make_scene(n, sh_degree, width, height, seed=seed, scale_mult=scale_mult)
    if dtype is not None:
        for name in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
            setattr(model, name, getattr(model, name).to(dtype))
    if device != "cpu":
        model = model.to(device)
    return model, cam


def oracle_frame(model, cam, dims, depth=True, raster_dtype=None, correct_viewdirs=False, conics_from=None):
    """The reference frame recipe (rasterize.py:26-62) executed with the oracle ops on CPU.
    ``raster_dtype=torch.float64``: projection, SH and binning as given (float32, bit-exact radii and
    lists), compositing arithmetic in float64 on those 2-D inputs.
    ``conics_from``: an [N,3] tensor of conic VALUES to composite (the ones the path under test projected) - the
    oracle's own conics keep their place in the autograd graph (their Jacobian carries the gradient), only the values
    are replaced.  For scenes whose projection is ill-conditioned (needles: a 1-ulp difference in exp(log-scale) moves
    a conic by 1e-4 of its size, which flips alpha >= 1/255 decisions the stability margin calls safe): the
    compositing and the projection are then each checked on their own inputs (tools/fuzz_frame.py)."""
    pa = project_args(model, cam, dims, "cpu")
    xys, depths, radii, conics, nth, cov3d = O.project_gaussians(*pa)
    if conics_from is not None:
        conics = conics + (conics_from.to(conics.dtype) - conics).detach()
    if xys.requires_grad:
        xys.retain_grad()
    colors = torch.clamp(O.spherical_harmonics(*sh_args(model, cam, "cpu", correct_viewdirs)) + 0.5, min=0.0)
    rgb, _, aux = O.rasterize_gaussians(*raster_args(model, xys, depths, radii, conics, nth, colors, dims),
                                        return_aux=True, compute_dtype=raster_dtype)
    rgb = torch.clamp(rgb, max=1.0)
    out = {"rgb": rgb, "xys": xys, "depths": depths, "radii": radii, "conics": conics, "nth": nth,
           "cov3d": cov3d, "colors": colors, "aux": aux}
    if depth:
        d, _ = O.rasterize_gaussians(*raster_args(model, xys, depths, radii, conics, nth,
                                                  depths[:, None].repeat(1, 3), dims),
                                      compute_dtype=raster_dtype)
        out["depth"] = d[:, :, 0]
    return out


IMAGE_LOG = []           # (test, what, masked max err, unmasked max err, masked fraction); printed by conftest


def assert_close_masked(a, b, atol, mask=None, max_bad_frac=0.0, what="", scale_by_value=False):
    """|a - b| <= atol per entry (``scale_by_value``: atol * max(1, |b|) per entry - the north_star's 1e-5
    taken relative for values above 1, e.g. a depth image whose values reach 10)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    if scale_by_value:
        err = err / b.abs().clamp_min(1.0)
    if mask is not None:
        unmasked = err.max().item() if err.numel() else 0.0
        m = mask
        while m.dim() < err.dim():
            m = m[..., None]
        err = torch.where(m.expand_as(err), err, torch.zeros_like(err))
        # the worst error over ALL pixels is recorded beside the asserted one (printed at the end of the session)
        import os
        test = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
        IMAGE_LOG.append((test, what, err.max().item() if err.numel() else 0.0, unmasked,
                          1.0 - mask.double().mean().item()))
    bad = (err > atol).double().mean().item()
    assert bad <= max_bad_frac, f"{what}: {bad:.3e} of entries exceed {atol} (max err {err.max():.3e})"


def report_unmasked(what, a, b, mask, scale_by_value=False):
    """Records the worst image error over ALL pixels beside the worst over the threshold-stable ones (the value
    checks assert on the latter): an error confined to the pixels the mask removes is visible in the report."""
    import os
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    if scale_by_value:
        err = err / b.abs().clamp_min(1.0)
    m = mask
    while m.dim() < err.dim():
        m = m[..., None]
    masked = torch.where(m.expand_as(err), err, torch.zeros_like(err)).max().item() if err.numel() else 0.0
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
    IMAGE_LOG.append((test, what, masked, err.max().item() if err.numel() else 0.0, 1.0 - mask.double().mean().item()))
    return masked, err.max().item() if err.numel() else 0.0


# --------------------------------------------------------------------------------------------------
# gradient comparison with a record of what was actually measured
# --------------------------------------------------------------------------------------------------
PARITY_LOG = []          # (test, tensor, max_abs_err, ref_inf_norm, tol, frac_over, frac_within_1e-5_abs, frac_entrywise); printed by conftest
ABS_BAR = 1e-5           # BASELINE.json north_star: "within 1e-5 abs on rendered RGB/depth and gradients"
ENTRYWISE_MIN = 0.99     # share of a tensor's entries that must meet 1e-5 * max(1, |ref ENTRY|) (see check_grad)
ENTRYWISE_NUMEL = 1000   # ... asserted on tensors with at least this many entries, recorded for all


def check_grad(what: str, got, ref, rel: float = 1e-5, max_bad_frac: float = 0.0, mask=None,
               entrywise_min: float = ENTRYWISE_MIN, entrywise_scale: float = 1.0, entry_extra=None):
    """What is enforced, per tensor:
      * |ref|_inf <= 1: the north_star's literal bar, |got - ref| <= 1e-5 ABSOLUTE for every entry
        (whatever ``rel`` says; times ``entrywise_scale`` where a fuzz scene's measured conditioning set one);
      * |ref|_inf > 1: |got - ref| <= rel * |ref|_inf per entry (float32 cannot hold 1e-5 absolute on a
        gradient of magnitude 1e3: one ulp of 1e3 is 6e-5);
    for all but ``max_bad_frac`` of the entries; AND, so that the infinity-norm scaling cannot excuse the small
    entries of a large-norm tensor,
      * at least ``entrywise_min`` (99 %) of the entries within 1e-5 * max(1, |ref ENTRY|) - the bar taken relative
        to the entry's own magnitude.  Every call records the worst absolute error, the
    reference magnitude, the worst error / tolerance and the fraction of entries within 1e-5 absolute,
    which the GPU test session prints at its end (and writes to gpurun_out/parity_report.txt)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    if mask is not None:
        m = mask
        while m.dim() < err.dim():
            m = m[..., None]
        err = torch.where(m.expand_as(err), err, torch.zeros_like(err))
    mag = ref.abs().max().item() if ref.numel() else 0.0
    # (|ref|_inf <= 1 on a scene whose measured conditioning allows entrywise_scale x the plain bar: the absolute bar
    # grows in the same proportion - otherwise a needle scene with |ref|_inf 0.99 would be held to a tolerance ten
    # times tighter than the same scene with |ref|_inf 1.01; fuzz seed 400.  Plain calls: entrywise_scale = 1.)
    tol = ABS_BAR * max(1.0, entrywise_scale) if mag <= 1.0 else rel * mag
    worst = err.max().item() if err.numel() else 0.0
    frac = (err > tol).double().mean().item() if err.numel() else 0.0
    within = (err <= ABS_BAR).double().mean().item() if err.numel() else 1.0
    # (entrywise_scale > 1: randomised scenes whose measured float32 conditioning allows more than the plain bar - the
    # entry-wise bar grows with the tolerance instead of being dropped, tools/fuzz_frame.py)
    # (entry_extra: an absolute allowance per entry on top of the entry-wise bar - the first-order propagation of float32
    # rounding of the 2-D gradients through the projection VJP, measured on the oracle's graph: tools/fuzz_frame.py)
    bar = entrywise_scale * ABS_BAR * ref.abs().clamp_min(1.0)
    if entry_extra is not None:
        bar = bar + entry_extra.detach().cpu().double()
    entrywise = (err <= bar).double().mean().item() if err.numel() else 1.0
    import os
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
    PARITY_LOG.append((test, what, worst, mag, tol, frac, within, entrywise))
    if os.environ.get("TS_PARITY_REPORT_ONLY") == "1":       # survey run: record, do not fail (conftest fails the session)
        return worst / tol if tol > 0 else 0.0
    assert frac <= max_bad_frac, (f"{what}: {frac:.3e} of entries exceed {tol:.3e} "
                                  f"(max err {worst:.3e}, |ref|_inf {mag:.3e}); allowed {max_bad_frac:.1e}")
    # (asserted on tensors of >= ENTRYWISE_NUMEL entries: in a 14-Gaussian fuzz scene one entry is 2 % of a tensor)
    assert entrywise >= entrywise_min or err.numel() < ENTRYWISE_NUMEL, (
        f"{what}: only {entrywise:.4f} of the entries are within {entrywise_scale:g} x 1e-5 * max(1, |ref entry|) "
        f"(required {entrywise_min}; max err {worst:.3e}, |ref|_inf {mag:.3e})")
    return worst / tol if tol > 0 else 0.0
