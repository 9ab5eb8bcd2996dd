"""Inputs shared by tests/test_antialias_cpu.py and tests/test_gpu_antialias.py: the covariance triples of the header
check with their rounding bound, the g++ build of tests/hostmath/antialias.cpp, the Gaussians of the kernel checks, the
oracle's antialiased frame and the down-sampling scene."""
import ctypes
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

import antialias_oracle as AO
import pose_cases as PC

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
F32P = ctypes.POINTER(ctypes.c_float)
I32P = ctypes.POINTER(ctypes.c_int32)
BLUR32 = float(np.float32(0.3))          # the header's kBlur: the float32 nearest 0.3
U = 2.0 ** -24                           # unit roundoff of float32


# ---- the g++ build
def build_host(directory):
    """g++ build of tests/hostmath/antialias.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_antialias.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "antialias.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i64, i32 = ctypes.c_int64, ctypes.c_int
    lib.ah_triples.restype, lib.ah_triples.argtypes = None, [i64, F32P, F32P, F32P, F32P]
    lib.ah_exp.restype, lib.ah_exp.argtypes = None, [i64, F32P, F32P, F32P]
    lib.ah_fwd.restype, lib.ah_fwd.argtypes = None, [i64, F32P, F32P, F32P, F32P, F32P, i32, F32P, i32, F32P, F32P, F32P]
    lib.ah_bwd.restype, lib.ah_bwd.argtypes = None, [i64, I32P, F32P, F32P, i32, F32P, F32P]
    lib.ah_comp_bwd.restype, lib.ah_comp_bwd.argtypes = None, [i64, F32P, F32P, F32P, F32P, F32P, i32, F32P, F32P, F32P,
                                                               F32P]
    return lib


def _f(a):
    return a.ctypes.data_as(F32P)


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cam10(fx, fy, width, height, glob_scale=1.0, clip=0.01):
    return np.array([fx, fy, width / 2, height / 2, width, height, -(-width // 16), -(-height // 16), glob_scale, clip],
                    dtype=np.float32)


def host_triples(lib, triples, v):
    triples, v = _c32(triples), _c32(v)
    n = triples.shape[0]
    comp, G = np.full(n, 7.0, np.float32), np.full((n, 3), 7.0, np.float32)
    lib.ah_triples(n, _f(triples), _f(v), _f(comp), _f(G))
    return comp, G


def host_fwd(lib, means, scales, quats, view, cam, project_flags, opacity, raster_flags):
    """-> (comp [n], o_eff [n], rows [n, 4]) of the host build."""
    means, scales, quats, opacity = _c32(means), _c32(scales), _c32(quats), _c32(opacity).reshape(-1)
    view = _c32(np.asarray(view)[:3, :])
    n = means.shape[0]
    comp, o_eff, rows = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32), np.full((n, 4), 7.0, np.float32)
    lib.ah_fwd(n, _f(means), _f(scales), _f(quats), _f(view), _f(cam), project_flags, _f(opacity), raster_flags, _f(comp),
               _f(o_eff), _f(rows))
    return comp, o_eff, rows


def host_bwd(lib, radii, rows, opacity, raster_flags, v_opacity, v_conic):
    """-> (v_opacity [n], v_conic [n, 3]) after the host build's in-place update."""
    radii = np.ascontiguousarray(radii, dtype=np.int32)
    rows, opacity = _c32(rows), _c32(opacity).reshape(-1)
    v_opacity, v_conic = _c32(v_opacity).reshape(-1).copy(), _c32(v_conic).copy()
    lib.ah_bwd(radii.shape[0], radii.ctypes.data_as(I32P), _f(rows), _f(opacity), raster_flags, _f(v_opacity), _f(v_conic))
    return v_opacity, v_conic


def host_comp_bwd(lib, means, scales, quats, view, cam, project_flags, v_comp):
    means, scales, quats, v_comp = _c32(means), _c32(scales), _c32(quats), _c32(v_comp)
    view = _c32(np.asarray(view)[:3, :])
    n = means.shape[0]
    out = [np.full((n, 3), 7.0, np.float32), np.full((n, 3), 7.0, np.float32), np.full((n, 4), 7.0, np.float32)]
    lib.ah_comp_bwd(n, _f(means), _f(scales), _f(quats), _f(view), _f(cam), project_flags, _f(v_comp), *[_f(a) for a in out])
    return out


# ---- 1. covariance triples (a_o, b, c_o), float32
def regular_triples():
    """float32 [m, 3] with det_o clearly positive: isotropic sub-pixel (1e-4 .. 0.1), pixel-sized, large (1e3),
    anisotropic up to 100 : 1 with b at 0 and at +-(1 - 1e-3) sqrt(a_o c_o)."""
    rows = []
    for s in (1e-4, 3e-4, 1e-3, 1e-2, 0.1, 0.3, 1.0, 4.0, 1e3):
        rows.append((s, 0.0, s))
    for ratio in (2.0, 10.0, 100.0):
        for s in (1e-3, 0.05, 1.0, 30.0, 1e3):
            for k in (0.0, 0.5, 1.0 - 1e-3, -(1.0 - 1e-3)):
                rows.append((s * ratio, k * s * math.sqrt(ratio), s))
                rows.append((s, k * s * math.sqrt(ratio), s * ratio))
    return np.array(rows, dtype=np.float32)


def clamped_triples():
    """float32 [m, 3] on which both the float32 header and the float64 restatement clamp: a_o = 0, c_o = 0, b^2 = a_o c_o
    exactly (4 9 6; 1 1 1; 0.25 4 1), a det_o that is negative by a rounding (b one ulp above sqrt(a_o c_o)), an
    indefinite triple, zeros."""
    one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    rows = [(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (4.0, 6.0, 9.0), (1.0, 1.0, 1.0), (0.25, -1.0, 4.0),
            (1.0, one_up, 1.0), (1.0, -one_up, 1.0), (1e-3, 2e-3, 1e-3), (2.0, 5.0, 3.0)]
    return np.array(rows, dtype=np.float32)


def triple_gradients(n, seed=2):
    g = np.random.default_rng(seed)
    return (g.normal(size=n) * 10.0 ** g.uniform(-2, 1, size=n)).astype(np.float32)


def rounding_bound(triples, v):
    """How far the float32 header may be from the exact comp and G of the same float32 triples, to first order in
    u = 2^-24, with a FACTOR 2 on the whole for the second-order terms (and for the float64 reference's own rounding).

    det_o = a c - b^2: two products and a difference, |error| <= 2 u M_o with M_o = a c + b^2.
    det_b = (a + h)(c + h) - b^2: two sums, two products, a difference, |error| <= 4 u M_b with M_b = a_b c_b + b^2.
    comp = sqrt(det_o / det_b): a quotient (u) and a root (halves what came before, adds u):
        E_c = u (M_o / det_o + 2 M_b / det_b + 3/2)        relative.
    w = comp / det_o: E_w = E_c + 2 u M_o / det_o + u.
    G0 = -k (comp + h c w) with k = (h / 2) v: h c w carries E_w + 2 u, the sum u of itself, the product with k another
    2 u:  |error| <= |k| (E_c comp + (E_w + 2 u) h c w + 3 u (comp + h c w)); G2 likewise with a.
    G1 = 2 k h b w: |error| <= |G1| (E_w + 4 u).
    -> (bound of comp [m], bound of G [m, 3]), absolute."""
    t = np.asarray(triples, dtype=np.float64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    v = np.abs(np.asarray(v, dtype=np.float64))
    h = BLUR32
    ab, cb = a + h, c + h
    det_o, det_b = a * c - b * b, ab * cb - b * b
    M_o, M_b = np.abs(a * c) + b * b, np.abs(ab * cb) + b * b
    comp = np.sqrt(det_o / det_b)
    E_c = U * (M_o / det_o + 2.0 * M_b / det_b + 1.5)
    E_w = E_c + 2.0 * U * M_o / det_o + U
    w = comp / det_o
    k = 0.5 * h * v

    def diag(x):
        return k * (E_c * comp + (E_w + 2.0 * U) * h * x * w + 3.0 * U * (comp + h * x * w))
    G1 = 2.0 * k * h * np.abs(b) * w * (E_w + 4.0 * U)
    return 2.0 * E_c * comp, 2.0 * np.stack([diag(c), G1, diag(a)], axis=1)


# ---- 4. the Gaussians of the kernel checks: a 50 x 35 image (partial tiles) seen by a rotated camera
KW, KH = 50, 35
KERNEL_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
KINDS = ("regular", "behind", "off_screen", "beyond_fov", "sub_pixel", "underflow")


def kernel_view():
    return PC.view_matrix(quat=(0.9, 0.25, -0.3, 0.15), position=(0.4, -0.3, -0.6))


def kernel_gaussians(n, seed):
    """dict of float32 arrays for n Gaussians in PLAIN form (scales and unit quaternions as the projection takes them) and
    in RAW form (log-scales, unnormalised quaternions), logits, and ``kind`` [n]: index into KINDS - rows cycle through
    the kinds so that every n >= 6 holds each.  behind: z = -1 .. 0.005 (clip 0.01); off_screen: inside the fov clamp's
    1.3 but left of the image by more than the radius; beyond_fov: 1.4 .. 1.6 of the half extent, wide enough to matter;
    sub_pixel: projected sigma about 0.05 px; underflow: log-scales of -40 (det_o underflows: comp = 0)."""
    g = np.random.default_rng(seed)
    fx, fy, _ = PC.intrinsics(KW, KH)
    tan_x, tan_y = KW / (2 * fx), KH / (2 * fy)
    kind = (np.arange(n) + seed) % len(KINDS)
    z = g.uniform(2.0, 8.0, size=n)
    x = z * tan_x * g.uniform(-0.95, 0.95, size=n)
    y = z * tan_y * g.uniform(-0.95, 0.95, size=n)
    sigma = z[:, None] / fx * g.uniform(0.5, 4.0, size=(n, 3))             # 0.5 .. 4 px
    k = KINDS.index
    sel = kind == k("behind")
    z[sel] = g.choice([-1.0, 0.0, 0.005, -0.2], size=sel.sum())
    sel = kind == k("off_screen")
    x[sel] = -z[sel] * tan_x * 1.25             # (to the left: on the right the last tile reaches past the image)
    sigma[sel] = z[sel, None] / fx * 0.3
    sel = kind == k("beyond_fov")
    x[sel] = z[sel] * tan_x * g.uniform(1.4, 1.6, size=sel.sum()) * g.choice([-1.0, 1.0], size=sel.sum())
    sigma[sel] = z[sel, None] * g.uniform(0.2, 0.4, size=(sel.sum(), 3))
    sel = kind == k("sub_pixel")
    sigma[sel] = z[sel, None] / fx * 0.05 * g.uniform(0.8, 1.25, size=(sel.sum(), 3))
    log_scales = np.log(sigma).astype(np.float32)
    log_scales[kind == k("underflow")] = -40.0
    view = kernel_view()
    means = ((np.stack([x, y, z], axis=1) - view[:3, 3]) @ view[:3, :3]).astype(np.float32)
    raw_quats = (1.7 * g.normal(size=(n, 4))).astype(np.float32)
    q64 = raw_quats.astype(np.float64)
    return {"means": means, "log_scales": log_scales, "scales": np.exp(log_scales.astype(np.float64)).astype(np.float32),
            "raw_quats": raw_quats, "quats": (q64 / np.linalg.norm(q64, axis=1, keepdims=True)).astype(np.float32),
            "logits": (1.5 * g.normal(size=n)).astype(np.float32), "kind": kind}


# ---- 2., 3., 6.: the oracle's antialiased frame
def oracle_antialiased_run(scene, view, width=PC.WIDTH, height=PC.HEIGHT, inject=False):
    """The weighted RGB + depth loss of pose_cases' scene through the oracle in float64 with o_eff = sigmoid(logit) comp
    in place of the opacity, the 4x4 view matrix a differentiated leaf.
    ``inject=False``: comp is part of the autograd graph - plain autograd, the reference.
    ``inject=True``: comp enters the graph as a constant; its gradient is put back by hand the way the kernels do it:
    v_comp = v_o_eff sigmoid, G = conic_gradient(...) added to the gradient of the oracle's conics, and the oracle's own
    projection backward carries it to means, scales and quats; v_logit = v_o_eff comp sigmoid (1 - sigmoid).
    -> dict of float64 gradients (means, scales, quats, opacities, pose) and intermediates."""
    from oracle import gsplat_oracle as O
    from tinysplat_amd.synthetic import loss_weights
    fx, fy, proj = PC.intrinsics(width, height)
    w_rgb, w_d = loss_weights(width, height)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in scene.items()}
    V = torch.tensor(np.asarray(view, dtype=np.float64), requires_grad=True)
    P = torch.tensor(proj)
    tb = (-(-width // 16), -(-height // 16), 1)
    unit = t["quats"] / t["quats"].norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, nth, cov3d = O.project_gaussians(t["means"], torch.exp(t["scales"]), 1.0, unit, V[:3, :],
                                                                 P @ V, fx, fy, width / 2, height / 2, height, width, tb)
    ao, b, co, in_front = AO.prior_cov2d(t["means"], cov3d, V[:3, :], fx, fy, width, height)
    comp = torch.where(in_front, AO.compensation(ao, b, co), torch.zeros_like(ao))
    sig = torch.sigmoid(t["opacities"])[:, 0]
    if inject:
        comp_c = comp.detach()
        o_eff = (sig.detach() * comp_c).requires_grad_(True)
    else:
        o_eff = sig * comp
    dirs = t["means"].detach() - V[:3, 3].detach()
    col = torch.clamp(O.spherical_harmonics(0, dirs / dirs.norm(dim=-1, keepdim=True), t["colors_dc"][:, None, :]) + 0.5,
                      min=0.0)
    bg = torch.zeros(3, dtype=torch.float64)
    if inject:
        conics.retain_grad()
    img, _ = O.rasterize_gaussians(xys, depths, radii, conics, nth, col, o_eff, height, width, bg)
    dimg, _ = O.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3), o_eff, height, width, bg)
    loss = (torch.clamp(img, max=1.0) * w_rgb.double()).sum() + (dimg[:, :, 0] * w_d.double()).sum()
    out = {"comp": comp.detach().numpy(), "radii": radii.numpy(), "loss": float(loss.detach())}
    if not inject:
        loss.backward()
        v_logit = t["opacities"].grad.numpy()
    else:
        # first pass: the frame's own gradients with comp a constant (what ts_frame_bwd_composite leaves) ...
        (v_oeff,) = torch.autograd.grad(loss, [o_eff], retain_graph=True)
        visible = radii > 0
        v_comp = torch.where(visible, v_oeff * sig.detach(), torch.zeros_like(v_oeff))
        G, _ = AO.conic_gradient(ao.detach().numpy(), b.detach().numpy(), co.detach().numpy(), v_comp.numpy())
        G = torch.as_tensor(G) * (in_front & visible)[:, None]
        # ... then one backward pass of the projection with G added to v_conic (everything else reaches the leaves through
        # the same pass: loss.backward() with the extra conic gradient)
        torch.autograd.backward([loss, conics], [torch.ones_like(loss), G])
        s = sig.detach()
        v_logit = (torch.where(visible, v_oeff * comp_c, torch.zeros_like(v_oeff)) * s * (1.0 - s)).numpy()[:, None]
    Gv, Vn = V.grad.numpy()[:3, :], V.detach().numpy()[:3, :]
    out.update({"means": t["means"].grad.numpy(), "scales": t["scales"].grad.numpy(), "quats": t["quats"].grad.numpy(),
                "opacities": v_logit,
                "pose": np.concatenate([Gv[:, 3], sum(np.cross(Vn[:, j], Gv[:, j]) for j in range(4))]),
                "clamped_comp": int(((out["comp"] == 0) & (radii.numpy() > 0)).sum())})
    return out


@functools.lru_cache(maxsize=None)
def small_scene_runs():
    """(scene, view, autograd run, injected run) of pose_cases' 60-Gaussian 48 x 32 scene, computed once per process."""
    scene, view = PC.small_scene(), PC.view_matrix()
    return scene, view, oracle_antialiased_run(scene, view), oracle_antialiased_run(scene, view, inject=True)


# ---- 5., 6., 8.: the adapter's frame through the oracle, classic or antialiased
def oracle_render(model, cam, dims, antialiased, raster_dtype=None, depth=True):
    """helpers.oracle_frame with the mode: the reference recipe on the CPU with the oracle ops (projection and binning in
    the model's dtype, so that a float32 model gives the integers the kernels give), and for an antialiased frame
    o_eff = sigmoid(logit) comp in place of the opacity, comp restated in float64 (antialias_oracle) from the same
    parameters.  -> dict as oracle_frame's, plus ``comp`` and ``o_eff``."""
    from oracle import gsplat_oracle as O
    from tinysplat_amd.rasterizer import project_args, raster_args, sh_args
    w, h = dims
    pa = project_args(model, cam, dims, "cpu")
    xys, depths, radii, conics, nth, cov3d = O.project_gaussians(*pa)
    if xys.requires_grad:
        xys.retain_grad()
    colors = torch.clamp(O.spherical_harmonics(*sh_args(model, cam, "cpu")) + 0.5, min=0.0)
    ra = raster_args(model, xys, depths, radii, conics, nth, colors, dims)
    out = {}
    if antialiased:
        comp, _ = AO.scene_compensation(pa[0].double(), pa[1].double(), pa[3].double(), pa[4].double(), cam.f_x, cam.f_y,
                                        w, h)
        ra[6] = torch.sigmoid(model.opacities.double()) * comp[:, None]
        out.update({"comp": comp.detach(), "o_eff": ra[6].detach()})
        if raster_dtype is None:
            ra[6] = ra[6].to(model.opacities.dtype)
    rgb, _, aux = O.rasterize_gaussians(*ra, return_aux=True, compute_dtype=raster_dtype)
    out.update({"rgb": torch.clamp(rgb, max=1.0), "xys": xys, "depths": depths, "radii": radii, "conics": conics,
                "nth": nth, "aux": aux})
    if depth:
        ra_d = list(ra)
        ra_d[5] = depths[:, None].repeat(1, 3)
        d, _ = O.rasterize_gaussians(*ra_d, compute_dtype=raster_dtype)
        out["depth"] = d[:, :, 0]
    return out


# ---- 8. the point of it: small, sparse, semi-transparent Gaussians seen at a quarter of the resolution
DOWN_N, DOWN_HI, DOWN_LO, DOWN_SEED, DOWN_SCALE = 300, (128, 96), (32, 24), 7, 4.0


def downsample_scene():
    """(model, camera at 128 x 96, the same camera at 32 x 24): make_scene's Gaussians at scale_mult 4 have a projected
    sigma of 0.35 .. 1.8 px at 128 x 96 (about 1 px) and a quarter of that at 32 x 24, well under the 0.55 px the blur
    alone gives; opacity logits ~ N(0, 1.5).  The low-resolution camera is the same view with a quarter of the focal length
    in pixels (built directly: the reference's Camera.rescale multiplies the fov angles, which is another view)."""
    from tinysplat_amd.synthetic import PinholeCamera, make_scene
    model, cam_hi = make_scene(DOWN_N, 0, DOWN_HI[0], DOWN_HI[1], seed=DOWN_SEED, scale_mult=DOWN_SCALE)
    model.background = torch.zeros(3)
    cam_lo = PinholeCamera.look_at_origin_plus_z(DOWN_LO[0], DOWN_LO[1])
    cam_lo.view_matrix = cam_hi.view_matrix.clone()
    return model, cam_hi, cam_lo


def box_mean(image, k=4):
    """[H, W, C] -> [H / k, W / k, C]: the mean over k x k pixel boxes."""
    h, w, c = image.shape
    return image.reshape(h // k, k, w // k, k, c).mean(dim=(1, 3))
