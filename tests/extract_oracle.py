"""Torch restatement of the level-set half of ``extract_mesh_poisson`` (model_gaussian.py:416-459, scene.py:165-192)
for tinysplat_amd.extract: pixel pairing, back-projection, ray range, the 16-neighbour density, the first crossing,
the interpolation and (an addition) the analytic normal, in float64 (the yardstick) or float32.

``level_set_oracle`` runs end to end from a depth map and flat pixel indices.  The crossing is a chain of discrete
choices (the nearest Gaussian, sixteen neighbours per sample, the first sample above the level), and a density along
the ray changes by up to 40 per world unit on a flattened Gaussian, so an implementation is judged stage by stage:
with ``given`` (its own float32 ``p_world``, ``samples`` and optionally ``knn``) everything downstream of a given
value is evaluated in float64 on exactly that value, and the back-projection is compared on its own.  A ray is
*decision-stable* when every one of its samples has ``|d - level| > DELTA`` here."""
import numpy as np
import torch
import torch.nn.functional as F

from density_oracle import quat_to_rot

K = 16
DELTA = 1e-4
PARAMS = ("means", "scales", "quats", "opacities")


def exact_knn(points, means, k=K, block=4096):
    """Neighbours ascending in (float64 distance, index), in blocks of queries."""
    out = []
    means = means.double()
    for r0 in range(0, points.shape[0], block):
        d = torch.cdist(points[r0:r0 + block].double(), means, compute_mode="donot_use_mm_for_euclid_dist")
        out.append(torch.argsort(d, dim=1, stable=True)[:, :k])
    return torch.cat(out) if out else torch.empty((0, k), dtype=torch.long)


def sigma_inverse(scales, quats):
    """R diag(exp(-2 s)) R^T: the inverse of model_gaussian.py:247-255's R diag(exp(2 s)) R^T, exact algebra."""
    R = quat_to_rot(quats)
    return R @ (R.transpose(-2, -1) * torch.exp(-2 * scales).unsqueeze(2))


def density(points, knn, p, sinv=None):
    """density_function (:257-274) of ``points`` [M,3] over the neighbours ``knn`` [M,16] -> (d [M], unclamped sum)."""
    sinv = sigma_inverse(p["scales"], p["quats"]) if sinv is None else sinv
    mu = (points[:, None] - p["means"][knn])[:, :, None, :]
    q = (torch.matmul(mu, sinv[knn]) * mu).sum(-1).clamp(min=0, max=1e8).squeeze(-1)
    raw = torch.sum(torch.exp(-0.5 * q) * torch.sigmoid(p["opacities"][knn].squeeze(-1)), dim=-1)
    return torch.where(raw > 1, torch.ones_like(raw), raw), raw


def pixel_ndc(ids, H, W, convention, dtype, pix_off=0.0):
    ids = torch.as_tensor(ids).long()
    if convention == "reference":               # model_gaussian.py:417-419, scene.py:183-186
        x, y = (ids % H).to(dtype), (ids // H).to(dtype)
        return (x + 0.5 - W // 2) / H * 2, (y + 0.5 - H // 2) / W * 2
    col, row = (ids % W).to(dtype), (ids // W).to(dtype)
    return (col + 0.5 + pix_off - W / 2) * 2 / W, (row + 0.5 + pix_off - H / 2) * 2 / H


def backproject(ids, depth, view, proj, convention="reference", dtype=torch.float64, pix_off=0.0):
    """-> (p_world [M,3], valid [M]); an invalid pixel (depth <= 0 or a non-finite result) gets zeros."""
    depth = torch.as_tensor(depth)
    H, W = depth.shape
    V, P = torch.as_tensor(view).to(dtype), torch.as_tensor(proj).to(dtype)
    z = depth.reshape(-1)[torch.as_tensor(ids).long()].to(dtype)
    nx, ny = pixel_ndc(ids, H, W, convention, dtype, pix_off)
    ok = (z > 0) & torch.isfinite(z)
    zs = torch.where(ok, z, torch.ones_like(z))
    nz = (P[2, 2] * zs + P[2, 3]) / zs
    h = torch.stack((nx, ny, nz, torch.ones_like(nz)), -1) @ torch.linalg.inv(P @ V).T
    pw = h[:, :3] / h[:, 3:4]
    ok = ok & torch.isfinite(pw).all(-1)
    return torch.where(ok[:, None], pw, torch.zeros_like(pw)), ok


def normals(points, knn, p, sinv=None):
    """-grad d / |grad d| at ``points`` over ``knn``, the analytic gradient; zero where d was clamped or grad is 0."""
    sinv = sigma_inverse(p["scales"], p["quats"]) if sinv is None else sinv
    mu = points[:, None] - p["means"][knn]
    a = torch.einsum("mkab,mkb->mka", sinv[knn], mu)
    q = (a * mu).sum(-1)
    e = torch.exp(-0.5 * q.clamp(min=0, max=1e8)) * torch.sigmoid(p["opacities"][knn].squeeze(-1))
    passes = ((q >= 0) & (q <= 1e8)).to(points.dtype)
    # grad q = (Sigma^-1 + Sigma^-T) mu
    g = -(e * passes)[..., None] * 0.5 * (a + torch.einsum("mkba,mkb->mka", sinv[knn], mu))
    g = g.sum(1)
    length = g.norm(dim=-1, keepdim=True)
    zero = (e.sum(-1, keepdim=True) > 1) | ~(length > 0)
    return torch.where(zero, torch.zeros_like(g), -g / length.clamp_min(1e-300))


def level_set_oracle(params, depth, view, proj, position, ids, level=0.3, steps=21, extent=3.0,
                     convention="reference", dtype=torch.float64, given=None, with_normals=True, pix_off=0.0):
    """-> dict(p_world, valid, dirs, nearest, p_std, samples [M,S,3], knn [M,S,16], density [M,S], keep, first, t,
    points, normals, stable, margin).  ``t`` / ``points`` / ``normals`` are zero where ``keep`` is False."""
    p = {k: torch.as_tensor(params[k]).to(dtype) for k in PARAMS}
    ids = torch.as_tensor(ids).long()
    pw, valid = backproject(ids, depth, view, proj, convention, dtype, pix_off)
    pos = torch.as_tensor(np.asarray(position, dtype=np.float64)).to(dtype)
    if given is not None and given.get("p_world") is not None:
        pw = torch.as_tensor(given["p_world"]).to(dtype)
        valid = valid & torch.isfinite(pw).all(-1)
    pw = torch.where(valid[:, None], pw, pos.expand_as(pw))
    dirs = F.normalize(pw - pos, dim=-1) * valid[:, None].to(dtype)
    nearest = exact_knn(pw, p["means"], 1)[:, 0]
    p_std = torch.exp(p["scales"])[nearest].norm(dim=-1)
    lin = torch.linspace(-extent, extent, steps, dtype=dtype)
    t_range = lin[None, :] * p_std[:, None]
    samples = pw[:, None, :] + t_range[..., None] * dirs[:, None, :]
    if given is not None and given.get("samples") is not None:
        samples = torch.as_tensor(given["samples"]).to(dtype).reshape(samples.shape)
        samples = torch.where(valid[:, None, None], samples, pos.expand_as(samples))
    flat = samples.reshape(-1, 3)
    if given is not None and given.get("knn") is not None:
        knn = torch.as_tensor(given["knn"]).long().reshape(-1, K)
    else:
        knn = exact_knn(flat, p["means"])
    sinv = sigma_inverse(p["scales"], p["quats"])
    d = density(flat, knn, p, sinv)[0].reshape(-1, steps)
    above = d > level
    first = above.to(torch.int8).argmax(dim=-1)                  # the first True, 0 if none
    keep = valid & (d[:, 0] < level) & (first >= 1)
    fb = (first - 1).clamp(min=0)
    d_a, d_b = d.gather(1, first[:, None])[:, 0], d.gather(1, fb[:, None])[:, 0]
    t_a, t_b = t_range.gather(1, first[:, None])[:, 0], t_range.gather(1, fb[:, None])[:, 0]
    t = (level - d_b) / (d_a - d_b) * (t_a - t_b) + t_b
    t = torch.where(keep, t, torch.zeros_like(t))
    points = torch.where(keep[:, None], pw + t[:, None] * dirs, torch.zeros_like(pw))
    margin = (d - level).abs().min(dim=-1).values
    out = {"p_world": pw, "valid": valid, "dirs": dirs, "nearest": nearest, "p_std": p_std, "samples": samples,
           "knn": knn.reshape(-1, steps, K), "density": d, "keep": keep, "first": first, "t": t, "points": points,
           "margin": margin, "stable": margin > DELTA}
    if with_normals:
        nrm = torch.zeros_like(points)
        sel = torch.nonzero(keep).view(-1)
        if sel.numel():
            pts = points[sel]
            nrm[sel] = normals(pts, exact_knn(pts, p["means"]), p, sinv)
        out["normals"] = nrm
    return out


def density_at(points, params, dtype=torch.float64):
    """The clamped density of arbitrary points over their own exact 16 neighbours, differentiable in ``points``."""
    p = {k: torch.as_tensor(params[k]).to(dtype) for k in PARAMS}
    knn = exact_knn(points.detach(), p["means"])
    return density(points, knn, p)
