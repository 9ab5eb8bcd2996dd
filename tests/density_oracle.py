"""Torch restatement of the SuGaR density regulariser (scripts/train.py:77-91, model_gaussian.py:244-326) for
tinysplat_amd.surface: sample_points' transform, density_function, approximate_density_function and the loss,
op for op, in float32 (the reference's own evaluation) or float64 (the GPU's yardstick).  ``projection="screen"``
is defined here: the same code with ``grid = (proj @ pc)[:2] / (proj @ pc)[3]`` and the mask ``z > znear``,
``-1 <= ndc < 1``.  The points carry the reference's retained graph: they are rebuilt from the parameters as they
were at sampling time (``sample``), and that part of the gradient is added to the current parameters' own."""
import torch
import torch.nn.functional as F

K = 16
ZNEAR = 0.001


def quat_to_rot(quat):
    """utils.py:42-64"""
    w, x, y, z = torch.unbind(F.normalize(quat, dim=-1), dim=-1)
    return torch.stack([
        torch.stack([1 - 2 * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=-1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x ** 2 + z ** 2), 2 * (y * z - w * x)], dim=-1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x ** 2 + y ** 2)], dim=-1),
    ], dim=-2)


def sample_transform(means, scales, quats, rows, normals):
    """model_gaussian.py:322-325 for given rows and normals."""
    rows = torch.as_tensor(rows).long()
    xi = normals * torch.exp(scales)[rows]
    xi = torch.bmm(quat_to_rot(quats[rows]), xi[..., None]).squeeze(-1)
    return means[rows] + xi


def exact_knn(points, means, k=K):
    """Neighbours ascending in (float64 distance, index)."""
    d = torch.cdist(points.double(), means.double(), compute_mode="donot_use_mm_for_euclid_dist")
    return torch.argsort(d, dim=1, stable=True)[:, :k]


def inverse_cdf(scales, uniforms, weights="reference"):
    """float64 inverse CDF of the row draw: weights C_i (the reference's cumulative sums) or a_i."""
    a = torch.prod(torch.exp(torch.as_tensor(scales, dtype=torch.float32)), -1).abs().double()
    w = a.cumsum(0) if weights == "reference" else a
    c = w.cumsum(0)
    t = torch.as_tensor(uniforms).double() * c[-1]
    return torch.searchsorted(c, t, right=True).clamp(max=a.shape[0] - 1)


def density_oracle(params, depth, view, proj, rows, normals, knn, projection="reference", dtype=torch.float64,
                   sample_params=None, points=None):
    """-> dict(loss, density, beta, approx, mask, grads={means, scales, quats, opacities, depth}, points).
    ``params``: {means, scales, quats, opacities} now; ``sample_params``: {means, scales, quats} at sampling time
    (default: the same values).  ``points``: the stored (float32) sample points, used for the value while the
    gradient still flows through the sampling expression.  ``approx`` is evaluated for every point (the loss reads
    it under ``mask``)."""
    cur = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    sp = sample_params if sample_params is not None else params
    smp = {k: torch.as_tensor(sp[k]).to(dtype).clone().requires_grad_(True) for k in ("means", "scales", "quats")}
    dep = torch.as_tensor(depth).to(dtype).clone().requires_grad_(True)
    V, P = torch.as_tensor(view).to(dtype), torch.as_tensor(proj).to(dtype)
    knn = torch.as_tensor(knn).long()
    points_expr = sample_transform(smp["means"], smp["scales"], smp["quats"], rows, torch.as_tensor(normals).to(dtype))
    points = points_expr if points is None else \
        torch.as_tensor(points).to(dtype) + (points_expr - points_expr.detach())
    # density_function (:257-274)
    R = quat_to_rot(cur["quats"])
    S2 = torch.exp(cur["scales"]).pow(2).unsqueeze(2)
    sigma_inv = (R @ (R.transpose(-2, -1) * S2)).inverse()
    mu = (points[:, None] - cur["means"][knn])[:, :, None, :]
    q = (torch.matmul(mu, sigma_inv[knn]) * mu).sum(-1).clamp(min=0, max=1e8)
    d = torch.exp(-0.5 * q).squeeze(-1)
    d = torch.sum(d * torch.sigmoid(cur["opacities"][knn].squeeze(-1)), dim=-1)
    d = torch.where(d > 1, torch.ones_like(d), d)          # 1 + 1e-12 is 1.0 in float32
    beta = torch.exp(cur["scales"]).min(dim=-1)[0][knn].mean(dim=1)
    # approximate_density_function (:276-316)
    H, W = dep.shape
    pc = torch.cat((points, torch.ones(points.shape[0], 1, dtype=dtype)), dim=1) @ V.t()
    z = pc[:, 2]
    mask = z > ZNEAR
    h = pc @ P.t()
    if projection == "reference":
        x, y = -W * h[:, 0], -H * h[:, 1]
        mask = mask & (-W < x) & (x <= 0) & (-H < y) & (y <= 0)
    else:
        x, y = h[:, 0] / h[:, 3], h[:, 1] / h[:, 3]
        mask = mask & (-1 <= x) & (x < 1) & (-1 <= y) & (y < 1)
    grid = torch.stack((x, y), -1)[None, :, None, :]
    z_map = F.grid_sample(dep[None, None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0, :, 0]
    approx = torch.exp(-0.5 * (z_map - z).pow(2) / beta.pow(2))
    loss = (d[mask] - approx[mask]).abs().mean()
    if bool(mask.any()):
        loss.backward()
    grads = {}
    for k in ("means", "scales", "quats", "opacities"):
        g = cur[k].grad if cur[k].grad is not None else torch.zeros_like(cur[k])
        if k in smp and smp[k].grad is not None:
            g = g + smp[k].grad
        grads[k] = g.detach()
    grads["depth"] = dep.grad.detach() if dep.grad is not None else torch.zeros_like(dep)
    return {"loss": loss.detach(), "density": d.detach(), "beta": beta.detach(), "approx": approx.detach(),
            "mask": mask, "grads": grads, "points": points.detach()}
