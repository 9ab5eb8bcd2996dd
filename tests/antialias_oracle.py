"""float64 restatement of the antialiased mode: the projected covariance before the projection's
0.3 blur, the compensation factor with a square root whose derivative at the clamp is 0, and the oracle's frame with the
compensated opacity in place of the opacity.  Projection and compositing are oracle/gsplat_oracle.py's; written from the
definitions, independently of csrc/antialias_math.h."""
import numpy as np
import torch

from oracle import gsplat_oracle as O


class _ClampedSqrt(torch.autograd.Function):
    """sqrt(max(0, x)) whose derivative is exactly 0 where the max clamps (x <= 0), not inf or NaN."""

    @staticmethod
    def forward(ctx, x):
        live = x > 0
        y = torch.where(live, torch.sqrt(torch.where(live, x, torch.ones_like(x))), torch.zeros_like(x))
        ctx.save_for_backward(y, live)
        return y

    @staticmethod
    def backward(ctx, g):
        y, live = ctx.saved_tensors
        return torch.where(live, g / (2.0 * torch.where(live, y, torch.ones_like(y))), torch.zeros_like(g))


def compensation(ao, b, co, blur=O.COV2D_BLUR):
    """comp = sqrt(max(0, det_o / det_b)) of float64 tensors; 0 (with a zero derivative) where det_o <= 0 or det_b is not
    positive."""
    det_o = ao * co - b * b
    det_b = (ao + blur) * (co + blur) - b * b
    live = (det_o > 0) & (det_b > 0)
    ratio = torch.where(live, det_o / torch.where(live, det_b, torch.ones_like(det_b)), torch.zeros_like(det_o))
    return _ClampedSqrt.apply(ratio)


def conic_gradient(ao, b, co, v_comp, blur=O.COV2D_BLUR):
    """float64 [n, 3]: v_comp times the true partials of comp with respect to the three stored entries (X00, X01, X11) of
    the conic X = Sigma_b^-1, from autograd's d comp / d(a_o, b, c_o) and the chain rule of the matrix inverse:
    with V the symmetric gradient matrix of comp with respect to the covariance (V01 = half the partial of b, which stands
    for two entries), G = -Sigma_b V Sigma_b, and the stored off-diagonal entry stands for two as well: 2 G01."""
    leaves = [torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True) for t in (ao, b, co)]
    comp = compensation(*leaves, blur=blur)
    da, db, dc = torch.autograd.grad(comp.sum(), leaves)
    a_, b_, c_ = (t.detach() for t in leaves)
    ab, cb = a_ + blur, c_ + blur
    V00, V01, V11 = da, 0.5 * db, dc
    # Y = Sigma_b V, G = -Y Sigma_b
    Y00, Y01 = ab * V00 + b_ * V01, ab * V01 + b_ * V11
    Y10, Y11 = b_ * V00 + cb * V01, b_ * V01 + cb * V11
    G00 = -(Y00 * ab + Y01 * b_)
    G01 = -(Y00 * b_ + Y01 * cb)
    G11 = -(Y10 * b_ + Y11 * cb)
    v = torch.as_tensor(np.asarray(v_comp, dtype=np.float64))
    return torch.stack([v * G00, v * 2.0 * G01, v * G11], dim=-1).numpy(), comp.detach().numpy()


def prior_cov2d(means3d, cov3d, viewmat, fx, fy, img_width, img_height, clip_thresh=O.CLIP_THRESH):
    """(a_o, b, c_o, in_front): the EWA covariance T cov3d T^T of oracle.project_gaussians WITHOUT the blur, from the
    oracle's own (differentiable) cov3d output; T = J W with the 1.3 fov clamp, as the oracle builds it."""
    V = viewmat.to(means3d.dtype)
    mx, my, mz = means3d[:, 0], means3d[:, 1], means3d[:, 2]
    px = V[0, 0] * mx + V[0, 1] * my + V[0, 2] * mz + V[0, 3]
    py = V[1, 0] * mx + V[1, 1] * my + V[1, 2] * mz + V[1, 3]
    pz = V[2, 0] * mx + V[2, 1] * my + V[2, 2] * mz + V[2, 3]
    in_front = pz > clip_thresh
    pz_s = torch.where(in_front, pz, torch.ones_like(pz))
    limx, limy = 1.3 * (0.5 * img_width / fx), 1.3 * (0.5 * img_height / fy)
    tx = pz_s * torch.clamp(px / pz_s, -limx, limx)
    ty = pz_s * torch.clamp(py / pz_s, -limy, limy)
    J = torch.zeros((means3d.shape[0], 2, 3), dtype=means3d.dtype)
    J[:, 0, 0], J[:, 0, 2] = fx / pz_s, -fx * tx / (pz_s * pz_s)
    J[:, 1, 1], J[:, 1, 2] = fy / pz_s, -fy * ty / (pz_s * pz_s)
    T = J @ V[:3, :3]
    c = cov3d
    C = torch.stack([torch.stack([c[:, 0], c[:, 1], c[:, 2]], -1), torch.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                     torch.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], dim=-2)
    S = T @ C @ T.transpose(1, 2)
    return S[:, 0, 0], S[:, 0, 1], S[:, 1, 1], in_front


def scene_compensation(means3d, scales, quats, viewmat, fx, fy, img_width, img_height):
    """comp [n] of prepared inputs (scales and unit quaternions as oracle.project_gaussians takes them); a Gaussian behind
    the clip plane has comp = 0.  Differentiable."""
    tb = (-(-img_width // 16), -(-img_height // 16), 1)
    out = O.project_gaussians(means3d, scales, 1.0, quats, viewmat, torch.eye(4, dtype=means3d.dtype), fx, fy,
                              img_width / 2, img_height / 2, img_height, img_width, tb)
    # cov3d is zeroed behind the clip plane by the oracle, which makes det_o = 0 there: the clamp
    ao, b, co, in_front = prior_cov2d(means3d, out[5], viewmat, fx, fy, img_width, img_height)
    comp = compensation(ao, b, co)
    return torch.where(in_front, comp, torch.zeros_like(comp)), (ao, b, co)
