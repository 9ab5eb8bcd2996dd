"""Float64 yardstick of the field colours (tinysplat_amd.mesh ``colors=True`` / ``vertex_colors``, csrc/field_color.hip;
DESIGN.md section 6h), plain torch; ``dtype=torch.float32`` gives the restatement whose deviation from the float64 run
is the bar's ``E_c``, as ``mesh_oracle.corner_densities`` does for the densities.

    w_j = sigmoid(o_j) exp(-clamp(q_j, 0, 1e8) / 2),  q_j = (x - mu_j)^T Sigma_j^-1 (x - mu_j)   (a NaN q counts as 1e8)
    c_j = max(sum_k Y_k(-n) coeffs[j, k, :] + 0.5, 0),  coeffs = cat(colors_dc[:, None], colors_rest, 1), bands <= degree
    colour(x) = min(sum_j w_j c_j / sum_j w_j, 1); c of the first listed neighbour where sum_j w_j is not positive and finite

The weights come from the raw parameters through ``extract_oracle.sigma_inverse``, not from packed records.  The SH
basis is written here from the closed forms of the real harmonics (normalisation constants computed, not copied) and is
held against ``oracle/gsplat_oracle.py``'s ``spherical_harmonics`` by tests/test_color_cpu.py."""
import math

import torch

import extract_oracle as EO

K = EO.K


def sh_basis(degree, d):
    """Real spherical harmonics of unit directions ``d`` [M,3] in the 3DGS order and signs -> [M, (degree + 1)^2]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    pi = math.pi
    cols = [torch.full_like(x, 0.5 * math.sqrt(1.0 / pi))]
    if degree >= 1:
        a = math.sqrt(3.0 / (4.0 * pi))
        cols += [-a * y, a * z, -a * x]
    if degree >= 2:
        a, b = 0.5 * math.sqrt(15.0 / pi), 0.25 * math.sqrt(5.0 / pi)
        cols += [a * (x * y), -a * (y * z), b * (2.0 * z * z - x * x - y * y), -a * (x * z), 0.5 * a * (x * x - y * y)]
    if degree >= 3:
        a, b = 0.25 * math.sqrt(35.0 / (2.0 * pi)), 0.25 * math.sqrt(21.0 / (2.0 * pi))
        e, f = 0.5 * math.sqrt(105.0 / pi), 0.25 * math.sqrt(7.0 / pi)
        xx, yy, zz = x * x, y * y, z * z
        cols += [-a * y * (3.0 * xx - yy), e * (x * y) * z, -b * y * (4.0 * zz - xx - yy),
                 f * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), -b * x * (4.0 * zz - xx - yy), 0.5 * e * z * (xx - yy),
                 -a * x * (xx - 3.0 * yy)]
    if degree >= 4:
        raise ValueError("bands 0..3")
    return torch.stack(cols, -1)


def weights(points, knn, p):
    """[M,16]: every listed neighbour's term of ``extract_oracle.density``; 0 for an index outside [0, N)."""
    n = p["means"].shape[0]
    inside = (knn >= 0) & (knn < n)
    j = knn.clamp(0, n - 1)
    sinv = EO.sigma_inverse(p["scales"], p["quats"])
    mu = points[:, None, :] - p["means"][j]
    q = (torch.einsum("mkab,mkb->mka", sinv[j], mu) * mu).sum(-1)
    q = torch.where(torch.isnan(q), torch.full_like(q, 1e8), q.clamp(min=0, max=1e8))
    w = torch.sigmoid(p["opacities"][j].squeeze(-1)) * torch.exp(-0.5 * q)
    return torch.where(inside, w, torch.zeros_like(w)), inside


def colors(params, colors_dc, colors_rest, points, normals, knn, degree, dtype=torch.float64, parts=False):
    """The colours [M,3] of ``points`` [M,3] with ``normals`` [M,3] (or None) over the listed neighbours ``knn`` [M,16],
    every input converted to ``dtype`` first.  ``parts``: also ``(w [M,16], c [M,16,3], fell_back [M])``."""
    p = {k: torch.as_tensor(params[k]).to(dtype) for k in EO.PARAMS}
    dc, rest = torch.as_tensor(colors_dc).to(dtype), torch.as_tensor(colors_rest).to(dtype)
    pts, knn = torch.as_tensor(points).to(dtype), torch.as_tensor(knn).long()
    m, nb = pts.shape[0], (degree + 1) ** 2
    if not 0 <= degree <= 3 or nb > rest.shape[1] + 1:
        raise ValueError("the degree exceeds the bands stored")
    if normals is None:
        usable = torch.zeros((m,), dtype=torch.bool)
        d = torch.zeros((m, 3), dtype=dtype)
    else:
        nrm = torch.as_tensor(normals).to(dtype)
        length = (nrm * nrm).sum(-1).sqrt()
        usable = torch.isfinite(length) & (length > 0)
        d = -nrm / torch.where(usable, length, torch.ones_like(length))[:, None]
    d = torch.where(usable[:, None], d, torch.tensor([0.0, 0.0, 1.0], dtype=dtype).expand(m, 3))
    Y = sh_basis(degree, d)
    Y = torch.cat((Y[:, :1], Y[:, 1:] * usable[:, None].to(dtype)), 1)       # band 0 alone without a usable normal
    w, inside = weights(pts, knn, p)
    coeffs = torch.cat((dc[:, None, :], rest[:, :nb - 1, :]), 1)[knn.clamp(0, dc.shape[0] - 1)]     # [M,16,nb,3]
    c = Y[:, None, 0, None] * coeffs[:, :, 0, :]
    for k in range(1, nb):                                                   # ascending bands, one rounding per step
        c = c + Y[:, None, k, None] * coeffs[:, :, k, :]
    c = (c + 0.5).clamp(min=0) * inside[..., None].to(dtype)
    sw = w.sum(-1)
    weighed = torch.isfinite(sw) & (sw > 0)
    mean = (w[..., None] * c).sum(1) / torch.where(weighed, sw, torch.ones_like(sw))[:, None]
    out = torch.where(weighed[:, None], mean, c[:, 0, :]).clamp(max=1)
    return (out, w, c, ~weighed) if parts else out


def exact_knn(points, params):
    return EO.exact_knn(torch.as_tensor(points), torch.as_tensor(params["means"]))


def coefficients(n, k_rest, seed, rest_std=0.3):
    """Seeded ``colors_dc ~ N(0, 1)`` [n,3] and ``colors_rest ~ N(0, rest_std)`` [n, k_rest, 3], float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), rest_std * torch.randn(n, k_rest, 3, generator=g)
