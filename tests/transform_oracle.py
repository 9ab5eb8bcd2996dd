"""Float64 restatement of the scene transform with code of its own: quaternion -> matrix, Hamilton
product, the SH rotation matrices D_l by a least-squares fit over 200 seeded random directions against the oracle's
``sh_basis`` (not the module's fixed directions and not its basis), and the camera move as a product of 4x4 matrices.

``transform`` takes the float32-rounded arrays the kernel receives (M, t, r, log s, D_l), so what it is compared with is the
kernel's arithmetic alone; it also returns the sums of absolute products the error bounds are stated in."""
import numpy as np
import torch

from oracle import gsplat_oracle as O

U = 2.0 ** -24            # unit roundoff of float32


def quat_to_matrix(q):
    w, x, y, z = (float(v) for v in np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64)))
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def hamilton_terms(r, q):
    """The four products of every component of r (x) q, signed: [..., 4 components, 4 products]."""
    r = np.asarray(r, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([np.stack([r[0] * w, -r[1] * x, -r[2] * y, -r[3] * z], -1),
                     np.stack([r[0] * x, r[1] * w, r[2] * z, -r[3] * y], -1),
                     np.stack([r[0] * y, -r[1] * z, r[2] * w, r[3] * x], -1),
                     np.stack([r[0] * z, r[1] * y, -r[2] * x, r[3] * w], -1)], -2)


def basis(degree, dirs):
    """oracle.gsplat_oracle.sh_basis in float64 on unit directions [M,3] -> [M, (degree+1)^2]."""
    return O.sh_basis(degree, torch.as_tensor(np.asarray(dirs, dtype=np.float64))).numpy()


def random_directions(count, seed):
    d = np.random.default_rng(seed).normal(size=(count, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sh_rotation(rotation, degree, seed=77):
    """[D_1 .. D_degree]: the least-squares solution of Y_l(d) D_l = Y_l(R^T d) over 200 random directions."""
    rot = np.asarray(rotation, dtype=np.float64)
    d = random_directions(200, seed)
    b, a = basis(degree, d), basis(degree, d @ rot)            # rows of d @ R are (R^T d)^T
    out = []
    for l in range(1, degree + 1):
        cols = slice(l * l, (l + 1) * (l + 1))
        out.append(np.linalg.lstsq(b[:, cols], a[:, cols], rcond=None)[0])
    return out


def camera_view(view, scale, rotation, translation):
    """V' with V' x' = s V x for x' = s R x + t: diag(s, s, s, 1) V T^-1 as 4x4 products."""
    t4 = np.eye(4)
    t4[:3, :3] = scale * np.asarray(rotation, dtype=np.float64)
    t4[:3, 3] = translation
    return np.diag([scale, scale, scale, 1.0]) @ np.asarray(view, dtype=np.float64) @ np.linalg.inv(t4)


def transform(xform, quat, log_scale, sh_mats, means, scales, quats, rest):
    """float64 results of the kernel's formulas on the arrays it receives -> dict with ``means``, ``scales``, ``quats``,
    ``rest`` and, under ``*_mag``, the sums of the absolute values of the terms of every output (the error bounds'
    right-hand sides).  ``sh_mats``: one (2l+1)^2 matrix per stored band."""
    with np.errstate(all="ignore"):
        m = np.asarray(xform, dtype=np.float64)[:9].reshape(3, 3)
        t = np.asarray(xform, dtype=np.float64)[9:]
        p = np.asarray(means, dtype=np.float64)
        terms = m[None, :, :] * p[:, None, :]                                      # [n, i, k]
        out = {"means": terms.sum(-1) + t, "means_mag": np.abs(terms).sum(-1) + np.abs(t)}
        out["scales"] = np.asarray(scales, dtype=np.float64) + float(log_scale)
        ht = hamilton_terms(quat, quats)
        out["quats"], out["quats_mag"] = ht.sum(-1), np.abs(ht).sum(-1)
        c = np.asarray(rest, dtype=np.float64)                                     # [n, k_rest, 3]
        ref, mag = np.zeros_like(c), np.zeros_like(c)
        for l, d in enumerate(sh_mats, start=1):
            d = np.asarray(d, dtype=np.float64)
            rows = slice(l * l - 1, (l + 1) * (l + 1) - 1)
            prod = d[None, :, :, None] * c[:, None, rows, :]                       # [n, j, k, channel]
            ref[:, rows, :], mag[:, rows, :] = prod.sum(2), np.abs(prod).sum(2)
        out["rest"], out["rest_mag"] = ref, mag
    return out

