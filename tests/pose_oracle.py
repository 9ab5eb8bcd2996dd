"""numpy float64 restatement of the pose gradient's six sums, of SE(3)'s Exp and Log and of the retraction update
(DESIGN.md section 6u).  Written from the definitions, independently of tinysplat_amd/pose.py and csrc/pose_math.h."""
import math

import numpy as np


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def row_terms(view, means, quats, v_means, v_quats):
    """float64 [n, 6]: per row (R g, p x R g + R tau) for the view matrix ``view`` ([3, 4] or [4, 4])."""
    view = np.asarray(view, dtype=np.float64)
    R, t = view[:3, :3], view[:3, 3]
    m, q = np.asarray(means, dtype=np.float64), np.asarray(quats, dtype=np.float64)
    g, h = np.asarray(v_means, dtype=np.float64), np.asarray(v_quats, dtype=np.float64)
    p = m @ R.T + t
    gc = g @ R.T
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ex = np.stack([-x, w, -z, y], axis=1)            # e_x (x) q, Hamilton product
    ey = np.stack([-y, z, w, -x], axis=1)
    ez = np.stack([-z, -y, x, w], axis=1)
    tau = 0.5 * np.stack([(h * ex).sum(1), (h * ey).sum(1), (h * ez).sum(1)], axis=1)
    return np.concatenate([gc, np.cross(p, gc) + tau @ R.T], axis=1)


def pose_gradient(view, means, quats, v_means, v_quats):
    """(dL/dv, dL/domega) float64 [6], summed with math.fsum (exact sum of the float64 terms, rounded once)."""
    terms = row_terms(view, means, quats, v_means, v_quats)
    return np.array([math.fsum(terms[:, k]) for k in range(6)])


def magnitude(view, means, quats, v_means, v_quats):
    """float64 [6]: per component the sum of the absolute values of every product that enters it - what the rounding
    bound of a sum of products is proportional to."""
    view = np.abs(np.asarray(view, dtype=np.float64))
    R, t = view[:3, :3], view[:3, 3]
    m, q = np.abs(np.asarray(means, dtype=np.float64)), np.abs(np.asarray(quats, dtype=np.float64))
    g, h = np.abs(np.asarray(v_means, dtype=np.float64)), np.abs(np.asarray(v_quats, dtype=np.float64))
    p = m @ R.T + t
    gc = g @ R.T
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tau = 0.5 * np.stack([(h * np.stack([x, w, z, y], 1)).sum(1), (h * np.stack([y, z, w, x], 1)).sum(1),
                          (h * np.stack([z, y, x, w], 1)).sum(1)], axis=1)
    cross = np.stack([p[:, 1] * gc[:, 2] + p[:, 2] * gc[:, 1], p[:, 2] * gc[:, 0] + p[:, 0] * gc[:, 2],
                      p[:, 0] * gc[:, 1] + p[:, 1] * gc[:, 0]], axis=1)
    return np.concatenate([gc, cross + tau @ R.T], axis=1).sum(axis=0)


def series_expm(a, terms=30):
    """exp of a square matrix by its Taylor series (for |a| of a few units)."""
    out, term = np.eye(a.shape[0]), np.eye(a.shape[0])
    for k in range(1, terms):
        term = term @ a / k
        out = out + term
    return out


def twist(delta):
    """The 4x4 generator of delta = (v, omega): Exp(delta) = expm(twist(delta))."""
    delta = np.asarray(delta, dtype=np.float64)
    out = np.zeros((4, 4))
    out[:3, :3] = hat(delta[3:])
    out[:3, 3] = delta[:3]
    return out


def se3_exp(delta):
    """expm of the twist, by scaling and squaring of the series (independent of the closed form)."""
    a = twist(delta) / 64.0
    out = series_expm(a)
    for _ in range(6):
        out = out @ out
    return out


def adam_retraction(T, m, v, step, grad, lr6, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0, log=None):
    """One update of a 4x4 correction T: -> (T', m', v').  ``log``: a function T -> delta for the decay term."""
    g = np.asarray(grad, dtype=np.float64)
    if weight_decay:
        g = g + weight_decay * log(T)
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    d = -np.asarray(lr6) * (m / (1 - betas[0] ** step)) / (np.sqrt(v / (1 - betas[1] ** step)) + eps)
    return se3_exp(d) @ T, m, v


def pose_error(T_true, T_found):
    """(angle, translation norm) of T_true^-1 T_found."""
    d = np.linalg.inv(T_true) @ T_found
    c = min(1.0, max(-1.0, 0.5 * (np.trace(d[:3, :3]) - 1.0)))
    s = 0.5 * np.linalg.norm([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
    return float(math.atan2(s, c)), float(np.linalg.norm(d[:3, 3]))
