"""A numpy restatement of the depth prior (tinysplat/depth.py:73-145): the projection and pixel
rounding, the last-wins de-duplication in row-major order, the sampling of a dense map, the objective, and the exact
optimum of the fit.  ``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` rounds every product, sum and quotient
on its own, which is what the reference's float32 numpy lines and the kernels do.  No scipy below m = 300."""
from fractions import Fraction

import numpy as np

BRUTE_FORCE_MAX = 300


def project(view, f_x, f_y, width, height, xyz, errors, dtype=np.float64):
    """depth.py:80-99 -> (px, py, z, keep): pixel coordinates as floats of ``dtype`` (rounded half to even), the
    camera-space depth, and which points are kept: inside the image, z finite and > 0, error finite and > 0."""
    t = dtype
    view, xyz = np.asarray(view, dtype=t), np.asarray(xyz).astype(t)
    cam = []
    for r in range(3):
        acc = (view[r, 0] * xyz[:, 0]).astype(t)
        acc = (acc + (view[r, 1] * xyz[:, 1]).astype(t)).astype(t)
        acc = (acc + (view[r, 2] * xyz[:, 2]).astype(t)).astype(t)
        cam.append((acc + view[r, 3]).astype(t))
    z = cam[2]
    with np.errstate(all="ignore"):
        x, y = (cam[0] / z).astype(t), (cam[1] / z).astype(t)
        px = np.round(((x * t(f_x)).astype(t) + t(width / 2)).astype(t))
        py = np.round(((y * t(f_y)).astype(t) + t(height / 2)).astype(t))
        errors = np.asarray(errors, dtype=np.float64)
        keep = (px >= 0) & (px < width) & (py >= 0) & (py < height) & np.isfinite(z) & (z > 0) & np.isfinite(errors) & \
            (errors > 0)
    return px, py, z, keep


def boundary_distance(view, f_x, f_y, width, height, xyz):
    """the smallest distance, in pixels and float64, of a projected coordinate from a rounding boundary (k + 0.5) and of
    a point from the image's border - over the points in front of the camera"""
    view, xyz = np.asarray(view, dtype=np.float64), np.asarray(xyz, dtype=np.float64)
    cam = xyz @ view[:3, :3].T + view[:3, 3]
    front = cam[:, 2] > 0
    u = cam[front, 0] / cam[front, 2] * f_x + width / 2
    v = cam[front, 1] / cam[front, 2] * f_y + height / 2
    frac = np.concatenate([u, v]) - 0.5
    return float(np.min(np.abs(frac - np.round(frac)))) if frac.size else np.inf


def sparse(view, f_x, f_y, width, height, xyz, errors, dtype=np.float64):
    """``_estimate_sparse``: -> (row, col, z, e) of the surviving points, row-major, the point latest in the list winning
    a pixel (what ``lil_matrix`` assignment and ``tocoo()`` leave); z in ``dtype``, e float64."""
    px, py, z, keep = project(view, f_x, f_y, width, height, xyz, errors, dtype)
    errors = np.asarray(errors, dtype=np.float64)
    last = {}
    for i in np.flatnonzero(keep):
        last[int(py[i]) * width + int(px[i])] = i
    pixels = np.array(sorted(last), dtype=np.int64)
    idx = np.array([last[p] for p in pixels], dtype=np.int64)
    return pixels // width, pixels % width, z[idx], errors[idx]


def sample_dense(dense, height, width, u, v, dtype=np.float64):
    """the map [h, w] at the pixels (u, v) of a height x width camera: the stored value at equal sizes, else bilinear with
    pixel centres aligned (align_corners=False) and edge clamp"""
    dense = np.asarray(dense)
    h, w = dense.shape
    u, v = np.asarray(u), np.asarray(v)
    if (h, w) == (height, width):
        return dense[v, u]
    t = dtype
    d = dense.astype(t)
    fx = ((u.astype(t) + t(0.5)) * (t(w) / t(width)).astype(t)).astype(t) - t(0.5)
    fy = ((v.astype(t) + t(0.5)) * (t(h) / t(height)).astype(t)).astype(t) - t(0.5)
    fx, fy = np.clip(fx, t(0), t(w - 1)).astype(t), np.clip(fy, t(0), t(h - 1)).astype(t)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    a, b = (fx - x0.astype(t)).astype(t), (fy - y0.astype(t)).astype(t)
    top = (((t(1) - a) * d[y0, x0]).astype(t) + (a * d[y0, x1]).astype(t)).astype(t)
    bottom = (((t(1) - a) * d[y1, x0]).astype(t) + (a * d[y1, x1]).astype(t)).astype(t)
    return (((t(1) - b) * top).astype(t) + (b * bottom).astype(t)).astype(t)


def objective(s, t, x, y, w):
    """f(s, t) = (1/m) sum w_i |y_i - s x_i - t| in float64: the reference's ``func``"""
    x, y, w = (np.asarray(a, dtype=np.float64) for a in (x, y, w))
    return float(np.mean(w * np.abs(y - (s * x + t))))


def objective_exact(s, t, x, y, w):
    """f(s, t) in rational arithmetic, rounded once: no cancellation error in the residuals"""
    s, t = Fraction(float(s)), Fraction(float(t))
    total = Fraction(0)
    for xi, yi, wi in zip(x, y, w):
        total += Fraction(float(wi)) * abs(Fraction(float(yi)) - s * Fraction(float(xi)) - t)
    return float(total / len(x))


def weighted_median_lower(r, w):
    """the smallest value v with sum_{r_i <= v} w_i >= half the total weight"""
    r, w = np.asarray(r, dtype=np.float64), np.asarray(w, dtype=np.float64)
    order = np.argsort(r, kind="stable")
    below = np.cumsum(w[order])
    return float(r[order][np.searchsorted(below, 0.5 * below[-1], side="left")])


def _through_pairs(x, y, w):
    """the best line through two data points (the LP's optimum is one) by brute force"""
    m = len(x)
    i, j = np.triu_indices(m, 1)
    ok = x[i] != x[j]
    i, j = i[ok], j[ok]
    best = (np.inf, 1.0, 0.0)
    for a in range(0, len(i), 4096):
        ii, jj = i[a:a + 4096], j[a:a + 4096]
        s = (y[jj] - y[ii]) / (x[jj] - x[ii])
        t = y[ii] - s * x[ii]
        f = np.mean(w[None, :] * np.abs(y[None, :] - (s[:, None] * x[None, :] + t[:, None])), axis=1)
        k = int(np.argmin(f))
        if f[k] < best[0]:
            best = (float(f[k]), float(s[k]), float(t[k]))
    return best


def optimum(x, y, w):
    """-> (f*, s, t): the minimiser by ``_optimum`` and the objective at it in rational arithmetic, rounded once."""
    _, s, t = _optimum(x, y, w)
    return objective_exact(s, t, x, y, w), s, t


def _optimum(x, y, w):
    """-> (f*, s, t): the exact minimum of the objective.  All x equal: s = 1, t = the weighted median of y - x (any s
    does as well).  m <= 300: every line through two data points.  Larger: scipy's HiGHS on the LP, its vertex snapped to
    the two data points it passes through and re-evaluated here, so that the value is one the objective really takes."""
    x, y, w = (np.asarray(a, dtype=np.float64) for a in (x, y, w))
    m = len(x)
    assert m >= 1
    if np.all(x == x[0]):
        t = weighted_median_lower(y - x, w)
        return objective(1.0, t, x, y, w), 1.0, t
    if m <= BRUTE_FORCE_MAX:
        return _through_pairs(x, y, w)
    from scipy.optimize import linprog
    cost = np.concatenate([[0.0, 0.0], w / m])
    from scipy.sparse import bmat, csr_matrix, identity
    line = csr_matrix(np.stack([x, np.ones(m)], axis=1))
    upper = bmat([[-line, -identity(m)],                                         # y - s x - t <= e
                  [line, -identity(m)]], format="csr")                           # -(y - s x - t) <= e
    res = linprog(cost, A_ub=upper, b_ub=np.concatenate([-y, y]), bounds=[(None, None)] * 2 + [(0, None)] * m,
                  method="highs")
    assert res.status == 0, res.message
    s, t = float(res.x[0]), float(res.x[1])
    candidates = [(objective(s, t, x, y, w), s, t)]
    near = np.argsort(np.abs(y - (s * x + t)))[:6]                               # the vertex's two points are among them
    for a in range(len(near)):
        for b in range(a + 1, len(near)):
            i, j = near[a], near[b]
            if x[i] != x[j]:
                sl = (y[j] - y[i]) / (x[j] - x[i])
                tl = y[i] - sl * x[i]
                candidates.append((objective(sl, tl, x, y, w), float(sl), float(tl)))
    return min(candidates)


def apply(s, t, dense, disparity=False):
    """train.py:66: float64 scalars times the map, one rounding to float32"""
    v = np.float64(s) * np.asarray(dense).astype(np.float64) + np.float64(t)
    return (1.0 / v if disparity else v).astype(np.float32)
