"""Adversarial 2-D inputs for the two alpha culls (ts::rect_may_contribute per 8x8 block, ts::TightTest per 16x16 tile)
and their reference: alpha evaluated in float64 at every integer sample position of a region, as
oracle/gsplat_oracle.py::rasterize_gaussians defines it (d = centre - sample, sigma = 0.5 (a dx^2 + c dy^2) + b dx dy,
alpha = opacity exp(-sigma)).  A region is NEEDED when its largest alpha is >= 1/255.

Used by tests/test_hostmath_cull.py (the header compiled for the host); the generators take no GPU and are meant to
feed a kernel-level check through the C ABI as well.
Every generator is seeded and returns float32 arrays: what a test hands to the code under test is exactly what the
reference casts to float64."""
import math

import numpy as np

ALPHA_MIN = 1.0 / 255.0
TILE = 16


# ---------------------------------------------------------------------------------------------------------------------
# Gaussians: (s1, s2, theta) = standard deviations along / across the axis at angle theta; cov = R diag(s1^2, s2^2) R^T
# ---------------------------------------------------------------------------------------------------------------------
def conic_of(s1, s2, theta):
    """-> (a, b, c) float64: the inverse of the covariance."""
    ct, st = np.cos(theta), np.sin(theta)
    i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    return ct * ct * i1 + st * st * i2, ct * st * (i1 - i2), st * st * i1 + ct * ct * i2


def cov_of(s1, s2, theta):
    ct, st = np.cos(theta), np.sin(theta)
    v1, v2 = s1 * s1, s2 * s2
    return ct * ct * v1 + st * st * v2, ct * st * (v1 - v2), st * st * v1 + ct * ct * v2


def level_radius(a, b, c, op, ux, uy):
    """distance from the centre at which alpha falls to 1/255 along the unit direction (ux, uy); 0 where opacity is
    below 1/255"""
    L = np.log(np.maximum(op * 255.0, 1.0))
    q = 0.5 * (a * ux * ux + c * uy * uy) + b * ux * uy
    return np.sqrt(L / np.maximum(q, 1e-300))


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def _ratio_for_rho(t, theta):
    """axis ratio k for which 1 - rho^2 = D4 / (4 hA hC) equals t at angle theta:
    a c / det = m / k^2 + (cos^4 + sin^4) + m k^2 with m = sin^2 cos^2"""
    c2, s2 = np.cos(theta) ** 2, np.sin(theta) ** 2
    m = c2 * s2
    w = (1.0 / t - (c2 * c2 + s2 * s2)) / m
    return np.sqrt(0.5 * (w + np.sqrt(np.maximum(w * w - 4.0, 0.0))))


# name -> (s1, s2, theta, opacity) float64 arrays of n Gaussians.  `size` scales the minor axis (pixels).
def shapes(family, rng, n, size=1.0):
    op = rng.uniform(0.05, 0.99, n)
    theta = rng.uniform(0.0, math.pi, n)
    s2 = _loguniform(rng, 0.35, 6.0, n) * size
    ratio = _loguniform(rng, 1.0, 300.0, n)
    if family == "axis_ratio":
        pass
    elif family == "fallback_boundary":
        # dense sweep of 1 - rho^2 across the 1e-2 switch between the closed form and the bounding box, both sides:
        # a third within 1e-5 relative, a third within 1 %, a third within a factor 2
        theta = np.where(rng.random(n) < 0.5, math.pi / 4, 3 * math.pi / 4) + rng.uniform(-0.5, 0.5, n) * (rng.random(n) < 0.5)
        spread = np.choose(rng.integers(0, 3, n), [1e-5, 1e-2, 0.7])
        t = 1e-2 * np.exp(rng.uniform(-1.0, 1.0, n) * spread)
        ratio = _ratio_for_rho(t, theta)
        s2 = _loguniform(rng, 0.35, 2.0, n) * size
    elif family == "faint":
        op = ALPHA_MIN * 2.0 ** rng.uniform(-0.03, 0.1, n)
        ratio = _loguniform(rng, 1.0, 30.0, n)
    elif family == "opaque":
        op = np.where(rng.random(n) < 0.3, 1.0, rng.uniform(0.99, 1.0, n))
        op = np.maximum(op, np.nextafter(np.float32(0.99), np.float32(1.0)))
    elif family == "round":
        ratio = _loguniform(rng, 1.0, 3.0, n)
    else:
        raise KeyError(family)
    return s2 * ratio, s2, theta, op


def records_of(x, y, op, a, b, c):
    """[n, 6] float32: the packed record's words x, y, opacity, conic.xx, conic.xy, conic.yy"""
    return np.ascontiguousarray(np.stack([x, y, op, a, b, c], axis=1).astype(np.float32))


def pipeline_radius(s1, s2):
    """ceil(3 sqrt(lambda_max)) as project_gaussians derives it"""
    return np.ceil(3.0 * np.maximum(s1, s2)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# block cases: one Gaussian, one rectangle of pixel INDICES [x0, x1] x [y0, y1] inside an 8x8 block
# ---------------------------------------------------------------------------------------------------------------------
def _rects(rng, n, kind):
    bx = rng.integers(0, 60, n) * 8
    by = rng.integers(0, 40, n) * 8
    x0 = rng.integers(0, 8, n); x1 = rng.integers(0, 8, n)
    y0 = rng.integers(0, 8, n); y1 = rng.integers(0, 8, n)
    x0, x1 = np.minimum(x0, x1), np.maximum(x0, x1)
    y0, y1 = np.minimum(y0, y1), np.maximum(y0, y1)
    full = rng.random(n) < 0.5                         # half of the blocks still have all 64 pixels live
    x0 = np.where(full, 0, x0); x1 = np.where(full, 7, x1); y0 = np.where(full, 0, y0); y1 = np.where(full, 7, y1)
    if kind == "degenerate":
        k = rng.integers(0, 3, n)                      # one pixel, one row, one column
        x1 = np.where(k != 1, x0, x1)
        y1 = np.where(k != 2, y0, y1)
    return np.stack([bx + x0, bx + x1, by + y0, by + y1], axis=1).astype(np.int64)


def _place_near_level_set(rng, rect, a, b, c, op, lo=0.9, hi=1.25):
    """centre such that a corner of the rectangle sits at `f` times the level-set radius, f uniform in [lo, hi], the
    rest of the rectangle on the far side of that corner as seen from the centre"""
    n = rect.shape[0]
    sx = rng.integers(0, 2, n); sy = rng.integers(0, 2, n)
    cx = np.where(sx == 1, rect[:, 1], rect[:, 0]).astype(np.float64)
    cy = np.where(sy == 1, rect[:, 3], rect[:, 2]).astype(np.float64)
    ang = rng.uniform(0.0, math.pi / 2, n)
    ux = np.cos(ang) * np.where(sx == 1, 1.0, -1.0)
    uy = np.sin(ang) * np.where(sy == 1, 1.0, -1.0)
    f = rng.uniform(lo, hi, n)
    r = level_radius(a, b, c, op, ux, uy)
    return cx + f * r * ux, cy + f * r * uy


def block_cases(family, seed, n, pix_off=0.0, max_ratio=None):
    """-> records [n,6] f32, rects [n,4] f32 (x0, x1, y0, y1 sample positions, inclusive)"""
    rng = np.random.default_rng(seed)
    rect = _rects(rng, n, "degenerate" if family == "degenerate_rects" else "any")
    shape_family = {"grid_centres": "axis_ratio", "far": "round", "degenerate_rects": "axis_ratio",
                    "tangent_bands": "axis_ratio", "non_psd": "round", "faint_on_threshold": "faint"}.get(family, family)
    s1, s2, theta, op = shapes(shape_family, rng, n)
    if max_ratio is not None:
        s1 = np.minimum(s1, s2 * max_ratio)
    if family == "far":
        # centres up to 4000 px away: round blobs as large as the distance, and needles that point at the block
        needle = (rng.random(n) < 0.5) & (max_ratio is None)
        dist = _loguniform(rng, 100.0, 4000.0, n)
        L = np.log(op * 255.0)
        s1 = dist / np.sqrt(2.0 * L)                   # level set reaches about `dist` along the major axis
        s2 = np.where(needle, s1 / _loguniform(rng, 5.0, 300.0, n), s1 / _loguniform(rng, 1.0, 2.0, n))
    a, b, c = conic_of(s1, s2, theta)
    if family == "far":
        # along the major axis (+- a few minor widths), so that needles are decided near their tip too
        n_ = rect.shape[0]
        sgn = np.where(rng.random(n_) < 0.5, 1.0, -1.0)
        f = rng.uniform(0.9, 1.25, n_)
        r = level_radius(a, b, c, op, np.cos(theta), np.sin(theta))
        side = rng.normal(0.0, 1.0, n_) * s2
        x = rect[:, 0] + sgn * f * r * np.cos(theta) - side * np.sin(theta)
        y = rect[:, 2] + sgn * f * r * np.sin(theta) + side * np.cos(theta)
    elif family == "tangent_bands":
        # the rectangle's first / last row tangent to the ellipse's bottom / top: |dy| = half height (1 +- 2e-3)
        _, vxy, vyy = cov_of(s1, s2, theta)
        H = np.sqrt(2.0 * np.log(op * 255.0) * vyy)
        f = 1.0 + rng.uniform(-2e-3, 2e-3, n)
        below = rng.random(n) < 0.5
        y = np.where(below, rect[:, 2] - f * H, rect[:, 3] + f * H)
        # x of the ellipse's top / bottom point, within the rectangle's columns
        xt = np.where(below, 1.0, -1.0) * H * vxy / vyy
        x = rng.uniform(rect[:, 0], rect[:, 1] + 1e-9) - xt
    elif family == "faint_on_threshold":
        # the centre a small fraction of the minor width off a corner, and the opacity such that the best sample of the
        # rectangle has alpha = 1/255 (1 +- 2e-6): the exponent to beat is ~1e-3, where the relative slack term of the
        # test is far below one rounding of log2(opacity) + log2(255) - only the absolute slack is left to cover it
        x, y = _place_near_level_set(rng, rect, a, b, c, np.full(n, 1.0), lo=0.0, hi=1.0)
        d = rng.uniform(0.005, 0.1, n) * s2
        cx = np.where(np.abs(x - rect[:, 0]) < np.abs(x - rect[:, 1]), rect[:, 0], rect[:, 1])
        cy = np.where(np.abs(y - rect[:, 2]) < np.abs(y - rect[:, 3]), rect[:, 2], rect[:, 3])
        r = np.hypot(x - cx, y - cy) + 1e-300
        x, y = cx + (x - cx) / r * d, cy + (y - cy) / r * d
        one = records_of(x, y, np.ones(n), a, b, c)
        op = ALPHA_MIN / block_alpha_max(one, rect.astype(np.float32)) * (1.0 + rng.uniform(-2e-6, 2e-6, n))
        # (a quarter clearly below the threshold, beyond the slack: blocks the test must still reject)
        op = op * np.where(rng.random(n) < 0.25, 2.0 ** -rng.uniform(0.021, 0.03, n), 1.0)
    else:
        x, y = _place_near_level_set(rng, rect, a, b, c, op)
    if family == "grid_centres":
        k = rng.integers(0, 3, n)
        snap = lambda v: np.where(k == 0, np.round(v), np.where(k == 1, np.floor(v) + 0.5, np.round(v / 16.0) * 16.0))
        x, y = snap(x), snap(y)
    if family == "non_psd":
        k = rng.integers(0, 5, n)
        g = np.sqrt(a * c)
        b = np.where(k == 0, np.sign(b + 1e-30) * g * rng.uniform(1.0, 4.0, n), b)          # |b| >= sqrt(a c)
        a = np.where(k == 1, 0.0, np.where(k == 2, -a, a))
        c = np.where(k == 3, 0.0, np.where(k == 4, -c, c))
    recs = records_of(x + pix_off, y + pix_off, op, a, b, c)
    return recs, np.ascontiguousarray((rect + pix_off).astype(np.float32))


BLOCK_FAMILIES = ["axis_ratio", "fallback_boundary", "faint", "opaque", "grid_centres", "far", "degenerate_rects",
                  "tangent_bands", "faint_on_threshold"]


def block_alpha_max(recs, rects):
    """float64 brute force: the largest alpha over the integer-spaced sample positions of each rectangle"""
    q = recs.astype(np.float64)
    r = rects.astype(np.float64)
    j = np.arange(8, dtype=np.float64)
    px = r[:, 0:1] + j[None, :]; py = r[:, 2:3] + j[None, :]
    okx = px <= r[:, 1:2]; oky = py <= r[:, 3:4]
    dx = (q[:, 0:1] - px)[:, None, :]; dy = (q[:, 1:2] - py)[:, :, None]
    a, b, c = q[:, 3, None, None], q[:, 4, None, None], q[:, 5, None, None]
    sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    with np.errstate(over="ignore"):
        alpha = q[:, 2, None, None] * np.exp(-sigma)
    alpha = np.where(oky[:, :, None] & okx[:, None, :], alpha, -np.inf)
    return alpha.reshape(len(q), -1).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# tile cases: one Gaussian with its integer radius on a W x H image
# ---------------------------------------------------------------------------------------------------------------------
TILE_FAMILIES = ["axis_ratio", "fallback_boundary", "faint", "opaque", "grid_centres", "far", "tangent_bands",
                 "extreme_in_band", "radius_edge", "faint_on_threshold", "needle_45"]


def tile_cases(family, seed, n, w, h, pix_off=0.0):
    """-> records [n,6] f32, radii [n] i32"""
    rng = np.random.default_rng(seed)
    shape_family = {"grid_centres": "axis_ratio", "far": "round", "tangent_bands": "axis_ratio",
                    "extreme_in_band": "axis_ratio", "radius_edge": "axis_ratio", "faint_on_threshold": "round",
                    "needle_45": "axis_ratio"}.get(family, family)
    s1, s2, theta, op = shapes(shape_family, rng, n, size=2.0)
    # keeps a bounding box to ~25 x 25 tiles; with a minor axis of at least 0.7 px it also limits the axis ratio of
    # these families to ~85 (the full 1 ... 300 is in "far" and "needle_45")
    shrink = np.minimum(1.0, 60.0 / s1)
    s1, s2 = s1 * shrink, s2 * shrink
    x = rng.uniform(-20.0, w + 20.0, n); y = rng.uniform(-20.0, h + 20.0, n)
    if family == "far":
        dist = _loguniform(rng, 100.0, 4000.0, n)
        L = np.log(op * 255.0)
        s1 = dist * rng.uniform(0.8, 1.1, n) / np.sqrt(2.0 * L)
        s2 = np.where(rng.random(n) < 0.5, s1 / _loguniform(rng, 5.0, 300.0, n), s1 / _loguniform(rng, 1.0, 2.0, n))
        # aimed at a point of the image from `dist` away
        tx_, ty_ = rng.uniform(0, w, n), rng.uniform(0, h, n)
        sgn = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        x = tx_ + sgn * dist * np.cos(theta); y = ty_ + sgn * dist * np.sin(theta)
    if family == "needle_45":
        # needles of axis ratio 20 ... 300 within 0.2 rad of a diagonal, at full size (major axis up to ~900 px): on
        # either side of the 1 - rho^2 = 1e-2 switch, where D4 cancels most
        theta = np.where(rng.random(n) < 0.5, math.pi / 4, 3 * math.pi / 4) + rng.uniform(-0.2, 0.2, n) * (rng.random(n) < 0.7)
        s2 = _loguniform(rng, 0.7, 3.0, n)
        s1 = s2 * _loguniform(rng, 20.0, 300.0, n)
    if family == "faint_on_threshold":
        # wide, nearly round Gaussians (30 ... 4000 px) whose opacity puts the best sample of the image at alpha =
        # 1/255 (1 +- 2e-6), under a SMALL radius: tau is 1e-7 ... 1e-3, the level set a few pixels across, and the
        # relative slack 4e-6 (hA + hC + |B|) far^2 is far below one rounding of log2(opacity) + log2(255)
        s2 = _loguniform(rng, 30.0, 4000.0, n)
        s1 = s2 * _loguniform(rng, 1.0, 3.0, n)
        k = rng.integers(0, 3, n)                      # anywhere / near a tile corner / a hair off a sample position
        x = rng.uniform(1.0, w - 2.0, n); y = rng.uniform(1.0, h - 2.0, n)
        x = np.where(k == 1, np.round(x / 16.0) * 16.0 + rng.uniform(-1.5, 1.5, n), x)
        y = np.where(k == 1, np.round(y / 16.0) * 16.0 + rng.uniform(-1.5, 1.5, n), y)
        x = np.where(k == 2, np.round(x) + rng.uniform(-0.06, 0.06, n), x)
        y = np.where(k == 2, np.round(y) + rng.uniform(-0.06, 0.06, n), y)
        x = np.clip(x, 1.0, w - 2.0); y = np.clip(y, 1.0, h - 2.0)
    a, b, c = conic_of(s1, s2, theta)
    if family == "faint_on_threshold":
        best = np.full(n, np.inf)
        for jx in (np.floor(x), np.floor(x) + 1.0):
            for jy in (np.floor(y), np.floor(y) + 1.0):
                dx, dy = x - jx, y - jy
                best = np.minimum(best, 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy)
        op = ALPHA_MIN * np.exp(best) * (1.0 + rng.uniform(-2e-6, 2e-6, n))
        # (a quarter clearly below the threshold, beyond the slack)
        op = op * np.where(rng.random(n) < 0.25, 2.0 ** -rng.uniform(0.021, 0.03, n), 1.0)
    vxx, vxy, vyy = cov_of(s1, s2, theta)
    L = np.log(np.maximum(op * 255.0, 1.0))
    Hh, Wh = np.sqrt(2.0 * L * vyy), np.sqrt(2.0 * L * vxx)           # half height / half width of the level set
    radius = pipeline_radius(s1, s2)
    if family == "grid_centres":
        k = rng.integers(0, 3, n)
        snap = lambda v: np.where(k == 0, np.round(v), np.where(k == 1, np.floor(v) + 0.5, np.round(v / 16.0) * 16.0))
        x, y = snap(x), snap(y)
    elif family == "tangent_bands":
        # the ellipse's bottom (top) on the first (last) sample row of a tile row, +- 2e-3 relative and +- 0.05 px
        row = rng.integers(0, (h + 15) // 16, n)
        below = rng.random(n) < 0.5
        f = 1.0 + rng.uniform(-2e-3, 2e-3, n) * (rng.random(n) < 0.5)
        jit = rng.uniform(-0.05, 0.05, n) * (rng.random(n) < 0.5)
        y = np.where(below, 16.0 * row - f * Hh, 16.0 * row + 15.0 + f * Hh) + jit
    elif family == "extreme_in_band":
        # the leftmost (rightmost) point of the ellipse within 2 kTightEps of a band edge, and on a tile's last
        # (first) sample column +- 0.05 px
        row = rng.integers(0, (h + 15) // 16, n)
        col = rng.integers(0, (w + 15) // 16, n)
        left = rng.random(n) < 0.5
        dy_ext = np.where(left, -1.0, 1.0) * Wh * vxy / vxx                 # dy of that extreme point
        edge = np.where(rng.random(n) < 0.5, 16.0 * row, 16.0 * row + 15.0)
        y = edge - dy_ext + rng.uniform(-0.04, 0.04, n)
        x = np.where(left, 16.0 * col + 15.0 + Wh, 16.0 * col - Wh) + rng.uniform(-0.05, 0.05, n)
    elif family == "faint_on_threshold":
        radius = np.choose(rng.integers(0, 5, n), [1, 1, 2, 5, 40]).astype(np.int32)
    elif family == "needle_45":
        # half with the ellipse's bottom / top on the first / last sample row of a tile row, half with its leftmost /
        # rightmost point on a band edge and a tile's last / first column; the pipeline's radius, or a smaller one
        row = rng.integers(0, (h + 15) // 16, n); col = rng.integers(0, (w + 15) // 16, n)
        flip = rng.random(n) < 0.5
        jit = rng.uniform(-0.04, 0.04, n) * (rng.random(n) < 0.7)
        y_t = np.where(flip, 16.0 * row - Hh, 16.0 * row + 15.0 + Hh)
        x_t = 16.0 * col + rng.uniform(0.0, 15.0, n) - np.where(flip, 1.0, -1.0) * Hh * vxy / vyy
        dy_ext = np.where(flip, -1.0, 1.0) * Wh * vxy / vxx
        y_e = np.where(rng.random(n) < 0.5, 16.0 * row, 16.0 * row + 15.0) - dy_ext
        x_e = np.where(flip, 16.0 * col + 15.0 + Wh, 16.0 * col - Wh)
        tangent = rng.random(n) < 0.5
        x = np.where(tangent, x_t, x_e) + jit; y = np.where(tangent, y_t, y_e) + jit[::-1]
        radius = np.where(rng.random(n) < 0.5, radius, np.ceil(radius * rng.uniform(0.02, 1.0, n))).astype(np.int32)
    elif family == "radius_edge":
        k = rng.integers(0, 3, n)
        radius = np.where(k == 0, 1, np.where(k == 1, radius + rng.integers(0, 3, n) * 16, 20000)).astype(np.int32)
    # (the kernels see sample = index + off: shift the whole configuration with the sample grid)
    return records_of(x + pix_off, y + pix_off, op, a, b, c), np.ascontiguousarray(radius.astype(np.int32))


def tile_pairs(boxes):
    """boxes [n,4] (minx, miny, maxx, maxy) -> flat (gaussian, tx, ty) of every bounding-box pair, and per-Gaussian
    row offsets into the (gaussian, tile row) arrays"""
    bw = np.maximum(boxes[:, 2] - boxes[:, 0], 0).astype(np.int64)
    bh = np.maximum(boxes[:, 3] - boxes[:, 1], 0).astype(np.int64)
    bh = np.where(bw > 0, bh, 0)
    cnt = bw * bh
    gi = np.repeat(np.arange(len(boxes)), cnt)
    first = np.cumsum(cnt) - cnt
    k = np.arange(cnt.sum()) - first[gi]
    tx = boxes[gi, 0] + k % np.maximum(bw[gi], 1)
    ty = boxes[gi, 1] + k // np.maximum(bw[gi], 1)
    row_off = np.cumsum(bh) - bh
    return gi, tx, ty, row_off, int(bh.sum())


def tile_alpha_max(recs, gi, tx, ty, pix_off=0.0, chunk=40000):
    """float64 brute force: the largest alpha over the 256 sample positions of tile (tx, ty) for Gaussian gi"""
    q = recs.astype(np.float64)
    out = np.empty(len(gi))
    j = np.arange(TILE, dtype=np.float64) + pix_off
    for s in range(0, len(gi), chunk):
        g = gi[s:s + chunk]
        dx = (q[g, 0:1] - (16.0 * tx[s:s + chunk, None] + j[None, :]))[:, None, :]
        dy = (q[g, 1:2] - (16.0 * ty[s:s + chunk, None] + j[None, :]))[:, :, None]
        a, b, c = q[g, 3, None, None], q[g, 4, None, None], q[g, 5, None, None]
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        with np.errstate(over="ignore"):
            out[s:s + chunk] = (q[g, 2, None, None] * np.exp(-sigma)).reshape(len(g), -1).max(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# compositing inputs: the block cases as the 2-D arguments of rasterize_gaussians
# ---------------------------------------------------------------------------------------------------------------------
COMPOSITE_W, COMPOSITE_H = 480, 320          # the image the block rectangles of _rects lie in
COMPOSITE_MAX_RATIO = 8.0


def composite_inputs(seed=0):
    """-> xys [n,2], depths [n], radii [n] i32, conics [n,3], colors [n,3], opacity [n,1] (float32 numpy), background:
    a few Gaussians per tile, each placed so that one 8x8 block is decided near its level set; colours near 1 over a
    black background, so that a block dropped although it is needed shows as an error of up to 1/255 of a colour.

    The image check compares float32 compositing with float64 at pixels whose float64 alpha is at least 1e-4
    (relative) away from 1/255: that presumes a float32 exponent good to well below 1e-4, i.e. a sum of |terms| of the
    exponent of a few hundred at most near the level set - axis ratios are limited to 8 here (the full range is the
    business of the host test), and the far-away Gaussians are round."""
    counts = {"axis_ratio": 500, "faint": 300, "opaque": 40, "grid_centres": 400, "far": 12, "degenerate_rects": 300,
              "tangent_bands": 400}
    recs = np.concatenate([block_cases(f, seed + 10 * k, m, max_ratio=COMPOSITE_MAX_RATIO)[0]
                           for k, (f, m) in enumerate(counts.items())])
    rng = np.random.default_rng(seed + 999)
    recs = recs[rng.permutation(len(recs))]
    a, b, c = (recs[:, k].astype(np.float64) for k in (3, 4, 5))
    det = a * c - b * b
    mid = 0.5 * (a + c) / det
    lam = mid + np.sqrt(np.maximum(mid * mid - 1.0 / det, 0.0))
    radii = np.ceil(3.5 * np.sqrt(lam)).astype(np.int32)       # the whole level set inside the box: the block cull decides
    n = len(recs)
    depths = rng.permutation(n).astype(np.float32) * 0.01 + 1.0
    colors = rng.uniform(0.9, 1.0, (n, 3)).astype(np.float32)
    return (np.ascontiguousarray(recs[:, :2]), depths, radii, np.ascontiguousarray(recs[:, 3:6]), colors,
            np.ascontiguousarray(recs[:, 2:3]), np.zeros(3, dtype=np.float32))
