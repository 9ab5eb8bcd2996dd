"""Float64 yardstick of the depth-map fusion (tinysplat_amd.fusion), plain numpy.

The definition, restated.  Inputs are the float32 values the kernels see (corner positions ``lo + (i, j, k) * h``, the
view matrix, ``PV = float32(proj @ view)`` with the product taken in double, the float32 ``trunc``, the depth maps);
everything from there is float64.  Per corner x and camera c, in list order: ``z = V_2 . x~``, skipped if ``z <= znear``;
``u = (W / 2) (PV_0 . x~ / (PV_3 . x~ + 1e-6)) + W / 2 - 0.5`` and likewise v with H (where ``project_gaussians`` puts a
Gaussian's centre), ``px = rint(u)``, ``py = rint(v)``, skipped outside the image; ``d = depth[py, px]``, skipped if not
finite, ``<= 0`` or ``> depth_max``; ``s = d - z``, skipped if ``s < -trunc``; the observation is ``t = min(1, s / trunc)``.
``F = -(sum t) / count``, NaN where ``count < min_observations``.  ``march`` / ``weld`` / ``edge_census`` are
tests/mesh_oracle.py's; a cell with a NaN corner emits nothing.

**Decision-unstable corners.**  A (corner, camera) decision is unstable when the quantity sits within a relative 1e-4 of
its threshold, and never closer than four times the float32 rounding the kernel's own evaluation can carry (U = 2^-24; a
sum of three products and a constant, evaluated left to right, carries at most 4 U A with A the sum of the terms'
magnitudes):
  z against znear         |z - znear| <= max(1e-4 znear, 4 E_z),  E_z = 4 U A_z
  rint and the border     the distance of u (of v) to the nearest half-integer - the image's borders -0.5 and W - 0.5 are
                          half-integers too - <= max(1e-4 of a pixel, 4 E_u); E_u from E_hx = 4 U A_x, E_hw = 4 U A_w + U |hw|:
                          q = hx / hw' carries E_q = E_hx / |hw'| + |q| (E_hw / |hw'| + 2 U), u carries (W / 2) E_q + 3 U (W + |u|)
  s against -trunc        |s + trunc| <= max(1e-4 trunc, 4 E_s),  E_s = E_z + U (|d| + |z|)
  d against depth_max     |d - depth_max| <= 1e-4 depth_max
A decision counts where the walk reaches it in float64.  A corner is unstable when any of its decisions is.

**The error bound of F** at a stable corner, derived, not measured.  An observation's float32 value differs from the
float64 one by the rounding of z (4 U A_z, above), of s = d - z (U |s| <= U (|d| + A_z)) and of the quotient s / trunc
(U |t| <= U (|d| + A_z) / trunc); min(1, .) does not enlarge a difference.  That is (6 A_z + 2 |d|) U / trunc
<= 6 U (A_z + |d|) / trunc to first order; the multiple stated is **8**, which leaves the second-order terms of
(1 + U)^4 and the 2^-53 steps of the double sum and quotient two parts in eight.  F is the mean of the observations,
rounded once to float32: ``bound = mean_obs(8 U (A_z + |d|) / trunc) + U |F|``.
"""
import numpy as np

import mesh_oracle as MO

U = 2.0 ** -24
REL = 1e-4
MULTIPLE = 8.0
EPS_W = float(np.float32(1e-6))


def projview(view, proj):
    """float32 [4,4]: the double product of the float32 matrices, rounded once."""
    return (np.asarray(proj, np.float32).astype(np.float64) @ np.asarray(view, np.float32).astype(np.float64)).astype(np.float32)


def observe(cam, x, trunc, znear=0.001, depth_max=np.inf):
    """One camera over corners ``x`` float32 [..., 3] -> dict of float64 / bool arrays of x's leading shape: ``seen`` (the
    pair contributes), ``t``, ``z``, ``u``, ``v``, ``px``, ``py``, ``in_image`` (steps 1 and 2 passed), ``unstable`` and
    ``e_t`` (the observation's error bound).  ``cam``: dict(view float32 [4,4], proj float32 [4,4], depth float32 [H,W])."""
    x = np.asarray(x, np.float32).astype(np.float64)
    V = np.asarray(cam["view"], np.float32).astype(np.float64)
    P = projview(cam["view"], cam["proj"]).astype(np.float64)
    depth = np.asarray(cam["depth"], np.float32)
    H, W = depth.shape
    trunc = float(np.float32(trunc))

    def dot(row):
        terms = x * row[:3]
        return terms.sum(-1) + row[3], np.abs(terms).sum(-1) + abs(row[3])
    z, a_z = dot(V[2])
    hx, a_x = dot(P[0])
    hy, a_y = dot(P[1])
    hw, a_w = dot(P[3])
    e_z = 4 * U * a_z
    unstable = np.abs(z - znear) <= np.maximum(REL * abs(znear), 4 * e_z)
    front = z > znear
    hwp = hw + EPS_W
    with np.errstate(divide="ignore", invalid="ignore"):
        e_hw = 4 * U * a_w + U * np.abs(hw)
        out = {}
        near_half = np.zeros(x.shape[:-1], dtype=bool)
        for name, hn, a_n, size in (("u", hx, a_x, W), ("v", hy, a_y, H)):
            q = hn / hwp
            pix = 0.5 * size * q + 0.5 * size - 0.5
            e_q = 4 * U * a_n / np.abs(hwp) + np.abs(q) * (e_hw / np.abs(hwp) + 2 * U)
            e_pix = 0.5 * size * e_q + 3 * U * (size + np.abs(pix))
            dist = np.abs(pix - (np.floor(pix) + 0.5))
            # a half-integer beyond the image's own borders separates two pixels that are both outside: no decision
            relevant = ~((pix <= -1.5) | (pix >= size + 0.5))
            near_half |= relevant & ~(dist > np.maximum(REL, 4 * e_pix))         # NaN counts as unstable
            out[name] = pix
    unstable |= front & near_half
    with np.errstate(invalid="ignore"):
        px, py = np.rint(out["u"]), np.rint(out["v"])
        in_image = front & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    ix = np.where(in_image, px, 0).astype(np.int64)
    iy = np.where(in_image, py, 0).astype(np.int64)
    d32 = depth[iy, ix]
    d = d32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        has = in_image & np.isfinite(d32) & (d32 > 0)
        if np.isfinite(depth_max):
            unstable |= has & (np.abs(d - depth_max) <= REL * depth_max)
        has &= ~(d > depth_max)
        dd = np.where(has, d, 0.0)
        s = dd - z
        e_s = e_z + U * (np.abs(dd) + np.abs(z))
        unstable |= has & (np.abs(s + trunc) <= np.maximum(REL * trunc, 4 * e_s))
        seen = has & ~(s < -trunc)
        t = np.where(seen, np.minimum(1.0, s / trunc), 0.0)
    e_t = np.where(seen, MULTIPLE * U * (a_z + np.abs(dd)) / trunc, 0.0)
    out.update(seen=seen, t=t, z=z, px=px, py=py, in_image=in_image, unstable=unstable, e_t=e_t, d=dd, has=has)
    return out


def fuse(lo, h, cells, cams, trunc, znear=0.001, depth_max=np.inf, min_observations=1):
    """The dense field -> dict(F float64 [Z,Y,X] with NaN, count int64, unstable bool, bound float64, positions float32
    [Z,Y,X,3], negative bool (some camera observed the corner with t < 0))."""
    positions = MO.corner_positions(lo, h, cells)
    shape = positions.shape[:3]
    total, e_sum = np.zeros(shape), np.zeros(shape)
    count = np.zeros(shape, dtype=np.int64)
    unstable, negative = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    for cam in cams:                                        # list order: the double sum's order
        o = observe(cam, positions, trunc, znear, depth_max)
        total = total + o["t"]
        e_sum += o["e_t"]
        count += o["seen"]
        unstable |= o["unstable"]
        negative |= o["seen"] & (o["t"] < 0)
    known = count >= min_observations
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where(known, -(total / count), np.nan)
        bound = np.where(known, e_sum / np.maximum(count, 1) + U * np.abs(np.nan_to_num(F)), 0.0)
    return dict(F=F, count=count, unstable=unstable, bound=bound, positions=positions, negative=negative)


def nan_cells(F):
    """[Z,Y,X] -> bool [nz,ny,nx]: the cell has a NaN corner."""
    bad = np.isnan(np.asarray(F))
    nz, ny, nx = (s - 1 for s in bad.shape)
    out = np.zeros((nz, ny, nx), dtype=bool)
    for c in range(8):
        out |= bad[(c >> 2):(c >> 2) + nz, ((c >> 1) & 1):((c >> 1) & 1) + ny, (c & 1):(c & 1) + nx]
    return out


def march_observed(F, positions=None):
    """``mesh_oracle.march`` at level 0 in F's own precision, without the triangles of cells that have a NaN corner."""
    F = np.asarray(F)
    m = MO.march(F, F.dtype.type(0), None)
    keep = ~nan_cells(F).reshape(-1)[m["cell"]] if m["cell"].size else np.zeros((0,), dtype=bool)
    out = {"keys": m["keys"][keep], "cell": m["cell"][keep], "ends": m["ends"][keep]}
    if positions is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["pos"] = MO.interpolate(F, F.dtype.type(0), positions, out["ends"])
    return out


def brick_corner_index(active, cells):
    """[A,729,3] global corner coordinates (x, y, z) of the listed bricks and the mask of corners inside the grid."""
    active = np.asarray(active, dtype=np.int64)
    nb = [-(-c // 8) for c in cells]
    b = np.stack((active % nb[0], (active // nb[0]) % nb[1], active // (nb[0] * nb[1])), -1)
    l = np.arange(729)
    loc = np.stack((l % 9, (l // 9) % 9, l // 81), -1)
    g = b[:, None, :] * 8 + loc[None, :, :]
    return g, np.all(g <= np.asarray(cells)[None, None, :], axis=-1)


def brick_of_cells(cell_mask):
    """bool [nz,ny,nx] -> the sorted ids of the bricks that hold a flagged cell."""
    nz, ny, nx = cell_mask.shape
    nb = [-(-nx // 8), -(-ny // 8), -(-nz // 8)]
    k, j, i = np.nonzero(cell_mask)
    return np.unique(((k // 8) * nb[1] + j // 8) * nb[0] + i // 8)
