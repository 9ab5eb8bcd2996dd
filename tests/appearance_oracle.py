"""A plain numpy restatement of the per-view appearance model for the tests.

The coordinates - grid cell, fraction, luminance level - are float32 by definition (each operation rounded on its own)
and are restated here in numpy float32; everything after them is float64.  Beside every output the oracle returns the sum
of the absolute values of its terms, expanded in the lerp form a + t (b - a) that the kernels evaluate:
``absum(lerp(a, b, t)) = absum(a) + t (absum(b) + absum(a))``.  A float32 evaluation whose longest path has n roundings
differs from the float64 value by at most n 2^-24 of that sum, to first order.
"""
import numpy as np

LUM = (np.float32(0.299), np.float32(0.587), np.float32(0.114))


def axis(P, G):
    """-> (i0, i1 int64 [P], t float32 [P]) of the pixels 0..P-1 along an axis with G vertices."""
    if G == 1:
        z = np.zeros(P, np.int64)
        return z, z.copy(), np.zeros(P, np.float32)
    u = ((np.arange(P, dtype=np.float32) + np.float32(0.5)) / np.float32(P)) * np.float32(G - 1)
    i0 = np.minimum(u.astype(np.int64), G - 2)
    return i0, i0 + 1, (u - i0.astype(np.float32)).astype(np.float32)


def level(image, L):
    """image float32 [H, W, 3] -> dict(w, l0, l1, t, inside)."""
    r, g, b = (image[..., k].astype(np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        gray = (LUM[0] * r + LUM[1] * g) + LUM[2] * b
        top = np.float32(L - 1)
        w = (gray * top).astype(np.float32)
    wc = np.where(w > 0, w, np.float32(0)).astype(np.float32)
    wc = np.minimum(wc, top)
    inside = (w > 0) & (w < top)
    if L == 1:
        z = np.zeros(w.shape, np.int64)
        return dict(w=w, l0=z, l1=z.copy(), t=np.zeros(w.shape, np.float32), inside=inside)
    l0 = np.minimum(wc.astype(np.int64), L - 2)
    return dict(w=w, l0=l0, l1=l0 + 1, t=(wc - l0.astype(np.float32)).astype(np.float32), inside=inside)


def _lerp(a, b, t, absolute):
    return a + t * (b + a) if absolute else a + t * (b - a)


def _level_matrix(G, l, j0, j1, i0, i1, tx, ty, absolute):
    """[H, W, 12]: the level's four vertices interpolated along x, then y."""
    J0, J1, I0, I1 = j0[:, None], j1[:, None], i0[None, :], i1[None, :]
    tx, ty = tx[None, :, None], ty[:, None, None]
    top = _lerp(G[l, J0, I0], G[l, J0, I1], tx, absolute)
    bot = _lerp(G[l, J1, I0], G[l, J1, I1], tx, absolute)
    return _lerp(top, bot, ty, absolute)


def _slices(image, grid):
    H, W, _ = image.shape
    L, Gh, Gw, _ = grid.shape
    i0, i1, tx = axis(W, Gw)
    j0, j1, ty = axis(H, Gh)
    z = level(image, L)
    tx64, ty64, tz64 = tx.astype(np.float64), ty.astype(np.float64), z["t"].astype(np.float64)
    out = dict(i0=i0, i1=i1, tx=tx64, j0=j0, j1=j1, ty=ty64, z=z, tz=tz64)
    for name, G, absolute in (("A", grid.astype(np.float64), False), ("S", np.abs(grid.astype(np.float64)), True)):
        out[name + "0"] = _level_matrix(G, z["l0"], j0, j1, i0, i1, tx64, ty64, absolute)
        out[name + "1"] = _level_matrix(G, z["l1"], j0, j1, i0, i1, tx64, ty64, absolute)
        out[name] = _lerp(out[name + "0"], out[name + "1"], tz64[..., None], absolute)
    return out


def forward(image, grid):
    """-> (out float64 [H, W, 3], the sum of |terms| of every output)."""
    s = _slices(image, grid)
    x = np.concatenate([image.astype(np.float64), np.ones(image.shape[:2] + (1,))], axis=2)
    A, S = s["A"].reshape(image.shape[:2] + (3, 4)), s["S"].reshape(image.shape[:2] + (3, 4))
    with np.errstate(all="ignore"):
        return np.einsum("hwrk,hwk->hwr", A, x), np.einsum("hwrk,hwk->hwr", S, np.abs(x))


def backward(image, grid, v_out):
    """-> dict(v_image, v_image_abs [H, W, 3]; v_grid, v_grid_abs [L, Gh, Gw, 12]), all float64."""
    H, W, _ = image.shape
    L, Gh, Gw, _ = grid.shape
    s = _slices(image, grid)
    V = v_out.astype(np.float64)
    x = np.concatenate([image.astype(np.float64), np.ones((H, W, 1))], axis=2)
    vA = (V[..., :, None] * x[..., None, :]).reshape(H, W, 12)
    A, S = s["A"].reshape(H, W, 3, 4), s["S"].reshape(H, W, 3, 4)
    lum = np.array([float(v) for v in LUM])
    slope = s["z"]["inside"][..., None] * float(L - 1) * lum[None, None, :]
    guide = (vA * (s["A1"] - s["A0"])).sum(axis=2)
    guide_abs = (np.abs(vA) * (s["S1"] + s["S0"])).sum(axis=2)
    v_image = np.einsum("hwrk,hwr->hwk", A, V)[..., :3] + slope * guide[..., None]
    v_image_abs = np.einsum("hwrk,hwr->hwk", S, np.abs(V))[..., :3] + slope * guide_abs[..., None]
    v_grid, v_grid_abs = np.zeros(grid.shape, np.float64), np.zeros(grid.shape, np.float64)
    z = s["z"]
    jj0, jj1 = np.broadcast_to(s["j0"][:, None], (H, W)), np.broadcast_to(s["j1"][:, None], (H, W))
    ii0, ii1 = np.broadcast_to(s["i0"][None, :], (H, W)), np.broadcast_to(s["i1"][None, :], (H, W))
    ty, tx = np.broadcast_to(s["ty"][:, None], (H, W)), np.broadcast_to(s["tx"][None, :], (H, W))
    for l, fz in ((z["l0"], 1.0 - s["tz"]), (z["l1"], s["tz"])):
        for j, fy in ((jj0, 1.0 - ty), (jj1, ty)):
            for i, fx in ((ii0, 1.0 - tx), (ii1, tx)):
                f = (fz * fy * fx)[..., None]
                np.add.at(v_grid, (l, j, i), f * vA)
                np.add.at(v_grid_abs, (l, j, i), f * np.abs(vA))
    return dict(v_image=v_image, v_image_abs=v_image_abs, v_grid=v_grid, v_grid_abs=v_grid_abs)


def tv(grid):
    """-> (tv(grid), d tv / d grid), float64: over the axes of size > 1, the mean squared difference of neighbours."""
    G = grid.astype(np.float64)
    value, grad = 0.0, np.zeros_like(G)
    for a in range(3):                                   # z, y, x: the order does not matter in float64 beyond 1e-16
        if G.shape[a] == 1:
            continue
        d = np.diff(G, axis=a)
        value += float((d * d).mean())
        g = np.zeros_like(G)
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        g[tuple(hi)] += d
        g[tuple(lo)] -= d
        grad += 2.0 * g / d.size
    return value, grad


def fit_sums(image, target):
    """-> float64 [22]: rr rg rb r gg gb g bb b 1, then phi_k t_c at 10 + 3 k + c (target float32, or uint8 for b / 255)."""
    if target.dtype == np.uint8:
        target = target.astype(np.float32) / np.float32(255.0)
    x = np.concatenate([image.reshape(-1, 3).astype(np.float64), np.ones((image.shape[0] * image.shape[1], 1))], axis=1)
    t = target.reshape(-1, 3).astype(np.float64)
    S, B = x.T @ x, x.T @ t
    return np.concatenate([S[np.triu_indices(4)], B.reshape(-1)])
