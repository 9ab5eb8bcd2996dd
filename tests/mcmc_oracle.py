"""Float64 oracle of the budgeted densifier, numpy / torch.  TEST INFRASTRUCTURE ONLY.

It restates the definitions of section 6r, not the kernels: the binomials are ``math.comb``, the series is summed term by
term in float64, the prefix sum repeats the fixed ORDER of csrc/prefix_scan.h (which is part of the definition: a draw
depends on it), and the bounds the float32 results are held to are derived here from the formats, never from what the
kernels give.  EPS = 2^-24 is float32's unit roundoff; an operation rounded to nearest errs by at most EPS relative, a
library function documented to 1 ulp by at most 2 EPS."""
import math

import numpy as np

EPS = 2.0 ** -24
N_MAX = 51
TOP = 1.0 - 2.0 ** -23
MIN_OPACITY = 0.005
F32_0995 = np.float32(0.995)
DOUBLE = 2e-10


def sigmoid32(x):
    """the float32 nearest to sigmoid(x), evaluated in float64: the o of section 6r"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def logit_just_above(p):
    """the smallest float32 logit whose sigmoid32 exceeds float32(p)"""
    p = np.float32(p)
    x = np.float32(math.log(float(p) / (1.0 - float(p)))) - np.float32(1e-3)
    while not sigmoid32(x) > p:
        x = np.nextafter(x, np.float32(np.inf))
    return x


# ------------------------------------------------------------------------------------------------ relocation
def split_opacity(o, M):
    """o' = 1 - (1 - o)^(1/M)"""
    with np.errstate(divide="ignore"):
        return -np.expm1(np.log1p(-np.float64(o)) / M)


# C(a-1, k) (-1)^k / sqrt(k+1): the binomials are exact in float64 (C(50, 25) < 2^47)
_COEF = np.array([[math.comb(a, k) * (-1.0) ** k / math.sqrt(k + 1) if k <= a else 0.0 for k in range(N_MAX)]
                  for a in range(N_MAX)])


def series(op, M):
    """D = sum_{a=1..M} sum_{k=0..a-1} C(a-1,k) (-1)^k o'^(k+1) / sqrt(k+1), row by row"""
    pw = np.float64(op) ** np.arange(1, M + 1)
    s = np.float64(0.0)
    for a in range(1, M + 1):
        s += _COEF[a - 1, :a] @ pw[:a]
    return s


def capped(o):
    """an opacity that has rounded to 1 counts as the largest float32 below 1 (section 6r: at o' = 1 no double sum of D
    keeps a digit)"""
    return np.float64(min(np.float64(o), 1.0 - 2.0 ** -24))


def new_opacity(o, M):
    return split_opacity(capped(o), M)


def coeff(o, M):
    o = capped(o)
    D = series(split_opacity(o, M), M)
    return o / D if D > 0 else np.float64(1.0)


def coeff_decimal(o, M, digits=80):
    """o / D with every term in ``digits``-digit decimal arithmetic: what the float64 sums are measured against"""
    from decimal import Decimal, getcontext
    getcontext().prec = digits
    od = Decimal(float(capped(o)))
    op = 1 - ((1 - od).ln() / M).exp()
    D = Decimal(0)
    for a in range(1, M + 1):
        for k in range(a):
            D += Decimal(math.comb(a - 1, k)) * (-1) ** k * op ** (k + 1) / Decimal(k + 1).sqrt()
    return float(od / D)


def relocate_row(o32, count, min_opacity=MIN_OPACITY):
    """A picked row: -> (new logit, log coeff, p) in float64, with p = clamp(float32(o'), float32(min), 1 - 2^-23): the
    single rounding of o' to float32 is part of the definition."""
    M = min(int(count) + 1, N_MAX)
    p = np.float32(new_opacity(o32, M))
    p = min(max(p, np.float32(min_opacity)), np.float32(TOP))
    p = np.float64(p)
    return math.log(p / (1.0 - p)), math.log(coeff(o32, M)), p


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def relocation_tolerances(logit, logc, p, new_scale):
    """What the float32 chain may add to the float64 values, rounding by rounding.
    opacity: the cast of o' (relative EPS on p: EPS / (1 - p) in the logit), 1 - p and the quotient (EPS each), logf at
    1 ulp of the result.  scales: the cast of o / D (EPS in its logarithm), logf at 1 ulp of log(o / D), the final add
    (half an ulp of the sum).  DOUBLE covers the two double evaluations of D, whose 1 326 terms reach 2.4e3 against a sum
    of 2: 1326 * 2.4e3 * 2^-53 / 2 < 2e-10 relative at the very worst (they agree to 1e-13 in practice)."""
    tol_o = EPS / (1.0 - p) + 2.0 * EPS + ulp32(logit) + 1e-15 / (p * (1.0 - p))
    tol_s = EPS + ulp32(logc) + 0.5 * ulp32(new_scale) + DOUBLE
    return tol_o, tol_s


# ------------------------------------------------------------------------------------------------ prefix and draws
THREADS, ITEMS = 256, 8


def _tree(acc):
    """Hillis-Steele over 256 values: sh[t] += sh[t - off] for off = 1, 2, ..., 128 (all lanes at once)"""
    sh = np.array(acc, dtype=np.float64)
    off = 1
    while off < THREADS:
        v = np.concatenate((np.zeros(off), sh[:-off]))
        sh = sh + v
        off <<= 1
    return sh


def scan_prefix(w):
    """The inclusive prefix of csrc/prefix_scan.h, addition by addition."""
    w = np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    block = THREADS * ITEMS
    nb = (n + block - 1) // block
    out = np.zeros(n)
    totals = np.zeros(nb)
    for b in range(nb):
        chunk = np.zeros(block)
        m = min(block, n - b * block)
        chunk[:m] = w[b * block:b * block + m]
        loc = np.zeros((THREADS, ITEMS))
        acc = np.zeros(THREADS)
        for t in range(ITEMS):
            acc = acc + chunk.reshape(THREADS, ITEMS)[:, t]
            loc[:, t] = acc
        sh = _tree(acc)
        before = np.concatenate(([0.0], sh[:-1]))
        out[b * block:b * block + m] = (before[:, None] + loc).reshape(-1)[:m]
        totals[b] = sh[-1]
    per = (nb + THREADS - 1) // THREADS
    acc = np.zeros(THREADS)
    for t in range(THREADS):
        for b in range(t * per, min(t * per + per, nb)):
            acc[t] += totals[b]
    sh = _tree(acc)
    offsets = np.zeros(nb)
    for t in range(THREADS):
        run = sh[t - 1] if t > 0 else 0.0
        for b in range(t * per, min(t * per + per, nb)):
            offsets[b] = run
            run += totals[b]
    return out + np.repeat(offsets, block)[:n]


def pick(P, w, target):
    """the bisection for the first P > target; from a row of weight 0 to the nearest earlier live row, else the next"""
    n = len(P)
    lo, hi = 0, n - 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if P[mid] > target:
            hi = mid
        else:
            lo = mid + 1
    r = lo
    while r > 0 and not w[r] > 0:
        r -= 1
    while r < n - 1 and not w[r] > 0:
        r += 1
    return r if w[r] > 0 else -1


def sample(w, u):
    """-> (picks, counts) of the draws ``u`` (float32) over the weights ``w`` (float64)"""
    w = np.asarray(w, dtype=np.float64)
    P = scan_prefix(w)
    picks = np.array([pick(P, w, np.float64(np.float32(x)) * P[-1]) for x in np.asarray(u)], dtype=np.int64)
    counts = np.bincount(picks[picks >= 0], minlength=len(w))
    return picks, counts


def weights(logits, min_opacity=MIN_OPACITY, zero_dead=True):
    """-> (w float64, dead bool)"""
    o = sigmoid32(np.asarray(logits).reshape(-1))
    dead = ~(o > np.float32(min_opacity))
    w = o.astype(np.float64)
    w[~(o > 0)] = 0.0
    if zero_dead:
        w[dead] = 0.0
    return w, dead


# ------------------------------------------------------------------------------------------------ Philox and normals
def philox4x32_10(ctr, key):
    c, k = [int(v) for v in ctr], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def uniform32(x):
    return (np.float32(x >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)


def normals(seed, step, rows):
    """-> (z float64 [len(rows),3], radius float64 [len(rows),3]): Box-Muller in float64 on the float32 uniforms"""
    two_pi = np.float64(np.float32(6.2831853071795864769))
    z, rad = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    for j, i in enumerate(rows):
        x = philox4x32_10([int(i), int(step), 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        u = [np.float64(uniform32(v)) for v in x]
        a0 = np.float64(np.float32(two_pi * u[1]))          # the float32 product is part of the definition
        a1 = np.float64(np.float32(two_pi * u[3]))
        r0, r1 = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
        z[j] = (r0 * math.cos(a0), r0 * math.sin(a0), r1 * math.cos(a1))
        rad[j] = (r0, r0, r1)
    return z, rad


def normals_tolerance(z, rad):
    """logf at 1 ulp and the -2 product and the root: the radius to 2.5 EPS relative; cosf / sinf at 2 ulp of a value
    <= 1: 4 EPS absolute; the product: EPS."""
    return rad * (4.0 * EPS) + np.abs(z) * (3.5 * EPS)


# ------------------------------------------------------------------------------------------------ noise
def gate(o):
    o = np.asarray(o, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - np.float64(F32_0995))))


def noise(means, scales, quats, logits, scale, z):
    """-> (new means float64, bound float64 [N], g float64 [N]).

    The bound, per row, on |float32 result - float64 result| in every component:
      the gate: o = sigmoid in float32 errs by <= 4 EPS (expf 2, the sum 1, the quotient 1); 1 - o and the difference
        with 0.995 add 2 EPS; times 100, plus the product's own rounding of a value <= 100: the exponent errs by
        <= 700 EPS absolute; expf 2 EPS, the sum and the quotient 2 EPS: g to 704 EPS relative;
      Sigma z: R's entries to <= 10 EPS absolute (norm, four quotients, products and sums of values <= 1), two 3-term
        dot products (3 EPS each), exp(2 s) to 2 EPS: <= 2 * (3 * 10 + 3) + 2 < 70 EPS of |Sigma| |z|, |Sigma| = exp(2
        max s);
      scale * g, its product with Sigma z and the final sum: 2 EPS of the step and EPS of the result.
    """
    means, scales, quats, z = (np.asarray(a, dtype=np.float64) for a in (means, scales, quats, z))
    o = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64).reshape(-1)))
    g = gate(o)
    q = quats / np.linalg.norm(quats, axis=1, keepdims=True)
    w, x, y, zz = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y)], -1),
                  np.stack([2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x)], -1),
                  np.stack([2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    t = np.einsum("nji,nj->ni", R, z) * np.exp(2.0 * scales)
    d = np.einsum("nij,nj->ni", R, t)
    step = (float(scale) * g)[:, None] * d
    new = means + step
    sigma = np.exp(2.0 * scales.max(axis=1))
    size = float(scale) * g * sigma * np.linalg.norm(z, axis=1)
    bound = (704 + 70 + 2) * EPS * size + EPS * np.abs(new).max(axis=1) + 1e-30
    return new, bound, g


# ------------------------------------------------------------------------------------------------ regularisers
def mean_terms(x, kind):
    """-> (value, gradient) of mean(sigmoid(x)) / mean(exp(x)) by torch autograd in float64"""
    import torch
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    v = torch.sigmoid(t).mean() if kind == "sigmoid" else torch.exp(t).mean()
    v.backward()
    return v.item(), t.grad.numpy()


# ------------------------------------------------------------------------------------------------ the host build
def build_host(out_dir):
    """g++ build of tests/hostmath/mcmc.cpp (csrc/mcmc_math.h compiled for the host, uncontracted) -> the ctypes library"""
    import ctypes
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    so = Path(out_dir) / "_mcmc.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(root / "tests" / "hostmath" / "mcmc.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    f, d, i32, u32, u64 = ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    F32P, F64P, I32P, U32P = (ctypes.POINTER(t) for t in (f, d, i32, u32))
    lib.mc_n_max.restype, lib.mc_n_max.argtypes = i32, []
    lib.mc_binom.restype, lib.mc_binom.argtypes = u64, [i32, i32]
    lib.mc_sigmoid.restype, lib.mc_sigmoid.argtypes = f, [f]
    lib.mc_pick.restype, lib.mc_pick.argtypes = i32, [i32, F64P, F64P, d]
    lib.mc_sample.restype, lib.mc_sample.argtypes = None, [i32, i32, F64P, F64P, F32P, I32P]
    lib.mc_split_opacity.restype, lib.mc_split_opacity.argtypes = d, [d, i32]
    lib.mc_series.restype, lib.mc_series.argtypes = d, [d, i32]
    lib.mc_relocate_values.restype, lib.mc_relocate_values.argtypes = None, [f, i32, F32P, F32P]
    lib.mc_relocate.restype, lib.mc_relocate.argtypes = None, [f, i32, f, F32P, F32P]
    lib.mc_philox.restype, lib.mc_philox.argtypes = None, [U32P, U32P, U32P]
    lib.mc_uniform.restype, lib.mc_uniform.argtypes = f, [u32]
    lib.mc_normals.restype, lib.mc_normals.argtypes = None, [u64, u32, u32, i32, F32P]
    lib.mc_gate.restype, lib.mc_gate.argtypes = f, [f]
    lib.mc_sigma_z.restype, lib.mc_sigma_z.argtypes = None, [F32P, F32P, F32P, F32P]
    return lib
