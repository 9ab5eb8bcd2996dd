"""The .splat record in numpy float64: keys, the stable descending order, encode, decode.  Test
infrastructure only: the package never imports it.  Inputs are the model's float32 arrays; every expression is evaluated
in float64 from them."""
import numpy as np

C0 = 0.28209479177387814
FLT_MIN = float(np.finfo(np.float32).tiny)
RECORD_BYTES = 32
# the byte-comparison rule: a byte may differ by one from the oracle's only where the oracle's value before truncation
# lies within EPS of an integer.  Sixteen float32 unit round-offs (2^-24) at magnitude 256: an upper bound for the at most
# eight float32 operations of either expression with library functions of at most 2 ulp.
EPS = 16 * 2.0 ** -24 * 256
MAX_EXCUSED_SHARE = 0.005


def _sigmoid(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(o, np.float64)))


def keys(scales, opacities):
    """float64 [n]: exp(s0 + s1 + s2) sigmoid(opacity)."""
    s = np.asarray(scales, np.float64).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(s[:, 0] + s[:, 1] + s[:, 2]) * _sigmoid(np.asarray(opacities).reshape(-1))


def order(k):
    """int64 [n]: descending keys, ties to the smaller index, NaN last."""
    return np.argsort(-np.asarray(k), kind="stable").astype(np.int64)


def _clip_trunc(v):
    """trunc(clip(v, 0, 255)) with NaN -> 0, and v itself: the value before the clip and the truncation."""
    return np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 255.0).astype(np.uint8), v


def encode(means, scales, colors_dc, opacities, quats):
    """-> (records uint8 [n,32], pre float64 [n,32]).  pre[:, 24:32] holds, per byte, the value before the clip and
    the truncation (elsewhere NaN: the float32 fields are not truncations).  A value far outside [0, 255] is far from
    every integer that matters: its byte is 0 or 255 on either side of any rounding."""
    means = np.ascontiguousarray(means, np.float32).reshape(-1, 3)
    n = means.shape[0]
    rec = np.zeros((n, RECORD_BYTES), np.uint8)
    pre = np.full((n, RECORD_BYTES), np.nan)
    rec[:, 0:12] = means.view(np.uint8).reshape(n, 12)
    with np.errstate(over="ignore"):
        ex = np.exp(np.asarray(scales, np.float64).reshape(n, 3)).astype(np.float32)
    rec[:, 12:24] = np.ascontiguousarray(ex).view(np.uint8).reshape(n, 12)
    with np.errstate(invalid="ignore"):
        rec[:, 24:27], pre[:, 24:27] = _clip_trunc(255.0 * (0.5 + C0 * np.asarray(colors_dc, np.float64).reshape(n, 3)))
        rec[:, 27], pre[:, 27] = _clip_trunc(255.0 * _sigmoid(np.asarray(opacities).reshape(n)))
        q = np.asarray(quats, np.float64).reshape(n, 4)
        norm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        good = np.isfinite(norm) & (norm > 0)
        rot = 128.0 * (q / np.where(good, norm, 1.0)[:, None]) + 128.0
    rot[~good] = (256.0, 128.0, 128.0, 128.0)                           # the identity: 255 128 128 128 after the clip
    rec[:, 28:32], pre[:, 28:32] = _clip_trunc(rot)
    return rec, pre


def exp_scales(scales):
    """float64 exp(scales): what bytes 12..23 round."""
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(scales, np.float64))


def decode(records):
    """uint8 [n,32] -> dict of float64 arrays (means: float32, the bits)."""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, RECORD_BYTES)
    n = rec.shape[0]
    f = np.ascontiguousarray(rec[:, :24]).view(np.float32).reshape(n, 6)
    s = f[:, 3:6].astype(np.float64)
    s = np.where(s > FLT_MIN, s, FLT_MIN)                               # NaN and negatives too
    a = np.clip(rec[:, 27].astype(np.float64), 1.0, 254.0) / 255.0
    return {"means": f[:, :3].copy(), "scales": np.log(s),
            "colors_dc": (rec[:, 24:27].astype(np.float64) / 255.0 - 0.5) / C0,
            "opacities": np.log(a / (1.0 - a)).reshape(n, 1),
            "quats": (rec[:, 28:32].astype(np.float64) - 128.0) / 128.0}


def excused(pre):
    """bool [n,32]: the bytes that may differ by one - the oracle's value before truncation within EPS of an integer."""
    with np.errstate(invalid="ignore"):
        return np.abs(pre - np.round(pre)) <= EPS


def compare_bytes(got, rec, pre, what=""):
    """The byte rule on the eight quantised bytes 24..31 of every record (the float32 fields have bars of their own:
    ``compare_floats``).  Asserts it and returns (flipped bytes, worst distance from an integer among them)."""
    got = np.asarray(got, np.uint8).reshape(rec.shape)[:, 24:]
    rec, pre = rec[:, 24:], pre[:, 24:]
    ok = excused(pre)
    share = ok.mean() if rec.shape[0] else 0.0
    assert share <= MAX_EXCUSED_SHARE, f"{what}: {share:.4%} of the bytes lie within EPS of an integer; pick another seed"
    diff = got.astype(np.int16) - rec.astype(np.int16)
    flipped = diff != 0
    worst = float(np.abs(pre - np.round(pre))[flipped].max()) if flipped.any() else 0.0
    print(f"{what}: {int(flipped.sum())} of {rec.shape[0] * 8} quantised bytes flipped, worst distance from an integer "
          f"{worst:.3e} (eps {EPS:.3e}); excused share {share:.4%}")
    bad = flipped & ~(ok & (np.abs(diff) == 1))
    assert not bad.any(), (f"{what}: {int(bad.sum())} bytes differ outside the rule, first at {np.argwhere(bad)[:5].tolist()}: "
                           f"got {got[bad][:5]}, oracle {rec[bad][:5]}, before truncation {pre[bad][:5]}")
    return int(flipped.sum()), worst


def ulp_distance(got32, want64):
    """|got - want| in units of float32 ulp at |want| (float64 result, inf where only one is non-finite)."""
    got = np.asarray(got32, np.float64)
    want = np.asarray(want64, np.float64)
    w32 = np.abs(want).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = (np.spacing(np.maximum(w32, np.float32(FLT_MIN)))).astype(np.float64)
        d = np.abs(got - want) / ulp
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))
