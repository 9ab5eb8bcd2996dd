"""Inputs shared by tests/test_splat_cpu.py and tests/test_gpu_splat.py: seeded random Gaussians, the edge cases of
DESIGN.md section 6k, and the bars the float32 fields are held to."""
import numpy as np

import splat_oracle as SO

U = 2.0 ** -24                    # float32 unit round-off
# exp(scales): HIP documents expf at 1 ulp; the oracle's cast to float32 adds one.  The decoded scales and opacities are
# held to logf's documented 1 ulp plus one as well (the header takes both logarithms in double and rounds once, so they
# sit well inside it)
EXP_ULPS = 2.0
LOG_ULPS = 2.0
# decoded colors_dc, opacities (double expressions rounded once) and quats (exact): the issue's 2 ulp
DECODE_ULPS = 2.0


def random_scene(n, seed):
    """means, scales, colors_dc, opacities, quats as float32 arrays: continuous values, about one colour in twelve
    clipped at either end."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return {"means": f(rng.standard_normal((n, 3)) * 5.0), "scales": f(rng.uniform(-7.0, 0.5, (n, 3))),
            "colors_dc": f(rng.standard_normal((n, 3)) * 1.3), "opacities": f(rng.standard_normal((n, 1)) * 2.5),
            "quats": f(rng.standard_normal((n, 4)))}


def edge_scene():
    """One Gaussian per edge rule; -> (scene, {name: row})."""
    rows, names = [], {}

    def add(name, mean=(0.5, -1.5, 2.5), scale=(-1.0, -2.0, -3.0), dc=(0.1, -0.2, 0.3), opacity=0.25, quat=(0.3, -0.4, 0.5, 0.6)):
        names[name] = len(rows)
        rows.append((mean, scale, dc, opacity, quat))

    nan, inf = float("nan"), float("inf")
    add("plain")
    add("clip_below", dc=(-1.7725, -2.0, -1e30), opacity=-200.0)           # 0.5 + C0 dc <= 0; sigmoid underflows to 0
    add("clip_above", dc=(1.7726, 2.0, 1e30), opacity=200.0)               # above 255; sigmoid = 1 -> 255
    add("inf_color", dc=(inf, -inf, 0.0))
    add("nan_color", dc=(nan, 0.0, nan))
    add("nan_opacity", opacity=nan)
    add("zero_quat", quat=(0.0, 0.0, 0.0, 0.0))
    add("nan_quat", quat=(1.0, nan, 0.0, 0.0))
    add("inf_quat", quat=(inf, 0.0, 0.0, 0.0))
    add("tiny_quat", quat=(0.3e-25, -0.4e-25, 0.5e-25, 0.6e-25))           # squares underflow float32, not double
    add("huge_quat", quat=(0.3e25, -0.4e25, 0.5e25, 0.6e25))               # squares overflow float32, not double
    add("negative_w", quat=(-1.0, 0.0, 0.0, 0.0))                          # w byte 0; no sign is flipped
    add("negative_w_mixed", quat=(-0.7, 0.1, -0.2, 0.3))
    add("identity", quat=(1.0, 0.0, 0.0, 0.0))
    add("huge_scale", scale=(50.0, 40.0, 30.0))                            # exp overflows the key, not the fields
    add("tiny_scale", scale=(-80.0, -70.0, -60.0))                         # the key underflows, the fields do not
    cols = list(zip(*rows))
    f = lambda a, w: np.ascontiguousarray(np.asarray(a, np.float64).reshape(len(rows), w), np.float32)
    with np.errstate(over="ignore"):
        scene = {"means": f(cols[0], 3), "scales": f(cols[1], 3), "colors_dc": f(cols[2], 3), "opacities": f(cols[3], 1),
                 "quats": f(cols[4], 4)}
    return scene, names


def concat(*scenes):
    return {k: np.concatenate([s[k] for s in scenes]) for k in scenes[0]}


def args(scene):
    return [scene[k] for k in ("means", "scales", "colors_dc", "opacities", "quats")]


def decode_edge_records():
    """Records whose decoding has a rule of its own: scale 0, negative, NaN, subnormal, huge; alpha bytes 0, 1, 254, 255;
    colour and rotation bytes 0, 127, 128, 255."""
    rec = np.zeros((6, 32), np.uint8)
    f = rec[:, :24].view(np.float32).reshape(6, 6)
    f[:, :3] = [[1, 2, 3], [-0.0, np.inf, np.nan], [1e-45, -1e38, 3e38], [4, 5, 6], [7, 8, 9], [0, 0, 0]]
    f[:, 3:] = [[0.0, -1.0, np.nan], [1e-45, 1e-38, 1.1754944e-38], [3.4e38, 1.0, 3e38], [0.5, 2.0, 1e-3],
                [1.0000001, 0.99999994, 1.0], [0.1, 0.2, 0.3]]
    rec[:, 24:28] = [[0, 127, 128, 0], [255, 1, 254, 255], [7, 77, 177, 1], [128, 128, 128, 254], [0, 0, 0, 127], [3, 2, 1, 128]]
    rec[:, 28:32] = [[255, 128, 128, 128], [0, 127, 128, 255], [1, 2, 3, 4], [128, 128, 128, 128], [0, 0, 0, 0], [200, 100, 50, 25]]
    return rec


def key_bar(scales, k64):
    """The bar on a float32 key against the float64 oracle's, derived: t1 = fl(s0 + s1) is off by at most U |t1| and
    t2 = fl(t1 + s2) by another U |t2|, so the exponent is off by D <= U (|s0 + s1| + |s0 + s1 + s2|) and the exponential
    by the factor exp(D) ~ 1 + D; expf adds 1 ulp <= 2 U; the sigmoid is expf (2 U, weighted by e / (1 + e) < 1), one sum
    (U) and one correctly rounded quotient (U); the product adds U: 7 U in all, 8 U with the comparison's own rounding
    of the float64 key to float32.  Second-order terms are covered by the factor 1.01."""
    s = np.asarray(scales, np.float64).reshape(-1, 3)
    d = U * (np.abs(s[:, 0] + s[:, 1]) + np.abs(s[:, 0] + s[:, 1] + s[:, 2]))
    return 1.01 * np.abs(k64) * (d + 8 * U)


def check_keys(got32, scales, opacities, what=""):
    """Keys against the oracle under key_bar, where the float64 key is a normal float32 number (an overflowing or
    underflowing key only has to be non-negative or NaN alike)."""
    k64 = SO.keys(scales, opacities)
    got = np.asarray(got32, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(k64)), what
    normal = np.isfinite(k64) & (k64 > 1e-30) & (k64 < 1e30)
    err, bar = np.abs(got - k64)[normal], key_bar(scales, k64)[normal]
    worst = float((err / bar).max()) if err.size else 0.0
    print(f"{what}: keys' worst error over bar {worst:.3f} on {int(normal.sum())} keys")
    assert (err <= bar).all(), (what, worst)
    rest = ~normal & ~np.isnan(k64)
    assert (got[rest] >= 0).all(), what
    return worst


def check_exp_scales(got_records, scales, what=""):
    """Bytes 12..23 against float64 exp within EXP_ULPS float32 ulp; returns the worst."""
    got = np.ascontiguousarray(np.asarray(got_records, np.uint8).reshape(-1, 32)[:, 12:24]).view(np.float32).reshape(-1, 3)
    d = SO.ulp_distance(got, SO.exp_scales(scales).reshape(-1, 3))
    worst = float(d.max()) if d.size else 0.0
    print(f"{what}: exp(scales) worst {worst:.3f} ulp")
    assert worst <= EXP_ULPS, what
    return worst


def check_decoded(got, records, what=""):
    """A decoded model's arrays (dict of numpy float32) against the oracle's decode of the same bytes."""
    want = SO.decode(records)
    n = want["means"].shape[0]
    assert np.array_equal(np.asarray(got["means"]).view(np.uint32).reshape(n, 3), want["means"].view(np.uint32)), what
    worst = {}
    for name, ulps in (("scales", LOG_ULPS), ("colors_dc", DECODE_ULPS), ("opacities", LOG_ULPS), ("quats", DECODE_ULPS)):
        g = np.asarray(got[name], np.float32).reshape(want[name].shape)
        assert np.isfinite(g).all(), (what, name)
        d = SO.ulp_distance(g, want[name])
        worst[name] = float(d.max()) if d.size else 0.0
        assert worst[name] <= ulps, (what, name, worst[name])
    print(f"{what}: decode worst ulp {worst}")
    return worst
