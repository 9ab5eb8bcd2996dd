"""The budgeted densifier without a GPU: properties of the float64 oracle (tests/mcmc_oracle.py), the
host build of csrc/mcmc_math.h (tests/hostmath/mcmc.cpp) against it - relocation values, the published Philox vectors, row
selection - the configuration and its schedule, the C entries' argument checks, and the refusal of CPU tensors."""
import ctypes
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import mcmc_oracle as MO

ROOT = Path(__file__).resolve().parent.parent
F32P, F64P, I32P, U32P = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_uint32))

# the opacity grid of DESIGN section 6r's tests, as logits
GRID_LOGITS = [MO.logit_just_above(MO.MIN_OPACITY)] + \
    [np.float32(math.log(p / (1 - p))) for p in (0.006, 0.1, 0.5, 0.9, 0.995)] + [np.float32(17.0), np.float32(30.0)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """g++ build of tests/hostmath/mcmc.cpp: the kernels' header compiled for the host."""
    return MO.build_host(tmp_path_factory.mktemp("mcmc"))


def _p(a, t):
    return a.ctypes.data_as(t)


def _adjacent(got, want64):
    """got (float32) is the float64 value rounded to float32, or a neighbour of it"""
    want = np.float32(want64)
    return got == want or got == np.nextafter(want, np.float32(np.inf)) or got == np.nextafter(want, np.float32(-np.inf))


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_properties():
    for x in GRID_LOGITS:
        o = MO.capped(MO.sigmoid32(x))
        last = 2.0
        for M in range(1, 52):
            op = MO.new_opacity(o, M)
            assert abs((1.0 - (1.0 - op) ** M) - o) <= 1e-12, (o, M)
            c = MO.coeff(o, M)
            assert c < last, (o, M)                        # decreases in M
            last = c
        assert MO.coeff(o, 1) == 1.0
    # a float32 sigmoid that rounds to 1 counts as 1 - 2^-24: the same row as sigmoid(17)
    assert MO.sigmoid32(17.0) == np.float32(1.0 - 2.0 ** -24) and MO.sigmoid32(30.0) == 1.0
    assert MO.coeff(1.0, 51) == MO.coeff(np.float32(1.0 - 2.0 ** -24), 51) and MO.new_opacity(1.0, 51) < 0.28
    assert MO.sigmoid32(GRID_LOGITS[0]) > np.float32(MO.MIN_OPACITY) >= MO.sigmoid32(np.nextafter(GRID_LOGITS[0], np.float32(-9)))


def test_the_float64_series_against_80_digit_arithmetic():
    """The float64 sums of D are good to 1e-12 on the whole grid at the M where its terms are largest: the yardstick is
    itself measured before anything is held to it."""
    for x in GRID_LOGITS:
        o = MO.sigmoid32(x)
        for M in (2, 17, 51):
            want = MO.coeff_decimal(o, M)
            assert abs(MO.coeff(o, M) - want) <= 1e-12 * want, (o, M)


def test_oracle_prefix_is_the_running_sum_on_exact_weights():
    rng = np.random.default_rng(3)
    for n in (1, 7, 2048, 2049, 5000):
        w = rng.integers(0, 1 << 20, n).astype(np.float64) * 2.0 ** -20
        assert np.array_equal(MO.scan_prefix(w), np.cumsum(w)), n


# ------------------------------------------------------------------------------------------------ the host build
def test_binomials_are_exact(host):
    assert host.mc_n_max() == MO.N_MAX == 51
    for n in range(51):
        for k in range(51):
            assert host.mc_binom(n, k) == math.comb(n, k), (n, k)


def test_relocation_values_against_the_oracle(host):
    p, c = np.zeros(1, np.float32), np.zeros(1, np.float32)
    for x in GRID_LOGITS:
        o = MO.sigmoid32(x)
        assert host.mc_sigmoid(x) == o
        for M in range(2, 52):
            host.mc_relocate_values(o, M, _p(p, F32P), _p(c, F32P))
            assert _adjacent(p[0], MO.new_opacity(o, M)), (o, M, p[0])
            assert _adjacent(c[0], MO.coeff(o, M)), (o, M, c[0])
    # the whole row, logarithms included: the host's logf is within an ulp
    lg, lc = np.zeros(1, np.float32), np.zeros(1, np.float32)
    for x in GRID_LOGITS:
        o = MO.sigmoid32(x)
        for count in (1, 7, 50, 60):
            host.mc_relocate(o, count, np.float32(MO.MIN_OPACITY), _p(lg, F32P), _p(lc, F32P))
            logit, logc, pp = MO.relocate_row(o, count)
            tol_o, tol_s = MO.relocation_tolerances(logit, logc, pp, logc)
            assert abs(float(lg[0]) - logit) <= tol_o and abs(float(lc[0]) - logc) <= tol_s, (o, count)
    host.mc_relocate(np.float32(0.3), 0, np.float32(MO.MIN_OPACITY), _p(lg, F32P), _p(lc, F32P))
    assert lc[0] == 0.0                                                      # M = 1: the scale stays


def test_philox_published_vectors(host):
    cases = [([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        host.mc_philox(_p(c, U32P), _p(k, U32P), _p(out, U32P))
        assert " ".join("%08x" % v for v in out) == want
        assert " ".join("%08x" % v for v in MO.philox4x32_10(ctr, key)) == want


def test_host_normals_follow_the_definition(host):
    assert host.mc_uniform(0) == np.float32(2.0 ** -25) and host.mc_uniform(0xFFFFFFFF) <= 1.0
    for x in (0, 0x100, 0x7FFFFF00, 0xDEADBEEF, 0xFFFFFFFF):
        assert host.mc_uniform(x) == MO.uniform32(x)
    out = np.zeros((64, 3), np.float32)
    host.mc_normals(0x1234567890ABCDEF, 7, 1000, 64, _p(out, F32P))
    z, rad = MO.normals(0x1234567890ABCDEF, 7, range(1000, 1064))
    assert (np.abs(out - z) <= MO.normals_tolerance(z, rad)).all()
    again = np.zeros((64, 3), np.float32)
    host.mc_normals(0x1234567890ABCDEF, 8, 1000, 64, _p(again, F32P))
    assert not np.array_equal(out, again)


def _exact_weights(n, seed, dead):
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1 << 9, n).astype(np.float64) * 2.0 ** -20         # every partial sum is exact in any order
    w[dead] = 0.0
    last = np.flatnonzero(w > 0)[-1]
    w[last] = 0.0
    w[last] = 0.5 - w.sum()                    # the total is 1/2: u = 2 P_i is a float32 and u * total is P_i exactly
    assert w[last] > 0 and w.sum() == 0.5
    return w


def test_row_selection_on_the_host_function(host):
    n = 1000
    dead = np.zeros(n, bool)
    dead[[0, 1, 2, 500, 501]] = True
    dead[-7:] = True
    w = _exact_weights(n, 5, dead)
    P = np.cumsum(w)
    live = np.flatnonzero(w > 0)
    u = np.array([0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 2.0 * P[400], 2.0 * P[499], 2.0 * P[10]], np.float32)
    assert np.array_equal(u[4:].astype(np.float64) * P[-1], P[[400, 499, 10]])     # draws landing exactly on a prefix value
    picks = np.zeros(len(u), np.int32)
    host.mc_sample(n, len(u), _p(P, F64P), _p(w, F64P), _p(u, F32P), _p(picks, I32P))
    want = np.searchsorted(P, u.astype(np.float64) * P[-1], side="right")
    assert np.array_equal(picks, want)
    assert picks[0] == live[0] == 3 and picks[1] == live[-1] == n - 8 and list(picks[4:]) == [401, 502, 11]
    # a target exactly on a prefix value picks the NEXT live row (first P > target), across a run of dead rows too
    for i in (10, 499, 400):
        r = host.mc_pick(n, _p(P, F64P), _p(w, F64P), P[i])
        assert r == live[np.searchsorted(live, i, side="right")] == np.searchsorted(P, P[i], side="right"), i
        assert MO.pick(P, w, P[i]) == r
    assert host.mc_pick(n, _p(P, F64P), _p(w, F64P), P[499]) == 502
    # no row exceeds the target (rounding): the last row of positive weight
    assert host.mc_pick(n, _p(P, F64P), _p(w, F64P), P[-1]) == n - 8 == MO.pick(P, w, P[-1])
    # a single live row takes every draw; no live row: -1
    one = np.zeros(50)
    one[17] = 2.0 ** -20
    P1 = np.cumsum(one)
    for t in (0.0, 2.0 ** -21, (1.0 - 2.0 ** -24) * 2.0 ** -20, 2.0 ** -20):
        assert host.mc_pick(50, _p(P1, F64P), _p(one, F64P), t) == 17 == MO.pick(P1, one, t)
    none = np.zeros(5)
    assert host.mc_pick(5, _p(none, F64P), _p(none, F64P), 0.0) == -1 == MO.pick(none, none, 0.0)
    # the oracle's own draw on the same weights
    picks_o, counts_o = MO.sample(w, u)
    assert np.array_equal(picks_o, want) and counts_o.sum() == len(u) and counts_o[dead].sum() == 0


def test_gate_is_exactly_zero_where_the_exponent_overflows(host):
    assert host.mc_gate(np.float32(0.9)) == 0.0 and host.mc_gate(np.float32(1.0)) == 0.0
    assert 0.0 < host.mc_gate(np.float32(0.006)) < 0.5 < host.mc_gate(np.float32(0.001)) < 1.0
    assert abs(host.mc_gate(np.float32(0.004)) - MO.gate(np.float32(0.004))) <= 704 * MO.EPS * MO.gate(np.float32(0.004))
    q = np.array([0.3, -1.2, 0.4, 2.0], np.float32)
    s = np.array([-3.0, -1.0, -2.0], np.float32)
    z = np.array([0.5, -1.5, 0.25], np.float32)
    d = np.zeros(3, np.float32)
    host.mc_sigma_z(_p(q, F32P), _p(s, F32P), _p(z, F32P), _p(d, F32P))
    new, _bound, _g = MO.noise(np.zeros((1, 3)), s[None], q[None], np.array([-20.0]), 1.0, z[None])
    g = MO.gate(1.0 / (1.0 + math.exp(20.0)))
    assert np.abs(d - new[0] / g).max() <= 70 * MO.EPS * math.exp(-2.0) * np.linalg.norm(z)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_defaults_and_schedule():
    from tinysplat_amd.mcmc import ExponentialLr, McmcConfig
    c = McmcConfig()
    assert (c.cap_max, c.noise_lr, c.min_opacity, c.opacity_reg, c.scale_reg) == (1_000_000, 5e5, 0.005, 0.01, 0.01)
    assert (c.refine_start, c.refine_stop, c.refine_every) == (500, 25_000, 100)
    fired = [s for s in range(1, 26_000) if c.fires(s)]
    assert fired[0] == 600 and fired[-1] == 24_900 and len(fired) == 244 and all(s % 100 == 0 for s in fired)
    assert not c.fires(500) and not c.fires(25_000) and not c.fires(650)
    c2 = McmcConfig(refine_start=50, refine_every=25, refine_stop=10 ** 9)
    assert [s for s in range(1, 130) if c2.fires(s)] == [75, 100, 125]
    lr = ExponentialLr(1.6e-4, 1.6e-6, 1000)
    assert lr(0)["means"] == pytest.approx(1.6e-4) and lr(1000)["means"] == pytest.approx(1.6e-6)
    assert lr(500)["means"] == pytest.approx(1.6e-5) and lr(5000)["means"] == pytest.approx(1.6e-6)
    with pytest.raises(ValueError):
        ExponentialLr(0.0, 1e-6, 10)


def test_fit_takes_an_lr_schedule_that_is_off_by_default():
    import inspect
    from tinysplat_amd.training import fit
    assert inspect.signature(fit).parameters["lr_schedule"].default is None


def test_train_tool_strategy_flags():
    spec = importlib.util.spec_from_file_location("train_tool_mcmc", ROOT / "tools" / "train.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    s = tool.parse_strategy([])
    assert vars(s) == {"strategy": "reference", "max_gaussians": 1_000_000, "means_lr_final": None}
    argv = ["--strategy", "mcmc", "--max-gaussians", "250000", "--means-lr-final", "1.6e-6", "--max-iter", "3"]
    s = tool.parse_strategy(argv)
    assert (s.strategy, s.max_gaussians, s.means_lr_final) == ("mcmc", 250000, 1.6e-6)
    assert tool.parse(argv).max_iter == 3 and not hasattr(tool.parse(argv), "strategy")
    for bad in (["--strategy", "adc"], ["--max-gaussians", "0"], ["--means-lr-final", "0"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)


def test_every_new_entry_refuses_null_and_non_positive_arguments():
    from tinysplat_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_float * 16)()
    p = ctypes.cast(one, ctypes.c_void_p)
    assert lib.ts_mcmc_noise(0, p, p, p, p, 1.0, None, 0, 0, None) == -1
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert lib.ts_mcmc_noise(4, *args, 1.0, None, 0, 0, None) == -1
    assert lib.ts_mcmc_noise(1, p, p, ctypes.c_void_p(p.value + 4), p, 1.0, None, 0, 0, None) == -1   # quats misaligned
    assert lib.ts_mcmc_normals(0, 0, 0, p, None) == -1 and lib.ts_mcmc_normals(4, 0, 0, None, None) == -1
    assert lib.ts_mcmc_mean_ws_bytes(0) == -1 and lib.ts_mcmc_mean_ws_bytes(1) >= 8
    assert lib.ts_mcmc_mean_ws_bytes(10 ** 10) == lib.ts_mcmc_mean_ws_bytes(10 ** 9)                # capped grid
    assert lib.ts_mcmc_mean(0, 0, p, p, p, p, None) == -1 and lib.ts_mcmc_mean(2, 4, p, p, p, p, None) == -1
    assert lib.ts_mcmc_mean(0, 4, None, p, p, p, None) == -1 and lib.ts_mcmc_mean(0, 4, p, None, p, p, None) == -1
    assert lib.ts_mcmc_mean(1, 4, p, p, p, None, None) == -1
    assert lib.ts_mcmc_weights(0, p, 0.005, 1, p, None, None) == -1 and lib.ts_mcmc_weights(4, None, 0.005, 1, p, None, None) == -1
    assert lib.ts_mcmc_weights(4, p, 0.005, 1, None, None, None) == -1 and lib.ts_mcmc_weights(4, p, -1.0, 1, p, None, None) == -1
    assert lib.ts_mcmc_weights(4, p, float("nan"), 1, p, None, None) == -1
    assert lib.ts_mcmc_sample_ws_bytes(0) == -1 and lib.ts_mcmc_sample_ws_bytes(5000) >= 5000 * 8 + 3 * 8
    assert lib.ts_mcmc_sample_rows(0, 1, p, p, p, p, p, None) == -1 and lib.ts_mcmc_sample_rows(4, 0, p, p, p, p, p, None) == -1
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert lib.ts_mcmc_sample_rows(4, 2, *args, None) == -1
    assert lib.ts_mcmc_rewrite(0, p, 0.005, p, p, 0, None, None, None, None) == -1
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert lib.ts_mcmc_rewrite(4, args[0], 0.005, args[1], args[2], 0, None, None, None, None) == -1
    assert lib.ts_mcmc_rewrite(4, p, 0.005, p, p, 1, None, None, None, None) == -1           # a moment table is missing
    assert lib.ts_mcmc_rewrite(4, p, 0.005, p, p, 9, None, None, None, None) == -1
    tab, wid = (ctypes.c_void_p * 1)(p.value), (ctypes.c_int32 * 1)(3)
    none = (ctypes.c_void_p * 1)(None)
    assert lib.ts_mcmc_rewrite(4, p, 0.005, p, p, 1, tab, none, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(0, 1, p, p, 1, tab, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 0, p, p, 1, tab, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, None, p, 1, tab, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, p, None, 1, tab, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, p, p, 0, tab, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, p, p, 1, None, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, p, p, 1, none, None, None, wid, None) == -1
    assert lib.ts_mcmc_copy_rows(4, 1, p, p, 1, tab, tab, None, wid, None) == -1             # one moment table without the other


def test_cpu_tensors_raise():
    import tinysplat_amd as ts
    from tinysplat_amd.synthetic import make_scene
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.sample_rows(torch.ones(4, dtype=torch.float64), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.relocation(torch.zeros(4, 1), torch.zeros(4, 3), torch.ones(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.mean_opacity(torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.mean_scale(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.mcmc_normals(4, 0, 0, "cpu")
    model, _cam = make_scene(32, 1, 32, 32, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.inject_noise(model, 1.0)
    d = ts.McmcDensifier(model, ts.McmcConfig(noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0))
    assert "McmcDensifier" in model.held_by and d.loss_terms(model, 1) == {} and d.update_grad_accum(1, None) is None
