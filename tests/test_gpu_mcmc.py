"""The budgeted densifier on the GPU (tinysplat_amd.mcmc, csrc/mcmc.hip) against the float64 oracle of
tests/mcmc_oracle.py: the relocation arithmetic, the draws, a relocation and a growth step on small models, the noise with
given and with in-kernel normals, the two mean regularisers, and the densifier inside ``TrainStep`` / ``fit``.  Every bound
is derived in the oracle from the number formats; none is fitted to what the kernels give."""
import math

import numpy as np
import pytest
import torch

import mcmc_oracle as MO
from tinysplat_amd.mcmc import (McmcConfig, McmcDensifier, inject_noise, mcmc_normals, mean_opacity, mean_scale, relocation,
                                sample_rows)
from tinysplat_amd.synthetic import SplatModel, make_scene
from tinysplat_amd.training import Adam, TrainStep, fit

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARAMS = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")
GRID_LOGITS = [MO.logit_just_above(MO.MIN_OPACITY)] + \
    [np.float32(math.log(p / (1 - p))) for p in (0.006, 0.1, 0.5, 0.9, 0.995)] + [np.float32(17.0), np.float32(30.0)]


def _gpu(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _model(n, seed, logits=None):
    """n rows on the GPU: make_scene's geometry with un-normalised quaternions; ``logits`` replace the opacities"""
    model, _cam = make_scene(n, 1, 64, 64, seed=seed)
    g = torch.Generator().manual_seed(seed)
    model.quats = model.quats * (0.5 + 2.0 * torch.rand(n, 1, generator=g))
    if logits is not None:
        model.opacities = torch.as_tensor(np.asarray(logits, dtype=np.float32)).reshape(n, 1)
    model = model.to(DEV)
    for nm in PARAMS:
        setattr(model, nm, getattr(model, nm).detach().clone().contiguous())
    return model


def _optim(model, seed):
    """Adam over the model with non-trivial moments and step counts"""
    optim = Adam({nm: getattr(model, nm) for nm in PARAMS})
    g = torch.Generator().manual_seed(seed)
    for k, nm in enumerate(PARAMS):
        optim.exp_avg[nm] = torch.randn(getattr(model, nm).shape, generator=g).to(DEV)
        optim.exp_avg_sq[nm] = torch.rand(getattr(model, nm).shape, generator=g).to(DEV) + 0.1
        optim.steps[nm] = 10 + k
    return optim


def _snapshot(model, optim):
    return ({nm: getattr(model, nm).detach().clone() for nm in PARAMS},
            {nm: optim.exp_avg[nm].clone() for nm in PARAMS}, {nm: optim.exp_avg_sq[nm].clone() for nm in PARAMS},
            dict(optim.steps))


# ------------------------------------------------------------------------------------------------ 1. relocation
def test_relocation_against_the_oracle():
    """4 099 rows (not a multiple of 64), counts 1..60 (the clamp at 51 is crossed), the opacity grid of tests/test_mcmc_cpu.py.

    Tolerance (mcmc_oracle.relocation_tolerances), in float32 roundings of the chain, none fitted:
      opacity  the cast of o' to float32 (EPS relative on p, i.e. EPS / (1 - p) in the logit), the difference 1 - p and the
               quotient (EPS each), the device's logf at its documented 1 ulp of the result;
      scales   the cast of o / D (EPS in its logarithm), logf at 1 ulp of log(o / D), the final add at half an ulp of the
               sum; plus 2e-10 for the two double evaluations of D (worst case; 1e-13 in practice).
    Rows with count 0 keep their bits."""
    n = 4099
    rng = np.random.default_rng(1)
    logits = np.array([GRID_LOGITS[i % len(GRID_LOGITS)] for i in range(n)], np.float32)
    counts = np.array([(i // len(GRID_LOGITS)) % 61 for i in range(n)], np.int32)           # 0..60
    scales = rng.uniform(-6.0, 1.0, (n, 3)).astype(np.float32)
    got_o, got_s = relocation(_gpu(logits).reshape(n, 1), _gpu(scales), _gpu(counts))
    got_o, got_s = got_o.cpu().numpy().reshape(-1).astype(np.float64), got_s.cpu().numpy().astype(np.float64)
    rows = {}
    worst_o = worst_s = 0.0
    for i in range(n):
        if counts[i] == 0:
            assert got_o[i] == logits[i] and np.array_equal(got_s[i], scales[i]), i
            continue
        key = (float(logits[i]), int(counts[i]))
        if key not in rows:
            rows[key] = MO.relocate_row(MO.sigmoid32(logits[i]), counts[i])
        logit, logc, p = rows[key]
        want_s = scales[i].astype(np.float64) + logc
        tol_o, tol_s = MO.relocation_tolerances(logit, logc, p, want_s)
        worst_o, worst_s = max(worst_o, abs(got_o[i] - logit) / tol_o), max(worst_s, (np.abs(got_s[i] - want_s) / tol_s).max())
    print(f"relocation: worst error / tolerance: opacity {worst_o:.3f}, scales {worst_s:.3f}")
    assert worst_o <= 1.0 and worst_s <= 1.0
    assert len(rows) >= 8 * 60 - 8 and max(c for _, c in rows) == 60


# ------------------------------------------------------------------------------------------------ 2. sample_rows
def _exact_weights(n, seed, dead, half=True):
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1 << 9, n).astype(np.float64) * 2.0 ** -20         # every partial sum is exact in any order
    w[dead] = 0.0
    if not half:
        return w
    last = np.flatnonzero(w > 0)[-1]
    w[last] = 0.0
    w[last] = 0.5 - w.sum()                    # the total is 1/2: u = 2 P_i is a float32 and u * total is P_i exactly
    assert w[last] > 0 and w.sum() == 0.5
    return w


def test_sample_rows_equals_searchsorted_on_exact_weights():
    n = 1000
    dead = np.zeros(n, bool)
    dead[[0, 1, 2, 500, 501]] = True                   # dead rows at the front, in the middle
    dead[-7:] = True                                   # and at the end
    w = _exact_weights(n, 5, dead)
    P = np.cumsum(w)
    rng = np.random.default_rng(6)
    on_prefix = (2.0 * P[[10, 400, 499, 2, 990]]).astype(np.float32)       # draws landing exactly on a prefix value
    u = np.concatenate(([0.0, 1.0 - 2.0 ** -24], on_prefix, rng.random(300))).astype(np.float32)
    picks, counts = sample_rows(_gpu(w), _gpu(u))
    want = np.searchsorted(P, u.astype(np.float64) * P[-1], side="right")
    assert np.array_equal(picks.cpu().numpy(), want)
    assert want[0] == 3 and want[1] == n - 8 and list(want[2:7]) == [11, 401, 502, 3, 991]
    assert np.array_equal(counts.cpu().numpy(), np.bincount(want, minlength=n)) and counts.cpu().numpy()[dead].sum() == 0
    assert np.array_equal(MO.sample(w, u)[0], want)                        # the oracle's restated scan agrees
    # one live row takes every draw
    one = np.zeros(77)
    one[40] = 2.0 ** -20
    picks, counts = sample_rows(_gpu(one), _gpu(u))
    assert bool((picks == 40).all()) and int(counts[40]) == len(u) and int(counts.sum()) == len(u)
    # more than one scan workgroup (2 048 rows each): still the running sum on exact weights
    big = _exact_weights(4500, 7, np.arange(4500) % 9 == 4, half=False)
    Pb = np.cumsum(big)
    picks, _ = sample_rows(_gpu(big), _gpu(u))
    assert np.array_equal(picks.cpu().numpy(), np.searchsorted(Pb, u.astype(np.float64) * Pb[-1], side="right"))


# ------------------------------------------------------------------------------------------------ 3. relocate
def _relocation_case(n=601, heavy=300):
    """logits of n rows: a quarter dead (o below 0.0049), the others at 0.006..0.05, and one heavy row at 0.97"""
    rng = np.random.default_rng(11)
    o = rng.uniform(0.006, 0.05, n)
    dead_rows = rng.choice(np.setdiff1d(np.arange(n), [heavy]), n // 4, replace=False)
    o[dead_rows] = rng.uniform(1e-4, 0.0049, len(dead_rows))
    o[heavy] = 0.97
    return np.log(o / (1.0 - o)).astype(np.float32), heavy


def test_relocate_moves_dead_rows_onto_drawn_sources():
    """601 rows, a quarter dead, one source drawn 60 times (M clamps at 51).  With given u: picks and counts are the
    oracle's; sources are rewritten within the relocation tolerances; destinations are bit-identical to their rewritten
    sources; other rows keep their bits; moments are zero on written rows and unchanged elsewhere; steps are unchanged."""
    n = 601
    logits, heavy = _relocation_case(n)
    w, dead = MO.weights(logits)
    assert dead.sum() == n // 4 and not dead[heavy]
    P = MO.scan_prefix(w)
    rng = np.random.default_rng(12)
    u = rng.random(int(dead.sum()))
    u[:60] = (P[heavy - 1] + (np.arange(60) + 0.5) / 60.0 * w[heavy]) / P[-1]          # 60 draws inside the heavy row
    u = u.astype(np.float32)
    want_picks, want_counts = MO.sample(w, u)
    assert want_counts[heavy] >= 60 and want_counts[dead].sum() == 0

    model = _model(n, 3, logits)
    optim = _optim(model, 4)
    before, m0, v0, steps0 = _snapshot(model, optim)
    objects = {nm: getattr(model, nm) for nm in PARAMS}
    d = McmcDensifier(model, McmcConfig())
    moved = d.relocate(optim, _gpu(u))
    assert moved == int(dead.sum()) == d.last_dead
    assert np.array_equal(d.last_picks.cpu().numpy(), want_picks) and np.array_equal(d.last_pick_counts.cpu().numpy(), want_counts)
    assert np.array_equal(d.last_dead_rows.cpu().numpy(), np.flatnonzero(dead))
    assert all(getattr(model, nm) is objects[nm] for nm in PARAMS) and optim.steps == steps0
    after = {nm: getattr(model, nm).detach() for nm in PARAMS}
    dead_t, picked_t = _gpu(dead), _gpu(want_counts > 0)
    written = dead_t | picked_t
    # sources: the oracle's values within the tolerances; their other tensors keep their bits
    got_o = after["opacities"].cpu().numpy().reshape(-1).astype(np.float64)
    got_s = after["scales"].cpu().numpy().astype(np.float64)
    old_s = before["scales"].cpu().numpy().astype(np.float64)
    for i in np.flatnonzero(want_counts > 0):
        logit, logc, p = MO.relocate_row(MO.sigmoid32(logits[i]), want_counts[i])
        tol_o, tol_s = MO.relocation_tolerances(logit, logc, p, old_s[i] + logc)
        assert abs(got_o[i] - logit) <= tol_o and (np.abs(got_s[i] - (old_s[i] + logc)) <= tol_s).all(), i
    for nm in ("means", "colors_dc", "colors_rest", "quats"):
        assert torch.equal(after[nm][picked_t], before[nm][picked_t]), nm
    # destinations: the j-th dead row is a bit copy of the j-th pick
    src = torch.as_tensor(want_picks).to(DEV)
    for nm in PARAMS:
        assert torch.equal(after[nm][dead_t], after[nm][src]), nm
        assert torch.equal(after[nm][~written], before[nm][~written]), nm
        assert not optim.exp_avg[nm][written].any() and not optim.exp_avg_sq[nm][written].any(), nm
        assert torch.equal(optim.exp_avg[nm][~written], m0[nm][~written]), nm
        assert torch.equal(optim.exp_avg_sq[nm][~written], v0[nm][~written]), nm


@pytest.mark.parametrize("case", ["all_dead", "none_dead"])
def test_relocate_changes_nothing_without_dead_or_without_live_rows(case):
    n = 601
    logits = np.full(n, -8.0 if case == "all_dead" else 1.0, np.float32)
    model = _model(n, 5, logits)
    optim = _optim(model, 6)
    before, m0, v0, steps0 = _snapshot(model, optim)
    d = McmcDensifier(model, McmcConfig(cap_max=n))
    assert d.relocate(optim) == 0 and d.last_dead == (n if case == "all_dead" else 0)
    assert d.refine(optim) is False and d.last_counts == (d.last_dead, 0, 0, n)
    for nm in PARAMS:
        assert torch.equal(getattr(model, nm), before[nm]) and torch.equal(optim.exp_avg[nm], m0[nm])
        assert torch.equal(optim.exp_avg_sq[nm], v0[nm])
    assert optim.steps == steps0


# ------------------------------------------------------------------------------------------------ 4. add
def test_add_grows_to_the_cap_and_then_reallocates_nothing():
    n, cap = 1000, 1030
    rng = np.random.default_rng(21)
    logits = rng.normal(0.0, 1.5, n).astype(np.float32)              # every row alive
    model = _model(n, 7, logits)
    optim = _optim(model, 8)
    before, m0, v0, steps0 = _snapshot(model, optim)
    u = rng.random(30).astype(np.float32)
    w, dead = MO.weights(logits, zero_dead=False)
    assert not dead.any()
    want_picks, want_counts = MO.sample(w, u)
    d = McmcDensifier(model, McmcConfig(cap_max=cap))
    assert d.refine(optim, _gpu(u)) is True and d.last_counts == (0, 0, 30, cap)          # 30 rows, not 5 % = 50
    assert np.array_equal(d.last_picks.cpu().numpy(), want_picks)
    picked = _gpu(want_counts > 0)
    src = torch.as_tensor(want_picks).to(DEV)
    for nm in PARAMS:
        p = getattr(model, nm)
        assert p.shape[0] == cap and p.requires_grad == before[nm].requires_grad and optim.params[nm] is p
        assert torch.equal(p[n:], p[src]), nm                                             # appended in draw order
        assert torch.equal(p[:n][~picked], before[nm][~picked]), nm
        assert not optim.exp_avg[nm][n:].any() and not optim.exp_avg_sq[nm][n:].any(), nm
        assert not optim.exp_avg[nm][:n][picked].any() and not optim.exp_avg_sq[nm][:n][picked].any(), nm
        assert torch.equal(optim.exp_avg[nm][:n][~picked], m0[nm][~picked]), nm
        assert torch.equal(optim.exp_avg_sq[nm][:n][~picked], v0[nm][~picked]), nm
    assert optim.steps == steps0
    i = int(np.flatnonzero(want_counts > 0)[0])
    logit, logc, pp = MO.relocate_row(MO.sigmoid32(logits[i]), want_counts[i])
    tol_o, _ = MO.relocation_tolerances(logit, logc, pp, 0.0)
    assert abs(float(model.opacities[i]) - logit) <= tol_o
    # at the cap: nothing is appended and the tensors stay the same objects
    objects = {nm: getattr(model, nm) for nm in PARAMS}
    assert d.refine(optim) is False and d.last_counts[2:] == (0, cap)
    assert all(getattr(model, nm) is objects[nm] for nm in PARAMS)


# ------------------------------------------------------------------------------------------------ 5. noise, given z
def _noise_case(n=5003, seed=31):
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 2.0, (n, 3)).astype(np.float32)
    scales = (np.log(10.0) * rng.uniform(-4.0, 0.0, (n, 3))).astype(np.float32)        # four decades
    quats = (rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.2, 5.0, (n, 1))).astype(np.float32)
    logits = (math.log(0.005 / 0.995) + rng.uniform(-4.0, 1.5, n)).astype(np.float32)   # 1 - o on both sides of the knee
    overflow = np.arange(n) % 7 == 3
    logits[overflow] = np.float32(math.log(0.9 / 0.1))                                  # exponent 89.5: expf overflows
    z = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    return means, scales, quats, logits, z, overflow


def _noise_model(means, scales, quats, logits):
    n = means.shape[0]
    return SplatModel(_gpu(means), torch.zeros(n, 3, device=DEV), torch.zeros(n, 0, 3, device=DEV), _gpu(scales),
                      _gpu(quats), _gpu(logits).reshape(n, 1), 0)


def test_noise_with_given_normals_against_the_oracle():
    """5 003 rows.  Bound per row (mcmc_oracle.noise): (704 + 70 + 2) EPS * scale * g * |Sigma| * |z| + EPS * |result| -
    the gate's 704 EPS is 100 times the seven roundings in front of its exponent, the 70 EPS the rotation and the two
    products, the rest the final product and sum.  Rows whose exponent overflows keep their bits."""
    means, scales, quats, logits, z, overflow = _noise_case()
    scale = 1.6e-4 * 5e5
    want, bound, g = MO.noise(means, scales, quats, logits, scale, z)
    assert (g[~overflow] > 0.55).any() and (g[~overflow] < 0.45).any() and (g[overflow] < 1e-38).all()     # g(1) = 0.62
    model = _noise_model(means, scales, quats, logits)
    inject_noise(model, scale, _gpu(z))
    got = model.means.cpu().numpy()
    assert np.array_equal(got[overflow].view(np.uint32), means[overflow].view(np.uint32))
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    print(f"noise: worst error / bound {float((err / bound).max()):.3f}; moved rows {int((got != means).any(axis=1).sum())}")
    assert (err <= bound).all() and np.isfinite(got).all()
    assert (got != means).any(axis=1)[~overflow].mean() > 0.9
    for nm, a in (("scales", scales), ("quats", quats)):
        assert np.array_equal(getattr(model, nm).cpu().numpy(), a)


# ------------------------------------------------------------------------------------------------ 6. in-kernel draws
def test_in_kernel_normals_are_the_published_ones(tmp_path):
    means, scales, quats, logits, _z, _overflow = _noise_case(n=5003, seed=32)
    seed, step = 0x0123456789ABCDEF, 41
    a, b, c, d = (_noise_model(means, scales, quats, logits) for _ in range(4))
    inject_noise(a, 80.0, None, seed, step)
    inject_noise(b, 80.0, mcmc_normals(5003, seed, step, DEV))
    inject_noise(c, 80.0, None, seed, step)
    inject_noise(d, 80.0, None, seed, step + 1)
    assert torch.equal(a.means, b.means) and torch.equal(a.means, c.means) and not torch.equal(a.means, d.means)
    assert not torch.equal(a.means, _gpu(means))
    # the distribution over 2^20 rows
    rows = 1 << 20
    zs = mcmc_normals(rows, seed, step, DEV)
    assert torch.equal(zs, mcmc_normals(rows, seed, step, DEV)) and torch.equal(zs[:5003], mcmc_normals(5003, seed, step, DEV))
    v = zs.double().reshape(-1)
    count = v.numel()
    mean, var = float(v.mean()), float(v.var())
    print(f"normals: mean {mean:.3e} (bar {5 / math.sqrt(count):.3e}), variance - 1 {var - 1:.3e} (bar {5 * math.sqrt(2 / count):.3e}), "
          f"max |z| {float(v.abs().max()):.4f}")
    assert abs(mean) <= 5.0 / math.sqrt(count) and abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / count)
    assert float(v.abs().max()) < math.sqrt(-2.0 * math.log(2.0 ** -25))
    # against the host build of the same header and the float64 definition: device logf / cosf / sinf, so to their
    # tolerance (the host's own libm is allowed the same again), not bit for bit
    import ctypes
    host = MO.build_host(tmp_path)
    first, cnt = 70_000, 4096
    out = np.zeros((cnt, 3), np.float32)
    host.mc_normals(seed, step, first, cnt, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    got = zs[first:first + cnt].cpu().numpy().astype(np.float64)
    z64, rad = MO.normals(seed, step, range(first, first + cnt))
    tol = MO.normals_tolerance(z64, rad)
    assert (np.abs(got - z64) <= tol).all() and (np.abs(got - out) <= 2.0 * tol).all()


# ------------------------------------------------------------------------------------------------ 7. regularisers
def test_mean_regularisers_against_float64_autograd_and_bitwise_run_to_run():
    """100 003 rows, saturated logits included.  Value: every float32 term within 4 EPS (sigmoid) / 2 EPS (exp) relative,
    summed in double, one cast: 5 EPS relative.  Gradient of mean sigmoid: o within 4 EPS, 1 - o within 5 EPS absolute,
    the two products: 12 EPS / n absolute; of mean exp: expf, the product and the float32 1 / n: 5 EPS relative."""
    n = 100_003
    rng = np.random.default_rng(41)
    logits = rng.normal(0.0, 3.0, (n, 1)).astype(np.float32)
    logits[::1000] = 30.0
    logits[1::1000] = -30.0
    logits[2::1000] = 100.0
    logits[3::1000] = -100.0
    scales = rng.uniform(-8.0, 2.0, (n, 3)).astype(np.float32)
    for fn, x, kind in ((mean_opacity, logits, "sigmoid"), (mean_scale, scales, "exp")):
        want, want_g = MO.mean_terms(x, kind)
        runs = []
        for _ in range(2):
            t = _gpu(x).requires_grad_(True)
            v = fn(t)
            (3.0 * v).backward()
            runs.append((v.detach().clone(), t.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        got, got_g = float(runs[0][0]), runs[0][1].cpu().numpy().astype(np.float64) / 3.0
        assert abs(got - want) <= 5 * MO.EPS * want, kind
        tol = 12 * MO.EPS / x.size if kind == "sigmoid" else 5 * MO.EPS * np.abs(want_g) + 1e-45
        print(f"mean {kind}: value error {abs(got - want) / want:.2e} relative; worst gradient error / tolerance "
              f"{float((np.abs(got_g - want_g) / tol).max()):.3f}")
        assert (np.abs(got_g - want_g) <= tol + 2 * MO.EPS * np.abs(want_g)).all(), kind     # (+ the test's own * 3 / 3)
        assert runs[0][1].shape == t.shape


# ------------------------------------------------------------------------------------------------ 8. integration
def _scene(n=3000, w=160, h=112, seed=5):
    """test_gpu_surface.py's small teacher scene"""
    from tinysplat_amd.rasterizer import GaussianRasterizer
    truth, cam = make_scene(n, 1, w, h, seed=seed, scale_mult=4.0)
    with torch.no_grad():
        tgt, extras = GaussianRasterizer(truth.to(DEV), None, device=torch.device(DEV))(cam, None, 1)
    gen = torch.Generator().manual_seed(seed + 1)
    start, _ = make_scene(n, 1, w, h, seed=seed, scale_mult=4.0)
    start.colors_dc = start.colors_dc + 0.3 * torch.randn(n, 3, generator=gen)
    start.opacities = start.opacities + 0.5 * torch.randn(n, 1, generator=gen)
    return start, cam, tgt.clone(), extras["depth"].clone()


def _fresh(start, rows=None):
    model = start.to(DEV)
    for nm in PARAMS:
        t = getattr(model, nm).detach()
        setattr(model, nm, (t if rows is None else t[:rows]).clone().contiguous())
    return model


def test_an_idle_densifier_leaves_the_fused_step_bitwise():
    start, cam, tgt, tgt_d = _scene()
    runs = []
    for with_densifier in (False, True):
        model = _fresh(start)
        step = TrainStep(model, DEV)
        dens = McmcDensifier(model, McmcConfig(noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0, refine_start=10 ** 9)) \
            if with_densifier else None
        outs = [step(cam, tgt, tgt_d, densifier=dens, step=s) for s in (1, 2, 3)]
        assert step.optimizer.fused_steps == 3
        runs.append((model, step.optimizer, outs))
    (m0, o0, r0), (m1, o1, r1) = runs
    for a, b in zip(r0, r1):
        assert torch.equal(a["loss"], b["loss"]) and "opacity_reg" not in b
    for nm in PARAMS:
        assert torch.equal(getattr(m0, nm), getattr(m1, nm)), nm
        assert torch.equal(o0.exp_avg[nm], o1.exp_avg[nm]) and torch.equal(o0.exp_avg_sq[nm], o1.exp_avg_sq[nm]), nm


def test_fit_grows_to_the_cap_and_stays_there():
    start, cam, tgt, _tgt_d = _scene()
    model = _fresh(start, rows=500)
    cfg = McmcConfig(cap_max=800, refine_start=50, refine_every=25)
    dens = McmcDensifier(model, cfg, generator=torch.Generator().manual_seed(2), seed=9)
    sizes, losses = [], []

    def on_step(step, out):
        sizes.append(model.means.shape[0])
        losses.append(out["loss"])
        assert ("opacity_reg" in out) and ("scale_reg" in out)

    fit(model, [cam], [tgt], DEV, 300, generator=torch.Generator().manual_seed(0), densifier=dens, on_step=on_step)
    losses = [float(v) for v in losses]
    print(f"fit: N {sizes[0]} -> {sizes[-1]}, reached the cap at step {sizes.index(800) + 1}; loss {losses[0]:.5f} -> {losses[-1]:.5f}; "
          f"last refinement {dens.last_counts}")
    assert sizes[0] == 500 and max(sizes) == 800 and sizes[-1] == 800
    at = sizes.index(800)
    assert all(s == 800 for s in sizes[at:]) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(sizes[s - 1] == sizes[s - 2] for s in range(2, 301) if not cfg.fires(s))          # N moves on refinements only
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 9. the shared rebuild
def _launches(fn):
    """-> {C-ABI entry: launches} of one call, recorded by ops.kernel_timer as tests/test_gpu_timer.py does"""
    from tinysplat_amd.ops import kernel_timer
    kernel_timer.start()
    try:
        fn()
    finally:
        table = kernel_timer.stop()
    return {name: count for name, (count, _ms) in table.items()}


@pytest.mark.parametrize("appended", [0, 7])
def test_update_state_is_the_densifiers_without_an_accumulator(appended):
    """601 rows, a third of them dropped, with and without 7 caller-made rows: parameters and both moments are what
    ``Densifier.update_state`` leaves on an identical copy, bit for bit; no Densifier is built or registered, and the
    gather of the gradient accumulator nobody reads is not launched."""
    from tinysplat_amd.densify import Densifier
    n = 601
    g = torch.Generator().manual_seed(51)
    mask = (torch.rand(n, generator=g) < 1.0 / 3.0).to(DEV)
    assert 150 < int(mask.sum()) < 250
    states = []
    for kind in ("densifier", "mcmc"):
        model = _model(n, 13)
        optim = _optim(model, 14)
        g2 = torch.Generator().manual_seed(52)
        rows = {nm: torch.randn((appended,) + tuple(getattr(model, nm).shape[1:]), generator=g2).to(DEV)
                for nm in PARAMS} if appended else None
        steps0 = dict(optim.steps)
        d = Densifier(model) if kind == "densifier" else McmcDensifier(model, McmcConfig())
        got = _launches(lambda: d.update_state(optim, mask, rows))
        assert got == {"ts_densify_plan": 1, "ts_gather_rows": 4 if kind == "densifier" else 3}
        assert optim.steps == steps0 and ("Densifier" in model.held_by) == (kind == "densifier")
        assert all(optim.params[nm] is getattr(model, nm) for nm in PARAMS)
        states.append((model, optim))
    (ma, oa), (mb, ob) = states
    assert mb.means.shape[0] == n - int(mask.sum()) + appended
    for nm in PARAMS:
        assert torch.equal(getattr(ma, nm), getattr(mb, nm)), nm
        assert torch.equal(oa.exp_avg[nm], ob.exp_avg[nm]) and torch.equal(oa.exp_avg_sq[nm], ob.exp_avg_sq[nm]), nm


def test_launch_inventory_of_a_relocation():
    logits, _heavy = _relocation_case()
    model = _model(len(logits), 3, logits)
    optim = _optim(model, 4)
    d = McmcDensifier(model, McmcConfig())
    got = _launches(lambda: d.relocate(optim))
    assert d.last_dead == len(logits) // 4
    assert got == {"ts_mcmc_weights": 1, "ts_densify_plan": 1, "ts_mcmc_sample_rows": 1, "ts_mcmc_rewrite": 1,
                   "ts_mcmc_copy_rows": 1}
