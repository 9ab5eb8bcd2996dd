"""Antialiased rendering on the host: the g++ build of csrc/antialias_math.h against the float64
restatement on covariance triples, the v_conic convention of the injected gradient against plain autograd through the
float64 oracle, and the pose-gradient identity of section 6u on an antialiased frame.  No GPU needed."""
import numpy as np
import pytest
import torch

import antialias_cases as AC
import antialias_oracle as AO
import pose_oracle as PO


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("antialias"))


# ---- 1. the header on triples
def test_header_on_regular_triples_is_within_its_rounding_bound(host):
    """comp and G of the float32 header against the float64 restatement on the same float32 triples (with the header's
    float32 blur), within antialias_cases.rounding_bound: first order in 2^-24, factor 2."""
    triples = AC.regular_triples()
    v = AC.triple_gradients(triples.shape[0])
    comp, G = AC.host_triples(host, triples, v)
    want_G, want_comp = AO.conic_gradient(triples[:, 0], triples[:, 1], triples[:, 2], v, blur=AC.BLUR32)
    b_comp, b_G = AC.rounding_bound(triples, v)
    assert np.isfinite(comp).all() and np.isfinite(G).all()
    assert (want_comp > 0).all() and (want_comp < 1).all() and (comp >= 0).all() and (comp <= 1).all()
    tiny = np.finfo(np.float64).tiny                   # (b = 0: the bound of G1 is 0, and so must the error be)
    r_comp = np.abs(comp - want_comp) / np.maximum(b_comp, tiny)
    r_G = np.abs(G - want_G) / np.maximum(b_G, tiny)
    print(f"{triples.shape[0]} triples: worst error / bound: comp {r_comp.max():.3g}, G {r_G.max():.3g}; "
          f"worst relative error: comp {(np.abs(comp - want_comp) / want_comp).max():.3g}, "
          f"G {(np.abs(G - want_G) / np.abs(want_G).max(axis=1, keepdims=True)).max():.3g}")
    assert (r_comp <= 1.0).all() and (r_G <= 1.0).all()
    # sub-pixel Gaussians keep their covariance: comp of an isotropic a_o = 1e-4 is a_o / (a_o + 0.3) to a few ulps
    assert abs(comp[0] / (1e-4 / (1e-4 + 0.3)) - 1.0) < 1e-6


def test_header_clamps_to_exact_zeros(host):
    """Exactly degenerate triples, a det_o that rounding made negative, indefinite ones: comp = 0 and G = 0 exactly
    (either sign of zero), in the header and in the restatement, whose clamped square root has a zero derivative."""
    triples = AC.clamped_triples()
    v = AC.triple_gradients(triples.shape[0], seed=4)
    comp, G = AC.host_triples(host, triples, v)
    want_G, want_comp = AO.conic_gradient(triples[:, 0], triples[:, 1], triples[:, 2], v, blur=AC.BLUR32)
    assert not np.isnan(comp).any() and not np.isnan(G).any() and not np.isnan(want_G).any()
    assert (comp == 0).all() and (G == 0).all()
    assert (want_comp == 0).all() and (want_G == 0).all()


def test_header_is_nan_free_on_hostile_triples(host):
    """No NaN anywhere: zeros, denormals, huge entries, mixed signs, a zero upstream gradient."""
    g = np.random.default_rng(9)
    vals = np.array([0.0, 1e-45, 1e-38, 1e-20, 1e-4, 0.3, 1.0, 1e3, 1e10, 1e19], dtype=np.float32)
    a, c = np.meshgrid(vals, vals, indexing="ij")
    triples = []
    for k in (0.0, 0.5, 1.0, -1.0, 2.0):
        with np.errstate(over="ignore"):
            b = (k * np.sqrt(a.astype(np.float64) * c.astype(np.float64))).astype(np.float32)
        triples.append(np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1))
    triples = np.concatenate(triples)
    v = g.normal(size=triples.shape[0]).astype(np.float32)
    v[::7] = 0.0
    comp, G = AC.host_triples(host, triples, v)
    assert not np.isnan(comp).any() and not np.isnan(G).any()
    assert (comp >= 0).all() and (comp <= 1).all()
    assert (G[comp == 0] == 0).all()


def test_header_exponential_is_within_two_ulps(host):
    """aa_exp (the header's own exponential, shared bit for bit by host and device) against numpy's float64 exp."""
    x = np.concatenate([np.linspace(-87, 88, 20001), np.array([-100.0, -87.5, 0.0, 1e-8, -40.0])]).astype(np.float32)
    y, sig = np.zeros_like(x), np.zeros_like(x)
    host.ah_exp(x.shape[0], AC._f(x), AC._f(y), AC._f(sig))
    inside = (x >= -87) & (x <= 88)
    want = np.exp(x.astype(np.float64))
    rel = np.abs(y[inside] - want[inside]) / want[inside]
    print(f"aa_exp: worst relative error {rel.max():.3g} ({rel.max() / AC.U / 2:.2f} ulp)")
    assert rel.max() <= 4 * AC.U           # 2 ulps (an ulp is between u and 2 u relative)
    assert (y[x < -87] == 0).all() and y[x == 0][0] == 1.0
    want_s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    assert (np.abs(sig - want_s) <= 6 * AC.U * want_s + 1e-38).all()


# ---- 2. the v_conic convention
def test_injected_conic_gradient_equals_autograd_through_the_oracle():
    """pose_cases' 60 Gaussians at 48 x 32 in float64: the gradients obtained by adding G to the gradient of the oracle's
    conics and running the oracle's own projection backward equal the gradients of plain autograd through
    o_eff = sigmoid(logit) comp, on means, scales, quats and logits, within 1e-10 of each tensor's largest entry
    (float64 rounding over ~1e3 operations; measured 4.5e-16 or less).  Pins v_conic's convention: the true partial of
    the stored off-diagonal entry, 2 G01."""
    scene, view, ref, inj = AC.small_scene_runs()
    assert (ref["radii"] > 0).sum() >= 40 and (ref["radii"] == 0).sum() >= 1
    assert ((ref["comp"] > 0) & (ref["comp"] < 1)).sum() >= 40
    assert abs(ref["loss"] - inj["loss"]) <= 1e-12 * abs(ref["loss"])
    for name in ("means", "scales", "quats", "opacities"):
        scale = np.abs(ref[name]).max()
        err = np.abs(ref[name] - inj[name]).max()
        print(f"{name}: largest entry {scale:.6g}, largest difference {err:.3g} ({err / scale:.3g} relative)")
        assert scale > 0 and err <= 1e-10 * scale
    # the compensation matters on this scene: without the injection the scale gradients are far off
    from pose_cases import oracle_pose_run
    classic = oracle_pose_run(scene, view)
    assert np.abs(classic["v_means"] - ref["means"]).max() > 1e-3 * np.abs(ref["means"]).max()


# ---- 3. the pose identity on antialiased rows
def test_pose_identity_holds_on_an_antialiased_frame():
    """The six sums of section 6u over the antialiased frame's means.grad and quats.grad equal autograd's gradient of the
    view matrix at the same 1e-10: comp depends on the camera only through the rigid view transform."""
    scene, view, ref, _ = AC.small_scene_runs()
    got = PO.pose_gradient(view, scene["means"], scene["quats"], ref["means"], ref["quats"])
    scale = np.abs(ref["pose"]).max()
    err = np.abs(got - ref["pose"]).max()
    print(f"largest component {scale:.6g}, largest difference {err:.3g} ({err / scale:.3g} relative)")
    assert scale > 1.0 and err <= 1e-10 * scale


# ---- the model attribute and what carries it (no GPU: plain tensors)
def _cpu_model(n=5, mode=None):
    from tinysplat_amd.synthetic import SplatModel
    g = torch.Generator().manual_seed(0)
    kw = {} if mode is None else {"rasterize_mode": mode}
    return SplatModel(torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.zeros(n, 0, 3),
                      torch.randn(n, 3, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, 1, generator=g), 0, **kw)


def test_mode_is_validated_and_carried_by_model_builders():
    from tinysplat_amd import ops
    from tinysplat_amd.edit import merge_models
    from tinysplat_amd.semantic import select_gaussians
    assert _cpu_model().rasterize_mode == "classic" and ops.rasterize_mode(_cpu_model()) == "classic"
    with pytest.raises(ValueError):
        _cpu_model(mode="smooth")
    m = _cpu_model(mode="antialiased")
    assert m.to("cpu").rasterize_mode == "antialiased"
    assert select_gaussians(m, torch.tensor([True, False, True, True, False])).rasterize_mode == "antialiased"
    assert merge_models([m, _cpu_model(mode="antialiased")]).rasterize_mode == "antialiased"
    with pytest.raises(ValueError, match="rasterize modes"):
        merge_models([m, _cpu_model()])
    bare = _cpu_model()
    del bare.rasterize_mode                       # a model from before the attribute existed
    assert ops.rasterize_mode(bare) == "classic" and bare.to("cpu").rasterize_mode == "classic"
    assert merge_models([bare, _cpu_model()]).rasterize_mode == "classic"
    bare.rasterize_mode = "bogus"
    with pytest.raises(ValueError):
        ops.rasterize_mode(bare)
