"""The SuGaR density regulariser without a GPU: the torch restatement (tests/density_oracle.py) against the reference's
own code (tests/golden/surface_density.npz), the configuration defaults, the update and prune rules, and the C-ABI
argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from density_oracle import density_oracle, exact_knn, inverse_cdf, sample_transform
from helpers import GOLD

CASES = ("wide", "tiny")
PARAMS = ("means", "scales", "quats", "opacities")


def _z():
    return np.load(GOLD / "surface_density.npz")


def _close(a, b, rel):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape
    scale = max(b.abs().max().item(), 1e-30)
    assert (a - b).abs().max().item() <= rel * scale, ((a - b).abs().max().item(), scale)


@pytest.mark.parametrize("case", CASES)
def test_sampling_transform_and_neighbours_match_the_reference(case):
    z = _z()
    c = case + "_"
    pts = sample_transform(torch.from_numpy(z[c + "means"]), torch.from_numpy(z[c + "scales"]),
                           torch.from_numpy(z[c + "quats"]), z[c + "rows"], torch.from_numpy(z[c + "normals"]))
    _close(pts, z[c + "points"], 1e-6)
    assert np.array_equal(exact_knn(pts, torch.from_numpy(z[c + "means"])).numpy(), z[c + "knn"])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype,rel", [(torch.float32, 1e-5), (torch.float64, 1e-3)])
def test_oracle_reproduces_the_reference(case, dtype, rel):
    z = _z()
    c = case + "_"
    params = {k: z[c + k] for k in PARAMS}
    r = density_oracle(params, z[c + "depth"], z[c + "view_matrix"], z[c + "proj_matrix"], z[c + "rows"],
                       z[c + "normals"], z[c + "knn"], dtype=dtype)
    assert np.array_equal(r["mask"].numpy(), z[c + "mask"])
    assert abs(r["loss"].item() - float(z[c + "loss"])) <= rel * abs(float(z[c + "loss"]))
    _close(r["density"], z[c + "density"], rel)
    _close(r["approx"][r["mask"]], z[c + "approx"], rel)
    for k in PARAMS + ("depth",):
        _close(r["grads"][k], z[c + "grad_" + k], rel)


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_frozen_graph_step(case):
    """The second, non-update step: current parameters for d and beta, the points and their backward frozen."""
    z = _z()
    c = case + "_"
    r = density_oracle({k: z[c + "step2_" + k] for k in PARAMS}, z[c + "depth"], z[c + "view_matrix"],
                       z[c + "proj_matrix"], z[c + "rows"], z[c + "normals"], z[c + "knn"], dtype=torch.float32,
                       sample_params={k: z[c + k] for k in ("means", "scales", "quats")})
    assert np.array_equal(r["mask"].numpy(), z[c + "step2_mask"])
    assert abs(r["loss"].item() - float(z[c + "step2_loss"])) <= 1e-5 * abs(float(z[c + "step2_loss"]))
    for k in PARAMS + ("depth",):
        _close(r["grads"][k], z[c + "step2_grad_" + k], 1e-5)


def test_tiny_case_exercises_the_grid_and_bilinear_gradients():
    """The fixture is only a check of the depth path if reference-mode grid coordinates land inside the image."""
    z = _z()
    g = z["tiny_grad_depth"]
    assert int(z["tiny_mask"].sum()) > 100
    assert np.count_nonzero(g) > 20 and np.count_nonzero(g[1:-1, 1:-1]) > 20


def test_inverse_cdf_follows_the_weights():
    scales = torch.log(torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 2.0], [1.0, 1.0, 1.0]]))
    # areas 1, 2, 1: cumulative weights 1, 3, 4 (total 8); plain weights 1, 2, 1 (total 4)
    u = torch.tensor([0.0, 0.124, 0.126, 0.49, 0.51, 0.99])
    assert inverse_cdf(scales, u, "reference").tolist() == [0, 0, 1, 1, 2, 2]
    assert inverse_cdf(scales, u, "area").tolist() == [0, 0, 0, 1, 1, 2]


def test_config_defaults_are_the_reference_command_line():
    from tinysplat_amd.surface import SurfaceConfig
    z = _z()
    c = SurfaceConfig()
    assert c.regularize_density == bool(z["default_regularize_density"]) is False
    assert c.lambda_density == float(z["default_lambda_density"])
    assert c.regularize_density_start == int(z["default_regularize_density_start"])
    assert c.regularize_density_end == int(z["default_regularize_density_end"])
    assert c.density_interval == int(z["default_interval_densify"])
    assert c.density_samples == 100_000
    assert (c.density_projection, c.density_sample_weights, c.density_prune_ungated) == ("reference", "reference", False)
    assert not hasattr(c, "regularize_sdf")
    with pytest.raises(ValueError):
        SurfaceConfig(density_projection="ndc")
    with pytest.raises(ValueError):
        SurfaceConfig(density_sample_weights="uniform")


@pytest.mark.parametrize("flag", [False, True])
def test_update_and_prune_rules_match_the_reference(flag):
    from tinysplat_amd.surface import SurfaceConfig, SurfaceRegularizer
    z = _z()
    steps = [int(s) for s in z["probe_steps"]]
    reg = SurfaceRegularizer(SurfaceConfig(regularize_density=flag))
    assert [reg.density_active(s) for s in steps] == z[f"active_{int(flag)}"].tolist()
    assert [reg.density_active(s) and reg.density_update(s) for s in steps] == z[f"update_{int(flag)}"].tolist()
    # the reference prunes at the window's start even with the term off: density_prune_ungated reproduces that
    ungated = SurfaceRegularizer(SurfaceConfig(regularize_density=flag, density_prune_ungated=True))
    assert [ungated.prune_due(s) for s in steps] == z[f"prune_{int(flag)}"].tolist()
    if flag:
        assert [reg.prune_due(s) for s in steps] == z["prune_1"].tolist()
    else:
        assert not any(reg.prune_due(s) for s in steps)
    assert not reg.frame_terms(None, 100, None, None) and reg.terms(None, 9500) == {}


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    bad = -1
    p = ctypes.c_void_p(16)
    cam = (ctypes.c_float * 32)()
    assert lib.ts_density_sample_ws_bytes(0) == bad
    assert lib.ts_density_loss_ws_bytes(0) == bad
    assert lib.ts_segment_sum_ws_bytes(0, 1) == bad and lib.ts_segment_sum_ws_bytes(10, 3) == bad
    assert lib.ts_density_sample_ws_bytes(100) > 0 and lib.ts_segment_sum_ws_bytes(10, 11) > 0
    # n < 1; bad weights; no uniforms and no rows; NULL means
    assert lib.ts_density_sample(0, 4, 0, p, p, p, p, None, p, p, p, p, p, None) == bad
    assert lib.ts_density_sample(20, 4, 2, p, p, p, p, None, p, p, p, p, p, None) == bad
    assert lib.ts_density_sample(20, 4, 0, p, p, p, None, None, p, p, p, p, p, None) == bad
    assert lib.ts_density_sample(20, 4, 0, None, p, p, p, None, p, p, p, p, p, None) == bad
    args = [20, 8, p, p, p, p, p, p, p, p, 48, 64, p, cam, 0, 0.001, p, None, None, None, None, None, None, None, p,
            None]
    for i, v in ((0, 15), (1, 0), (10, 0), (11, 0), (10, 65536), (14, 2), (2, None), (13, None), (16, None),
                 (17, p), (20, p)):
        a = list(args)
        a[i] = v
        if i == 10 and v == 65536:
            a[11] = 65536                            # H * W >= 2^31
        assert lib.ts_density_loss(*a) == bad, (i, v)
    assert lib.ts_segment_sum(0, 1, 4, p, p, p, p, p, p, None) == bad
    assert lib.ts_segment_sum(8, 2, 4, p, p, p, p, p, p, None) == bad
    assert lib.ts_segment_sum(8, 1, 0, p, p, p, p, p, p, None) == bad
    assert lib.ts_segment_sum(8, 1, 4, p, None, p, p, p, p, None) == bad
    assert lib.ts_abi_version() == 9


def test_density_entries_refuse_cpu_tensors_and_small_models():
    from tinysplat_amd.surface import sample_points
    from tinysplat_amd.synthetic import make_scene
    model, _ = make_scene(40, 0, 32, 32, seed=1)
    with pytest.raises(RuntimeError):
        sample_points(model, 8)
    small, _ = make_scene(15, 0, 32, 32, seed=1)
    with pytest.raises((ValueError, RuntimeError)):
        sample_points(small, 8)
