"""The opacity-entropy regulariser without a GPU: the float64 oracle against the reference's own training-script
block (tests/golden/surface_opacity.npz, tests/golden/make_surface_fixtures.py), SurfaceConfig's defaults against
the script's arg_parser(), the schedule against its Scheduler, and the argument checks of the new C entries."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import GOLD
from surface_oracle import opacity_entropy_oracle


def _fixture():
    return np.load(GOLD / "surface_opacity.npz")


@pytest.mark.parametrize("case", ["random", "extreme"])
def test_oracle_matches_the_reference_block(case):
    """float32: the reference's numbers bit for bit.  float64: within float32 rounding of them (absolute in the
    gradient: where 1 - o rounds to 0 in float32, sigmoid' is 0 there and ~1e-9 in float64)."""
    z = _fixture()
    x, lam = z[f"{case}_opacities"], float(z["default_lambda_opacity"])
    lo32, grad32 = opacity_entropy_oracle(x, torch.float32, lam)
    assert lo32.numpy() == z[f"{case}_loss_opacity"]
    assert np.array_equal(grad32.numpy(), z[f"{case}_grad"])
    lo, grad = opacity_entropy_oracle(x)
    assert grad.shape == z[f"{case}_grad"].shape
    assert abs(lo.item() - float(z[f"{case}_loss_opacity"])) <= 2e-7 * max(1.0, abs(lo.item()))
    assert abs(lam * lo.item() - float(z[f"{case}_loss"])) <= 2e-7
    ref = z[f"{case}_grad"].astype(np.float64)
    err = np.abs(lam * grad.numpy() - ref)
    assert err.max() <= 1e-5 * np.abs(ref).max(), (err.max(), np.abs(ref).max())


def test_surface_config_defaults_are_the_reference_command_line():
    from tinysplat_amd.surface import SurfaceConfig
    z = _fixture()
    c = SurfaceConfig()
    assert c.regularize_opacity == bool(z["default_regularize_opacity"]) is False
    assert c.lambda_opacity == float(z["default_lambda_opacity"])
    assert c.regularize_opacity_start == int(z["default_regularize_opacity_start"])
    assert c.regularize_opacity_end == int(z["default_regularize_opacity_end"])


def test_schedule_fires_on_the_reference_steps():
    from tinysplat_amd.surface import SurfaceConfig, SurfaceRegularizer
    z = _fixture()
    reg = SurfaceRegularizer(SurfaceConfig(regularize_opacity=True))
    got = [reg.opacity_active(int(s)) for s in z["probe_steps"]]
    assert got == [bool(a) for a in z["opacity_active"]]
    off = SurfaceRegularizer()
    assert not any(off.active(int(s)) for s in z["probe_steps"])
    assert off.terms(None, 7500) == {}                      # nothing active: no term, the model is not touched


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    assert lib.ts_opacity_entropy_ws_bytes(0) == -1
    assert lib.ts_opacity_entropy_ws_bytes(1) >= 8
    assert lib.ts_opacity_entropy_ws_bytes(1_000_000) >= 8 * 256
    buf = ctypes.c_float()
    assert lib.ts_opacity_entropy(0, ctypes.addressof(buf), ctypes.addressof(buf), None, ctypes.addressof(buf),
                                  None) == -1
    assert lib.ts_opacity_entropy(4, None, ctypes.addressof(buf), None, ctypes.addressof(buf), None) == -1
    assert lib.ts_opacity_entropy(4, ctypes.addressof(buf), None, None, ctypes.addressof(buf), None) == -1
    assert lib.ts_opacity_entropy(4, ctypes.addressof(buf), ctypes.addressof(buf), None, None, None) == -1


def test_opacity_entropy_refuses_cpu_tensors():
    from tinysplat_amd.surface import opacity_entropy
    with pytest.raises(RuntimeError):
        opacity_entropy(torch.zeros(4, 1))
