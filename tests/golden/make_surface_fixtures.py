#!/usr/bin/env python
"""Generates tests/golden/surface_opacity.npz from the REFERENCE's own training script (scripts/train.py).

Runs only in the build container (needs the reference checkout).  ``make_fixtures.load_reference()`` stubs the
reference's third-party imports; the script's own modules that are not needed here (dataset, depth, viewer) are
stubbed too, and scripts/train.py is loaded as a module.  Stored:
  * the command-line defaults of ``arg_parser()`` for the opacity term (train.py:201, :234-236);
  * the steps on which the script's own ``Scheduler`` enables the opacity term (train.py:33-35, :152-159) with
    ``--regularize-opacity`` and its default window, on a list of probe steps;
  * the opacity-entropy block of ``train()`` (train.py:71-75), cut out of the script's source and executed as it
    stands on float32 logits on the CPU: ``loss`` (starting from 0, so it is ``lambda_opacity * L_o``),
    ``loss_opacity`` and ``d loss / d opacities`` from autograd, for two sets of logits: random ones and a set of
    extreme ones (|x| up to 40, where 1 - o rounds to 0 and the +1e-10 terms decide the value).
"""
import importlib.util
import inspect
import sys
import textwrap
from pathlib import Path
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True
import make_fixtures  # noqa: E402

PROBE_STEPS = [1, 2, 100, 6999, 7000, 7001, 7500, 8999, 9000, 9001, 15000]


def load_train_script():
    make_fixtures.load_reference()
    pkg = sys.modules["tinysplat"]
    pkg.GaussianModel, pkg.GaussianRasterizer = MagicMock(), MagicMock()
    for name in ("tinysplat.dataset", "tinysplat.depth", "tinysplat.viewer"):
        sys.modules[name] = MagicMock()
    spec = importlib.util.spec_from_file_location("reference_train", str(make_fixtures.REF / "scripts" / "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def opacity_block(mod):
    """The body of ``if regularize_opacity_schedule(step):`` in train() (train.py:72-75), dedented."""
    lines = inspect.getsource(mod.train).split("\n")
    at = next(i for i, ln in enumerate(lines) if "if regularize_opacity_schedule(step):" in ln)
    body = []
    for ln in lines[at + 1:]:
        body.append(ln)
        if "loss += args.lambda_opacity * loss_opacity" in ln:
            break
    return textwrap.dedent("\n".join(body))


def run_block(block, args, logits):
    x = torch.tensor(logits, dtype=torch.float32).requires_grad_(True)
    env = {"torch": torch, "args": args, "model": SimpleNamespace(opacities=x), "loss": torch.zeros(())}
    exec(block, env)
    env["loss"].backward()
    return env["loss"].detach().numpy(), env["loss_opacity"].detach().numpy(), x.grad.numpy()


def main():
    mod = load_train_script()
    defaults = mod.arg_parser().parse_args([])
    args = mod.arg_parser().parse_args(["--regularize-opacity"])
    sched = mod.Scheduler(args.regularize_opacity, args.regularize_opacity_start, args.regularize_opacity_end)
    out = {"probe_steps": np.array(PROBE_STEPS), "opacity_active": np.array([bool(sched(s)) for s in PROBE_STEPS])}
    for k in ("lambda_opacity", "regularize_opacity_start", "regularize_opacity_end"):
        out["default_" + k] = np.array(getattr(defaults, k))
    out["default_regularize_opacity"] = np.array(bool(defaults.regularize_opacity))
    block = opacity_block(mod)
    g = np.random.default_rng(31)
    cases = {
        "random": (3.0 * g.standard_normal((2000, 1)) + 0.5).astype(np.float32),
        "extreme": np.array([[v] for v in (-40.0, -30.0, -25.0, -20.0, -17.0, -16.0, -10.0, -1e-3, 0.0, 1e-3, 5.0, 10.0,
                                           15.0, 16.0, 17.0, 20.0, 25.0, 30.0, 40.0, 0.5, -0.5)], dtype=np.float32),
    }
    for name, x in cases.items():
        loss, lo, grad = run_block(block, args, x)
        out[f"{name}_opacities"], out[f"{name}_loss"], out[f"{name}_loss_opacity"], out[f"{name}_grad"] = x, loss, lo, grad
    np.savez_compressed(HERE / "surface_opacity.npz", **out)
    print(block)
    print({k: v for k, v in out.items() if k.startswith("default_") or k.endswith("loss_opacity")})


if __name__ == "__main__":
    main()
