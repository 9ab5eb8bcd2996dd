"""The per-view appearance model without a GPU: the float64 oracle against torch's grid_sample, the
host build of csrc/appearance_math.h against the oracle at the derived bounds, the exact cases (identity and constant
grids), the total variation, the affine colour fit's solve, the configuration, the tools' parsers and the C entries'
argument checks."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import appearance_cases as AC
import appearance_oracle as AO
import tinysplat_amd.appearance as AP
from tinysplat_amd import metrics as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return AC.build_host(tmp_path_factory.mktemp("appearance_host"))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", str(ROOT / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------ the oracle
def _grid_sample_reference(image, grid, v_out):
    """The same function through torch.nn.functional.grid_sample (5-D, align_corners=True, padding_mode="border") in
    float64 with autograd.  The sample positions are the oracle's float32 coordinates (the definition's); the luminance
    coordinate carries the gradient of the float64 luminance, so that autograd sees the slope (L - 1) lum_k."""
    H, W, _ = image.shape
    L, Gh, Gw, _ = grid.shape
    i0, _, tx = AO.axis(W, Gw)
    j0, _, ty = AO.axis(H, Gh)
    img = torch.tensor(image, dtype=torch.float64, requires_grad=True)
    G = torch.tensor(grid, dtype=torch.float64, requires_grad=True)
    w32 = torch.tensor(AO.level(image, L)["w"].astype(np.float64))
    lum = torch.tensor([float(v) for v in AO.LUM], dtype=torch.float64)
    gray = (img * lum).sum(dim=2)
    wz = w32 + (gray - gray.detach()) * (L - 1)                      # the float32 value, the float64 slope

    def norm(index, size):
        return 2.0 * index / (size - 1) - 1.0 if size > 1 else torch.zeros_like(index)
    gx = norm(torch.tensor(i0 + tx.astype(np.float64)), Gw)[None, :].expand(H, W)
    gy = norm(torch.tensor(j0 + ty.astype(np.float64)), Gh)[:, None].expand(H, W)
    gz = norm(wz, L)
    coords = torch.stack([gx, gy, gz], dim=2)[None, None]             # [1, 1, H, W, 3]
    vol = G.permute(3, 0, 1, 2)[None]                                 # [1, 12, L, Gh, Gw]
    A = torch.nn.functional.grid_sample(vol, coords, mode="bilinear", padding_mode="border", align_corners=True)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    x = torch.cat([img, torch.ones(H, W, 1, dtype=torch.float64)], dim=2)
    out = (A * x[:, :, None, :]).sum(dim=3)
    out.backward(torch.tensor(v_out, dtype=torch.float64))
    return out.detach().numpy(), img.grad.numpy(), G.grad.numpy()


@pytest.mark.parametrize("h,w,grid", AC.CASES, ids=AC.IDS)
def test_oracle_against_grid_sample(h, w, grid):
    image, G, v_out = AC.inputs(h, w, grid)
    ref = AC.reference(h, w, grid)
    out, v_image, v_grid = _grid_sample_reference(image, G, v_out)
    # both sides are float64 evaluations of one function from the same float32 coordinates; grid_sample recovers the
    # fractions from normalised coordinates (a few 2^-53 of the coordinate, up to 15): 1e-11 of the sum of |terms|
    for name, got in (("out", out), ("v_image", v_image), ("v_grid", v_grid)):
        err = float(np.max(np.abs(got - ref[name]) / (ref[name + "_abs"] + 1e-300)))
        print(f"{name}: max |difference| / sum|terms| = {err:.2e}")
        assert err < 1e-11, name


# --------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("h,w,grid", AC.CASES, ids=AC.IDS)
def test_host_build_against_the_oracle(host, h, w, grid):
    image, G, v_out = AC.inputs(h, w, grid)
    ref = AC.reference(h, w, grid)
    out = AC.host_forward(host, image, G)
    v_image, v_grid = AC.host_backward(host, image, G, v_out)
    AC.check_against_oracle(ref, out=out, v_image=v_image, v_grid=v_grid)
    # with these inputs only planted pixels sit on a luminance-cell boundary
    planted = {(y, x) for y, x, _ in AC.PLANTED}
    assert {(int(y), int(x)) for y, x in zip(*np.nonzero(~ref["compare"]))} <= planted


def test_coordinates_are_the_oracles(host):
    i0, i1, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    for P, G in ((53, 16), (37, 16), (480, 16), (53, 1), (53, 3), (5, 9), (1, 2)):
        want = AO.axis(P, G)
        for p in range(P):
            host.ah_axis(p, P, G, ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(t))
            assert (i0.value, i1.value) == (want[0][p], want[1][p]) and np.float32(t.value) == want[2][p], (P, G, p)
            assert 0 <= i0.value <= i1.value < G
    l0, l1, inside = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    pixels = np.array([[0, 0, 0], [1, 1, 1], [-0.1, 0.0, 0.0], [40, -25, 7], [0.5, 0.25, 0.125], [np.nan, 0, 0],
                       [np.inf, 0, 0]], np.float32)
    for L in (1, 2, 8):
        want = AO.level(pixels[None], L)
        for k, (r, g, b) in enumerate(pixels):
            host.ah_level(r, g, b, L, ctypes.byref(l0), ctypes.byref(l1), ctypes.byref(t), ctypes.byref(inside))
            assert (l0.value, l1.value, bool(inside.value)) == (want["l0"][0, k], want["l1"][0, k], bool(want["inside"][0, k]))
            assert np.float32(t.value) == want["t"][0, k] and 0 <= l0.value <= l1.value < L
    host.ah_level(np.nan, 0.0, 0.0, 8, ctypes.byref(l0), ctypes.byref(l1), ctypes.byref(t), ctypes.byref(inside))
    assert (l0.value, t.value, inside.value) == (0, 0.0, 0)          # a NaN luminance is clamped to level 0


@pytest.mark.parametrize("h,w,grid", AC.CASES, ids=AC.IDS)
def test_identity_and_constant_grids_are_exact(host, h, w, grid):
    image, _, v_out = AC.inputs(h, w, grid)
    out = AC.host_forward(host, image, AC.identity(grid))
    assert out.tobytes() == image.tobytes()                           # the image's bits
    v_image, _ = AC.host_backward(host, image, AC.identity(grid), v_out)
    assert np.array_equal(v_image, v_out)                             # (equal values: -0 comes back as +0)
    m = np.random.default_rng(5).standard_normal(12).astype(np.float32)
    out = AC.host_forward(host, image, np.broadcast_to(m, grid + (12,)).copy())
    r, g, b = image[..., 0], image[..., 1], image[..., 2]
    want = np.stack([((m[4 * q] * r + m[4 * q + 1] * g) + m[4 * q + 2] * b) + m[4 * q + 3] for q in range(3)], axis=2)
    assert out.tobytes() == want.astype(np.float32).tobytes()         # the constant's affine map, no interpolation error


def test_workspace_size_is_a_function_of_the_shapes(host):
    from tinysplat_amd import _lib
    lib = _lib.load()
    for h, w, grid in AC.CASES + ((1080, 1920, AC.DEFAULT), (1, 1, (1, 1, 1)), (9, 65, (2, 40, 40))):
        assert lib.ts_appearance_ws_bytes(h, w, *grid) == host.ah_ws_bytes(h, w, *grid) > 0
    # 1080p, default grid: 30 x 135 tiles of 64 x 8 pixels; a cell is 128 x 72 pixels, so that no tile straddles a cell border
    # and each reaches 2 x 2 vertex columns of 8 x 12 doubles
    assert lib.ts_appearance_ws_bytes(1080, 1920, 8, 16, 16) == 30 * 135 * 4 * 96 * 8
    assert lib.ts_appearance_ws_bytes(1080, 1900, 8, 16, 16) == 30 * 135 * 6 * 96 * 8      # (three where one does)
    assert lib.ts_appearance_ws_bytes(0, 10, 8, 16, 16) == 0 and lib.ts_appearance_ws_bytes(10, 10, 0, 16, 16) == 0
    assert lib.ts_affine_fit_ws_bytes(1080, 1920) == 22 * 8 * -(-1080 * 1920 // 2048) and lib.ts_affine_fit_ws_bytes(0, 5) == 0


# ------------------------------------------------------------------------------------------------------ total variation
@pytest.mark.parametrize("grid", [AC.DEFAULT, (1, 1, 1), (2, 1, 3), (3, 2, 1), (1, 5, 1)], ids=str)
def test_total_variation_against_the_oracle(host, grid):
    G = AC.inputs(37, 53, grid)[1] if grid != (1, 5, 1) else \
        np.random.default_rng(3).standard_normal(grid + (12,)).astype(np.float32)
    want, want_grad = AO.tv(G)
    value, grad = AC.host_tv(host, G)
    assert abs(value - want) <= 1e-13 * max(want, 1.0)               # double sums of at most 24 576 squares
    assert np.all(np.abs(grad - want_grad) <= AC.EPS * np.abs(want_grad) + 1e-18)     # one rounding to float32
    if grid == (1, 1, 1):
        assert value == 0.0 and not grad.any()
    base = np.random.default_rng(4).standard_normal(G.shape).astype(np.float32)
    _, summed = AC.host_tv(host, G, 10.0, base)                       # v_in + weight * gradient, each rounded once
    assert summed.tobytes() == (base + np.float32(10.0) * grad).astype(np.float32).tobytes()
    assert AO.tv(AC.identity(grid))[0] == 0.0 and AC.host_tv(host, AC.identity(grid))[0] == 0.0


# ------------------------------------------------------------------------------------------------------- the affine fit
def test_fit_sums_against_the_oracle(host):
    image, target, u8 = AC.fit_inputs()
    for tgt in (target, u8):
        got, want = AC.host_fit_sums(host, image, tgt), AO.fit_sums(image, tgt)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))     # exact double products, 5063 double sums
    as_float = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    assert AC.host_fit_sums(host, image, u8).tobytes() == AC.host_fit_sums(host, image, as_float).tobytes()


def test_affine_fit_recovers_a_planted_map(host):
    """The sums come from the host build of the kernels' header (the device's sums are its bits:
    tests/test_gpu_appearance.py), the solve is metrics.affine_fit_solve, which metrics.affine_color_fit calls.  The image
    is random on the 2^-8 lattice and M0 on the 2^-4 lattice, so that target = M0 phi is exact in float32."""
    rng = np.random.default_rng(11)
    image = (rng.integers(0, 256, (61, 83, 3)) / 256.0).astype(np.float32)
    M0 = np.array([[14, 1, -1, 1], [1, 20, 1, -2], [-1, 1, 11, 2]], np.float64) / 16.0
    x = np.concatenate([image.astype(np.float64), np.ones(image.shape[:2] + (1,))], axis=2)
    target = (x @ M0.T).astype(np.float32)
    assert np.array_equal(target.astype(np.float64), x @ M0.T)
    sums = AC.host_fit_sums(host, image, target)
    S = np.zeros((4, 4))
    S[np.triu_indices(4)] = sums[:10]
    S = S + np.triu(S, 1).T
    cond = float(np.linalg.cond(S))
    got = M.affine_fit_solve(sums)
    bound = 64 * 2.0 ** -53 * cond * np.abs(M0).max()
    print(f"cond(S) = {cond:.1f}; max |M - M0| = {np.abs(got - M0).max():.3e} (bound {bound:.3e})")
    assert cond < 1e4 and got.shape == (3, 4) and got.dtype == np.float64
    assert np.abs(got - M0).max() <= bound


def test_affine_fit_of_a_single_colour_is_the_minimum_norm_map(host):
    image = np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (20, 30, 3)).copy()
    target = np.broadcast_to(np.array([0.5, 0.25, 1.0], np.float32), (20, 30, 3)).copy()
    got = M.affine_fit_solve(AC.host_fit_sums(host, image, target))
    phi = np.array([0.25, 0.5, 0.75, 1.0])
    want = np.outer([0.5, 0.25, 1.0], phi) / (phi @ phi)              # the least-norm M with M phi = t
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() < 1e-12 and np.abs(got @ phi - [0.5, 0.25, 1.0]).max() < 1e-12


# ------------------------------------------------------------------------------------------ configuration, tools, entries
def test_config_defaults_and_checks():
    cfg = AP.AppearanceConfig()
    assert (cfg.grid, cfg.lr, cfg.betas, cfg.eps, cfg.tv_weight) == ((8, 16, 16), 2e-3, (0.9, 0.999), 1e-15, 10.0)
    assert AP.AppearanceConfig(grid=[1, 1, 1]).grid == (1, 1, 1)
    for bad in (dict(grid=(0, 16, 16)), dict(grid=(8, 16)), dict(lr=-1.0), dict(tv_weight=-1.0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            AP.AppearanceConfig(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AP.apply_grid(torch.zeros(4, 4, 3), torch.zeros(1, 1, 1, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AP.AppearanceModel(2, cfg, device="cpu")
    import inspect
    from tinysplat_amd.training import TrainStep, fit
    assert inspect.signature(fit).parameters["appearance"].default is None
    params = inspect.signature(TrainStep.__call__).parameters
    assert params["appearance"].default is None and params["view"].default is None
    assert inspect.signature(M.evaluate).parameters["color_correct"].default is False


def test_train_tool_appearance_flags():
    tool = _tool("train")
    args = tool.parse_appearance([])
    assert (args.appearance, args.appearance_grid, args.appearance_lr, args.appearance_tv, args.appearance_out) == \
        ("none", [8, 16, 16], 2e-3, 10.0, None)
    assert tool.appearance_config(args) is None
    assert "appearance" not in vars(tool.parse([]))                   # the options live in a namespace of their own
    args = tool.parse_appearance(["--appearance", "affine", "--appearance-out", "a.pt", "--max-iter", "5"])
    assert tool.appearance_config(args).grid == (1, 1, 1) and args.appearance_out == "a.pt"
    args = tool.parse_appearance(["--appearance", "grid", "--appearance-grid", "4", "8", "9", "--appearance-lr", "0.01",
                                  "--appearance-tv", "0"])
    cfg = tool.appearance_config(args)
    assert (cfg.grid, cfg.lr, cfg.tv_weight) == ((4, 8, 9), 0.01, 0.0)
    assert tool.parse(["--appearance", "grid", "--max-iter", "7"]).max_iter == 7
    for bad in (["--appearance", "bilateral"], ["--appearance", "grid", "--appearance-grid", "0", "4", "4"],
                ["--appearance", "grid", "--appearance-lr", "-1"], ["--appearance-out", "a.pt"],
                ["--appearance", "affine", "--appearance-grid", "2", "2", "2"]):
        with pytest.raises(SystemExit):
            tool.parse_appearance(bad)


def test_eval_tool_color_correct_flag():
    tool = _tool("eval")
    assert tool.parse(["scene.ply", "--dataset-dir", "d"]).color_correct is False
    assert tool.parse(["scene.ply", "--dataset-dir", "d", "--color-correct"]).color_correct is True


def test_entries_refuse_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                         # 16-byte aligned host memory: never dereferenced
    assert p % 16 == 0
    good = [4, 5, 2, 2, 2]
    for k in range(5):
        for bad in (0, -3):
            sizes = list(good)
            sizes[k] = bad
            assert lib.ts_appearance_fwd(*sizes, p, p, p, None) == -1
            assert lib.ts_appearance_bwd(*sizes, p, p, p, p, p, p, None) == -1
            assert lib.ts_appearance_ws_bytes(*sizes) == 0
    for missing in range(3):
        ptrs = [p, p, p]
        ptrs[missing] = None
        assert lib.ts_appearance_fwd(*good, *ptrs, None) == -1
    for missing in range(6):
        ptrs = [p] * 6
        ptrs[missing] = None
        assert lib.ts_appearance_bwd(*good, *ptrs, None) == -1
    assert lib.ts_appearance_fwd(*good, p, p + 4, p, None) == -1              # the grid's 16-byte alignment
    for k in range(3):
        for bad in (0, -1):
            sizes = [2, 2, 2]
            sizes[k] = bad
            assert lib.ts_grid_tv(*sizes, p, 1.0, None, p, p, None) == -1
    assert lib.ts_grid_tv(2, 2, 2, None, 1.0, None, p, p, None) == -1
    assert lib.ts_grid_tv(2, 2, 2, p, 1.0, None, None, p, None) == -1
    assert lib.ts_grid_tv(2, 2, 2, p, 1.0, None, p, None, None) == -1
    assert lib.ts_grid_tv(2, 2, 2, p, 1.0, None, p + 4, p, None) == -1        # the double's alignment
    for h, w in ((0, 4), (4, 0), (-1, 4)):
        assert lib.ts_affine_fit_sums(h, w, p, p, 0, p, p, None) == -1 and lib.ts_affine_fit_ws_bytes(h, w) == 0
    for missing in range(4):
        ptrs = [p] * 4
        ptrs[missing] = None
        assert lib.ts_affine_fit_sums(4, 4, ptrs[0], ptrs[1], 0, ptrs[2], ptrs[3], None) == -1
    assert lib.ts_affine_fit_sums(4, 4, p, p + 1, 0, p, p, None) == -1        # a float target on an odd byte
