"""The depth prior without a GPU: the oracle against the reference's own run (the golden fixture),
the host build of csrc/depth_prior_math.h against the oracle, the new symbols, the wrappers' refusals and the training
tool's flags."""
import ctypes
import importlib.util
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import depth_prior_cases as DC
import depth_prior_oracle as DO

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("ts_depth_prior_project", "ts_depth_prior_mark", "ts_depth_prior_gather", "ts_depth_prior_fit",
           "ts_depth_prior_apply")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return DC.build_host(tmp_path_factory.mktemp("depth_prior_host"))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(DC.GOLDEN))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", str(ROOT / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ the oracle and the reference
def test_oracle_reproduces_the_references_sparse_lists(golden):
    g = golden
    w, h = int(g["width"]), int(g["height"])
    assert DO.boundary_distance(g["view"], float(g["f_x"]), float(g["f_y"]), w, h, g["xyz"].astype(np.float32)) > 1e-3
    for dtype in (np.float32, np.float64):
        fx, fy = (np.float32(g["f_x"]), np.float32(g["f_y"])) if dtype is np.float32 else (float(g["f_x"]), float(g["f_y"]))
        row, col, z, e = DO.sparse(g["view"], fx, fy, w, h, g["xyz"].astype(np.float32), g["errors"], dtype)
        assert np.array_equal(row, g["ref_row"]) and np.array_equal(col, g["ref_col"])       # pixels and order: exactly
        assert np.array_equal(e, g["ref_e"])                                                 # the last point won
        # z: the reference's is a float32 matrix product, whose summation order (and use of fma) is the BLAS's
        assert len(row) == 166 and np.max(np.abs(z.astype(np.float64) - g["ref_z"])) <= DC.z_tolerance(g["view"], g["xyz"])
    assert len(set(zip(g["ref_row"].tolist(), g["ref_col"].tolist()))) == len(g["ref_row"]) < len(g["ids"])


def test_oracle_optimum_is_no_worse_than_the_references_nelder_mead(golden):
    g = golden
    x = g["dense"][g["ref_row"], g["ref_col"]].astype(np.float64)
    y, w = g["ref_z"], 1.0 / g["ref_e"]
    f_opt, s, t = DO.optimum(x, y, w)
    f_nm = DO.objective(float(g["ref_s"]), float(g["ref_t"]), x, y, w)
    print(f"optimum {f_opt!r} at ({s!r}, {t!r}); Nelder-Mead {f_nm!r} (recorded {float(g['ref_objective'])!r}) "
          f"at ({float(g['ref_s'])!r}, {float(g['ref_t'])!r}) after {int(g['ref_nfev'])} evaluations")
    assert f_opt <= f_nm and f_opt <= float(g["ref_objective"])
    assert abs(f_nm - float(g["ref_objective"])) < 1e-6 * f_nm          # (the reference sums partly in float32)
    assert DO.objective_exact(s, t, x, y, w) == pytest.approx(f_opt, rel=1e-13)
    # t is a weighted median of the residuals at s, and no line through two points is better
    assert DO.objective(s, DO.weighted_median_lower(y - s * x, w), x, y, w) <= f_opt * (1 + 1e-12)


def test_oracle_optimum_brute_force_and_lp_agree():
    x, z, w = DC.fit_case("outliers", 257)
    brute = DO.optimum(x, DC.fit_y(z), w)
    old, DO.BRUTE_FORCE_MAX = DO.BRUTE_FORCE_MAX, 10
    try:
        lp = DO.optimum(x, DC.fit_y(z), w)
    finally:
        DO.BRUTE_FORCE_MAX = old
    assert lp[0] == pytest.approx(brute[0], rel=1e-12) and lp[0] >= brute[0] * (1 - 1e-15)
    x, z, w = DC.fit_case("linear", 64)
    f, s, t = DO.optimum(x, DC.fit_y(z), w)
    assert f == 0.0 and s == DC.LINEAR_A and t == DC.LINEAR_B
    x, z, w = DC.fit_case("equal_x", 65)
    f, s, t = DO.optimum(x, DC.fit_y(z), w)
    assert s == 1.0 and t == DO.weighted_median_lower(DC.fit_y(z) - 2.5, w)
    assert DO.weighted_median_lower([3.0, 1.0, 2.0], [1.0, 1.0, 2.0]) == 2.0
    assert DO.weighted_median_lower([3.0, 1.0, 2.0, 4.0], [1.0, 1.0, 1.0, 1.0]) == 2.0      # the lower of the two


# -------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("width,height,n", [(40, 24, 5000), (128, 96, 5000), (128, 96, 300)])
def test_host_projection_and_key_order_against_the_oracle(host, width, height, n):
    c = DC.scene_case(width, height, n, 1)
    cam, cam_p = DC.host_camera(c)
    xyz = c.xyz.astype(np.float32)
    keys, zs = [], np.zeros(n, np.float32)
    z_out = ctypes.c_float()
    for i in range(n):
        pixel = host.dh_project(cam_p, width, height, xyz[i, 0], xyz[i, 1], xyz[i, 2], c.errors[i], ctypes.byref(z_out))
        zs[i] = z_out.value
        keys.append(host.dh_key(0, pixel, i))
    px, py, z, keep = DO.project(c.view, np.float32(c.f_x), np.float32(c.f_y), width, height, xyz, c.errors, np.float32)
    pixels = np.array([host.dh_key_pixel(k) for k in keys])
    assert np.array_equal(pixels != host.dh_no_pixel(), keep) and 0.6 * n < keep.sum() < n
    assert np.array_equal(pixels[keep], (py[keep] * width + px[keep]).astype(np.int64))
    assert zs.tobytes() == z.astype(np.float32).tobytes()
    # sorted keys, the last of every (camera, pixel) run: the oracle's survivors in the oracle's order
    order = np.argsort(np.array(keys, dtype=np.int64), kind="stable")
    runs = np.array([host.dh_key_run(keys[i]) for i in order])
    last = np.concatenate([runs[1:] != runs[:-1], [True]]) & (pixels[order] != host.dh_no_pixel())
    ref_pixel, ref_z, ref_w = DC.scene_reference(width, height, n, 1)
    assert np.array_equal(pixels[order][last], ref_pixel) and zs[order][last].tobytes() == ref_z.tobytes()
    assert np.array_equal(1.0 / c.errors[order][last], ref_w)
    assert len(ref_pixel) < keep.sum()                                   # some points collided


def test_host_key_fields_and_rounding(host):
    no = host.dh_no_pixel()
    assert no == (1 << 28) - 1
    key = host.dh_key(32767, no - 1, (1 << 20) - 1)
    assert 0 < key < 1 << 63 and host.dh_key_camera(key) == 32767 and host.dh_key_pixel(key) == no - 1
    assert host.dh_key(3, 17, 5) < host.dh_key(3, 17, 6) < host.dh_key(3, 18, 0) < host.dh_key(3, no, 0) < host.dh_key(4, 0, 0)
    # half to even: x / z f_x + W / 2 = 2.5 and 3.5 land on 2 and 4; the identity view
    cam = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 8.0, 8.0], dtype=np.float32)
    p, z = cam.ctypes.data_as(DC.F32P), ctypes.c_float()
    for x, want in ((-1.5 / 8, 2), (-0.5 / 8, 4), (-4.5 / 8, 0), (3.5 / 8, 8)):
        got = host.dh_project(p, 8, 6, x, 0.0, 1.0, 1.0, ctypes.byref(z))
        assert got == (no if want == 8 else 3 * 8 + want), (x, got)           # row 3 = rint(0 + 6 / 2); column 8 is outside
    for z_in, err in ((0.0, 1.0), (-1.0, 1.0), (math.inf, 1.0), (math.nan, 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, math.inf),
                      (1.0, math.nan)):
        assert host.dh_project(p, 8, 6, 0.0, 0.0, z_in, err, ctypes.byref(z)) == no
    assert host.dh_project(p, 8, 6, 0.0, 0.0, 2.0, 0.5, ctypes.byref(z)) == 3 * 8 + 4 and z.value == 2.0


def test_host_sampling_against_the_oracle(host):
    rng = np.random.default_rng(3)
    for (h, w), (height, width) in (((24, 40), (24, 40)), ((48, 80), (24, 40)), ((13, 21), (24, 40)), ((96, 128), (48, 64)),
                                    ((1, 1), (5, 7))):
        dense = rng.uniform(0.5, 5.0, (h, w)).astype(np.float32)
        v, u = (a.reshape(-1) for a in np.mgrid[0:height, 0:width])
        got = np.array([host.dh_sample(dense.ctypes.data_as(DC.F32P), h, w, height, width, int(a), int(b))
                        for a, b in zip(u, v)], dtype=np.float32)
        f32 = DO.sample_dense(dense, height, width, u, v, np.float32)
        assert got.tobytes() == np.asarray(f32, dtype=np.float32).tobytes()
        f64 = DO.sample_dense(dense, height, width, u, v, np.float64)
        assert np.max(np.abs(got - f64)) <= DC.sample_tolerance(h, w)
        if (h, w) == (height, width):
            assert got.tobytes() == dense.tobytes()
    # align_corners=False, edge clamp: torch's own bilinear resize
    dense = rng.uniform(0.5, 5.0, (48, 80)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(dense)[None, None], size=(24, 40), mode="bilinear",
                                           align_corners=False)[0, 0].numpy()
    v, u = (a.reshape(-1) for a in np.mgrid[0:24, 0:40])
    assert np.allclose(DO.sample_dense(dense, 24, 40, u, v).reshape(24, 40), want, rtol=0, atol=1e-5)


def test_host_order_keys_and_apply(host):
    values = [-math.inf, -1e300, -2.5, -1e-310, -0.0, 0.0, 1e-310, 1.0, 1.0 + 2.0 ** -52, 3e300, math.inf]
    keys = [host.dh_order_key(v) for v in values]
    assert keys[4] == keys[5] and sorted(keys) == keys and len(set(keys)) == len(values) - 1
    assert [host.dh_order_value(k) for k in keys] == [v + 0.0 for v in values]
    rng = np.random.default_rng(4)
    dense = rng.uniform(0.5, 5.0, 200).astype(np.float32)
    s, t = 1.6124406361055066, 0.3871563123421506
    for disparity in (0, 1):
        got = np.array([host.dh_apply(s, t, float(d), disparity) for d in dense], dtype=np.float32)
        assert got.tobytes() == DO.apply(s, t, dense, bool(disparity)).tobytes()


# ----------------------------------------------------------------------------------------------- the symbols, the wrappers
def test_new_symbols_are_declared_exported_and_bound():
    from tinysplat_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tinysplat_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 9 and lib.ts_abi_version() == 9
    import tinysplat_amd
    for name in ("DepthPriors", "SparseDepth", "match_scale", "sparse_depth"):
        assert name in tinysplat_amd.__all__ and hasattr(tinysplat_amd, name)
    src = (ROOT / "tinysplat_amd" / "depth.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(oracle|scipy)", src, flags=re.M)


def test_entries_refuse_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.ts_depth_prior_project(-1, 4, 4, *([p] * 9), None) == -1
    assert lib.ts_depth_prior_project((1 << 15) + 1, 4, 4, *([p] * 9), None) == -1
    assert lib.ts_depth_prior_project(0, 4, 4, *([p] * 9), None) == -1           # entries but no camera
    assert lib.ts_depth_prior_project(2, 0, 4, *([None] * 9), None) == 0          # nothing to do
    for missing in (0, 1, 4, 5, 6, 7, 8):
        ptrs = [p] * 9
        ptrs[missing] = None
        assert lib.ts_depth_prior_project(1, 4, 4, *ptrs, None) == -1
    assert lib.ts_depth_prior_mark(-1, p, p, None) == -1 and lib.ts_depth_prior_mark(4, None, p, None) == -1
    assert lib.ts_depth_prior_mark(0, None, None, None) == 0
    assert lib.ts_depth_prior_gather(4, p, p, p, p, p, p, None, None, None, p, p, p, None, None) == -1   # no camera sizes
    assert lib.ts_depth_prior_gather(4, p, p, p, p, p, p, p, None, p, p, p, p, p, None) == -1            # maps, no sizes
    assert lib.ts_depth_prior_gather(0, *([None] * 13), None) == 0
    assert lib.ts_depth_prior_fit(-1, p, p, p, p, 0, p, None) == -1 and lib.ts_depth_prior_fit(0, *([None] * 4), 0, None, None) == 0
    assert lib.ts_depth_prior_fit(1, None, p, p, p, 0, p, None) == -1 and lib.ts_depth_prior_fit(1, p, p, p, p, 0, p + 4, None) == -1
    assert lib.ts_depth_prior_apply(None, 4, 4, 4, 4, p, 0, p, None) == -1
    assert lib.ts_depth_prior_apply(p, 0, 4, 4, 4, p, 0, p, None) == -1 and lib.ts_depth_prior_apply(p, 4, 4, 4, 0, p, 0, p, None) == -1
    assert lib.ts_depth_prior_apply(p, 4, 4, 1 << 14, 1 << 14, p, 0, p, None) == -1            # 2^28 pixels
    assert lib.ts_depth_prior_apply(p, 4, 4, 4, 4, p, 0, p + 8, None) == -1                   # the vector stores


def test_wrappers_refuse_cpu_tensors_and_unknown_spaces(tmp_path):
    from tinysplat_amd import DepthPriors, PointCloud, match_scale, sparse_depth
    from tinysplat_amd.depth import fit_scale
    c = DC.scene_case(40, 24, 3, 1)
    pcd = PointCloud(torch.from_numpy(c.ids.copy()), torch.from_numpy(c.xyz.copy()), torch.zeros(3, 3, dtype=torch.uint8),
                     torch.from_numpy(c.errors.copy()))
    cam = type("Cam", (), dict(view_matrix=torch.from_numpy(c.view.copy()), f_x=c.f_x, f_y=c.f_y, width=40, height=24,
                               visible_point_ids=torch.from_numpy(c.ids.copy()), name="a.png"))()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_depth([cam], pcd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match_scale([torch.ones(24, 40)], [cam], pcd)
    with pytest.raises(ValueError, match="space"):
        match_scale([torch.ones(24, 40)], [cam], pcd, space="inverse")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_scale(torch.ones(3), torch.ones(3), torch.ones(3, dtype=torch.float64), torch.tensor([0, 3]))
    with pytest.warns(UserWarning, match="a.png trains without a depth term: no file"):
        priors = DepthPriors([cam], pcd, tmp_path)                     # no file: nothing reaches the GPU
    assert priors.targets == [None] and len(priors) == 1 and np.isnan(priors.fits).all()
    priors.write_csv(tmp_path / "fits.csv")
    lines = (tmp_path / "fits.csv").read_text().splitlines()
    assert lines[0] == "name,s,t,objective,m,evaluations,status,used" and lines[1] == "a.png,nan,nan,nan,,,,0"


# ------------------------------------------------------------------------------------------------------------ the tool
def test_train_tool_depth_flags():
    tool = _tool("train")
    d = tool.parse_depth([])
    assert vars(d) == {"regularize_depth": False, "depths_path": "depths", "lambda_depth": 0.2, "regularize_depth_start": 1,
                       "regularize_depth_end": 15000, "depth_space": "depth", "depth_fits_csv": None}
    argv = ["--regularize-depth", "--depths-path", "mono", "--lambda-depth", "0.5", "--regularize-depth-start", "10",
            "--regularize-depth-end", "200", "--depth-space", "disparity", "--depth-fits-csv", "f.csv", "--max-iter", "3"]
    d = tool.parse_depth(argv)
    assert (d.regularize_depth, d.depths_path, d.lambda_depth, d.regularize_depth_start, d.regularize_depth_end,
            d.depth_space, d.depth_fits_csv) == (True, "mono", 0.5, 10, 200, "disparity", "f.csv")
    assert tool.parse(argv).max_iter == 3                                # the other flags parse as before
    for bad in (["--depth-space", "log"], ["--lambda-depth", "-1", "--regularize-depth"], ["--depth-fits-csv", "f.csv"],
                ["--regularize-depth", "--regularize-depth-start", "5", "--regularize-depth-end", "4"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    assert "without its depth prior" not in tool.__doc__ and "--regularize-depth" in tool.__doc__
