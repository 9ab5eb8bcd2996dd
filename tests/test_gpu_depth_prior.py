"""The depth prior on the GPU: the sparse lists against the oracle's float32 restatement, batches
against single cameras, the fit against the exact optimum and against the reference's Nelder-Mead run, the targets, and the
whole path from a COLMAP folder with stored maps through ``DepthPriors`` into ``fit`` and the training tool."""
import math
import subprocess
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import colmap_cases as CC
import depth_prior_cases as DC
import depth_prior_oracle as DO
from tinysplat_amd import Dataset, DepthPriors, GaussianRasterizer, PointCloud, from_pcd, match_scale, sparse_depth
from tinysplat_amd.depth import COLUMNS, STATUS, apply_scale, fit_scale
from tinysplat_amd.training import PARAM_ORDER, fit

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"


def _bits(t):
    return t.cpu().numpy().tobytes()


def _world(cases):
    """scene cases -> (cameras, a PointCloud on the GPU holding all their points, the dense maps); ids made unique"""
    ids = [c.ids * 8 + k for k, c in enumerate(cases)]
    pcd = PointCloud(torch.from_numpy(np.concatenate(ids)).to(DEV), torch.from_numpy(np.concatenate([c.xyz for c in cases])).to(DEV),
                     torch.zeros((sum(len(i) for i in ids), 3), dtype=torch.uint8, device=DEV),
                     torch.from_numpy(np.concatenate([c.errors for c in cases])).to(DEV))
    cams = [SimpleNamespace(view_matrix=torch.from_numpy(c.view.copy()), f_x=c.f_x, f_y=c.f_y, width=c.width, height=c.height,
                            visible_point_ids=torch.from_numpy(i).to(DEV), name=c.name) for c, i in zip(cases, ids)]
    return cams, pcd, [torch.from_numpy(c.dense.copy()).to(DEV) for c in cases]


def _check_lists(sparse, k, reference):
    pixel, z, weight = sparse.camera(k)
    ref_pixel, ref_z, ref_w = reference
    assert pixel.dtype == torch.int32 and z.dtype == torch.float32 and weight.dtype == torch.float64
    assert np.array_equal(pixel.cpu().numpy(), ref_pixel)                         # pixels and order
    assert _bits(z) == ref_z.tobytes() and _bits(weight) == ref_w.tobytes()       # z bits, weights


# ------------------------------------------------------------------------------------------------------ the sparse lists
@pytest.mark.parametrize("n", [0, 1, 3, 65, 300, 5000])
@pytest.mark.parametrize("width,height", DC.SIZES)
def test_sparse_lists_against_the_oracle(width, height, n):
    case = DC.scene_case(width, height, n, 1)
    cams, pcd, _ = _world([case])
    sparse = sparse_depth(cams, pcd)
    reference = DC.scene_reference(width, height, n, 1)
    print(f"{width}x{height}, {n} points: {int(sparse.offsets[1])} survivors")
    assert sparse.offsets.tolist() == [0, len(reference[0])] and sparse.x is None
    _check_lists(sparse, 0, reference)
    if n == 5000:                                                # de-duplication did the work / many survivors
        assert len(reference[0]) <= width * height and (len(reference[0]) > 2000 if width == 128 else len(reference[0]) > 900)


def test_a_visible_id_the_cloud_does_not_hold_is_dropped():
    case = DC.scene_case(128, 96, 65, 1)
    cams, pcd, _ = _world([case])
    whole = sparse_depth(cams, pcd)
    extra = torch.tensor([5, (1 << 40) + 1], dtype=torch.int64, device=DEV)       # below and above every id of the cloud
    cams[0].visible_point_ids = torch.cat([extra[:1], cams[0].visible_point_ids, extra[1:]])
    again = sparse_depth(cams, pcd)
    assert _bits(again.pixel) == _bits(whole.pixel) and _bits(again.z) == _bits(whole.z)


# ------------------------------------------------------------------------------------------------------------ batches
@pytest.fixture(scope="module")
def batch():
    cases = [DC.scene_case(*b) for b in DC.BATCH]
    cams, pcd, maps = _world(cases)
    fits, targets = match_scale(maps, cams, pcd)
    return cases, cams, pcd, maps, fits, targets


def test_a_batch_of_seven_cameras(batch):
    cases, cams, pcd, maps, fits, targets = batch
    assert fits.shape == (7, len(COLUMNS)) and fits.dtype == np.float64 and len(targets) == 7
    sparse = sparse_depth(cams, pcd)
    for k, b in enumerate(DC.BATCH):
        reference = DC.scene_reference(*b)
        _check_lists(sparse, k, reference)
        assert fits[k, 3] == len(reference[0])
        assert tuple(targets[k].shape) == (cases[k].height, cases[k].width) and targets[k].dtype == torch.float32
    print("m:", fits[:, 3].tolist(), "evaluations:", fits[:, 4].tolist(), "status:", [STATUS[int(s)] for s in fits[:, 5]])
    assert STATUS[int(fits[2, 5])] == "no_points" and np.isnan(fits[2, :3]).all() and fits[2, 3] == 0
    assert STATUS[int(fits[3, 5])] == "equal_x" and fits[3, 0] == 1.0 and fits[3, 3] == 1
    # the same bytes on a second run
    fits2, targets2 = match_scale(maps, cams, pcd)
    assert fits2.tobytes() == fits.tobytes() and all(_bits(a) == _bits(b) for a, b in zip(targets, targets2))


@pytest.mark.parametrize("k", range(len(DC.BATCH)))
def test_a_camera_alone_gives_the_bytes_it_gives_in_the_batch(batch, k):
    cases, cams, pcd, maps, fits, targets = batch
    alone_fits, alone_targets = match_scale([maps[k]], [cams[k]], pcd)
    assert alone_fits.tobytes() == fits[k:k + 1].tobytes() and _bits(alone_targets[0]) == _bits(targets[k])
    # the fit saw the oracle's x: the dense map at the surviving pixels, bit for bit
    pixel = DC.scene_reference(*DC.BATCH[k])[0]
    if len(pixel) > 1 and np.isfinite(fits[k, 0]):
        x = cases[k].dense.reshape(-1)[pixel]
        y, w = DC.scene_reference(*DC.BATCH[k])[1].astype(np.float64), DC.scene_reference(*DC.BATCH[k])[2]
        f = DO.objective_exact(fits[k, 0], fits[k, 1], x, y, w)
        f_opt = DO.optimum(x, y, w)[0]
        print(f"camera {k}: m {len(pixel)} f {f!r} optimum {f_opt!r} reported {fits[k, 2]!r}")
        assert f <= f_opt + DC.fit_bound(fits[k, 0], x, w, f)


# ---------------------------------------------------------------------------------------------------------------- the fit
@pytest.fixture(scope="module")
def family_fits():
    """every family at every m as the spans of ONE launch -> {(family, m): row}"""
    order = [(family, m) for family in DC.FAMILIES for m in DC.COUNTS]
    x, z, w, offsets = DC.concat_cases([DC.fit_case(*key) for key in order])
    args = [torch.from_numpy(a).to(DEV) for a in (x, z, w, offsets)]
    table = fit_scale(*args).cpu().numpy()
    assert fit_scale(*args).cpu().numpy().tobytes() == table.tobytes()
    return dict(zip(order, table))


@pytest.mark.parametrize("m", DC.COUNTS)
@pytest.mark.parametrize("family", DC.FAMILIES)
def test_fit_against_the_exact_optimum(family_fits, family, m):
    s, t, f_reported, m_out, evaluations, status = family_fits[(family, m)]
    assert m_out == m
    if m == 0:
        assert STATUS[int(status)] == "no_points" and math.isnan(s) and math.isnan(t) and evaluations == 0
        return
    x, z, w = DC.fit_case(family, m)
    y = DC.fit_y(z)
    f_opt, s_opt, t_opt = DC.fit_reference(family, m)
    f = DO.objective_exact(s, t, x, y, w)                       # the kernel's (s, t), judged by the oracle
    bound = DC.fit_bound(s, x, w, f)
    print(f"{family} m={m}: s {s!r} t {t!r} f {f!r} optimum {f_opt!r} (at {s_opt!r}, {t_opt!r}) bound {bound:.3e} "
          f"reported {f_reported!r} evaluations {int(evaluations)} status {STATUS[int(status)]}")
    assert f <= f_opt + bound
    # the kernel's own f: its sum's rounding, and per term the roundings of r_i, t and r_i - t, each half an ulp of a
    # value below max |y| + |s| max |x|
    assert abs(f_reported - f) <= 4 * m * 2.0 ** -53 * f + \
        4 * 2.0 ** -53 * float(np.mean(w)) * (float(np.abs(y).max()) + abs(s) * float(np.abs(x).max()))
    assert 1 <= evaluations <= 1 + 128 + 1100
    if np.all(x == x[0]):                                       # every family at m = 1
        assert STATUS[int(status)] == "equal_x" and s == 1.0 and evaluations == 1
        assert t == DO.weighted_median_lower(y - x.astype(np.float64), w)
    else:
        assert STATUS[int(status)] in ("ok", "adjacent")
    if family == "linear" and m >= 2:
        tol_s, tol_t = DC.linear_bounds(x)
        assert abs(s - DC.LINEAR_A) <= tol_s and abs(t - DC.LINEAR_B) <= tol_t


def test_fit_in_disparity_space():
    x, z, w = (a.copy() for a in DC.fit_case("outliers", 257))
    x = (1.0 / x).astype(np.float32)                            # a disparity map against 1 / z
    offsets = np.array([0, len(x)], dtype=np.int64)
    row = fit_scale(*[torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (x, z, w, offsets)], space="disparity")
    s, t = float(row[0, 0]), float(row[0, 1])
    y = DC.fit_y(z, disparity=True)
    f, f_opt = DO.objective_exact(s, t, x, y, w), DO.optimum(x, y, w)[0]
    print(f"disparity: s {s!r} t {t!r} f {f!r} optimum {f_opt!r}")
    assert f <= f_opt + DC.fit_bound(s, x, w, f)
    dense = torch.from_numpy(DC.scene_case(40, 24, 3, 1).dense.copy()).to(DEV)
    target = apply_scale(dense, row[0], 24, 40, space="disparity")
    assert _bits(target) == DO.apply(s, t, dense.cpu().numpy(), disparity=True).tobytes()


def test_fit_against_the_references_nelder_mead():
    g = dict(np.load(DC.GOLDEN))
    w, h = int(g["width"]), int(g["height"])
    pcd = PointCloud(torch.from_numpy(g["ids"]).to(DEV), torch.from_numpy(g["xyz"]).to(DEV),
                     torch.zeros((len(g["ids"]), 3), dtype=torch.uint8, device=DEV), torch.from_numpy(g["errors"]).to(DEV))
    cam = SimpleNamespace(view_matrix=torch.from_numpy(g["view"]), f_x=float(g["f_x"]), f_y=float(g["f_y"]), width=w,
                          height=h, visible_point_ids=torch.from_numpy(g["ids"]).to(DEV), name="golden")
    sparse = sparse_depth([cam], pcd)
    pixel, z, weight = (a.cpu().numpy() for a in sparse.camera(0))
    assert np.array_equal(pixel, g["ref_row"] * w + g["ref_col"]) and np.array_equal(weight, 1.0 / g["ref_e"])
    assert np.max(np.abs(z.astype(np.float64) - g["ref_z"])) <= DC.z_tolerance(g["view"], g["xyz"])
    fits, targets = match_scale([torch.from_numpy(g["dense"])], [cam], pcd)
    s, t = fits[0, 0], fits[0, 1]
    x = g["dense"].reshape(-1)[pixel]
    f = DO.objective_exact(s, t, x, g["ref_z"], 1.0 / g["ref_e"])             # on the reference's own lists
    print(f"kernel ({s!r}, {t!r}) f {f!r}; Nelder-Mead ({float(g['ref_s'])!r}, {float(g['ref_t'])!r}) "
          f"f {float(g['ref_objective'])!r}; evaluations {int(fits[0, 4])} against {int(g['ref_nfev'])}")
    assert f <= float(g["ref_objective"]) and fits[0, 2] <= float(g["ref_objective"])
    assert _bits(targets[0]) == DO.apply(s, t, g["dense"]).tobytes()


# ------------------------------------------------------------------------------------------------------------ the targets
def test_apply_on_maps_of_the_cameras_size_and_of_twice_it():
    fit_row = torch.tensor([1.6124406361055066, 0.3871563123421506, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    rng = np.random.default_rng(11)
    for width, height in DC.SIZES + ((41, 23),):                 # 41 x 23 = 943 pixels: a tail of 3 after the groups of 4
        same = rng.uniform(0.5, 5.0, (height, width)).astype(np.float32)
        got = apply_scale(torch.from_numpy(same).to(DEV), fit_row, height, width)
        assert _bits(got) == DO.apply(float(fit_row[0]), float(fit_row[1]), same).tobytes()
        double = rng.uniform(0.5, 5.0, (2 * height, 2 * width)).astype(np.float32)
        got = apply_scale(torch.from_numpy(double).to(DEV), fit_row, height, width).cpu().numpy()
        v, u = (a.reshape(-1) for a in np.mgrid[0:height, 0:width])
        sampled = DO.sample_dense(double, height, width, u, v).reshape(height, width)
        want = float(fit_row[0]) * sampled + float(fit_row[1])
        # the sample's float32 error times s, and the target's own rounding
        assert np.max(np.abs(got - want)) <= float(fit_row[0]) * DC.sample_tolerance(2 * height, 2 * width) + 2.0 ** -24 * 9.0
        f32 = DO.sample_dense(double, height, width, u, v, np.float32).reshape(height, width)
        assert got.tobytes() == DO.apply(float(fit_row[0]), float(fit_row[1]), f32).tobytes()


# ------------------------------------------------------------------------------------------------------------ end to end
A, B = 0.5, 0.25                                                # the stored maps: a depth + b
MISSING = "view_e.png"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """a COLMAP folder with images, and the depth of a small model rendered from every camera stored as a depth + b"""
    base = tmp_path_factory.mktemp("depth_scene")
    CC.write(base / "colmap" / "sparse" / "0")
    CC.write_images(base / "images")
    ds = Dataset(base / "colmap" / "sparse" / "0", base / "images", device=DEV)
    model = from_pcd(ds.pcd, sh_degree=1, device=DEV, generator=torch.Generator().manual_seed(0))
    model.background = torch.zeros(3, device=DEV)
    render = GaussianRasterizer(model, ds.cameras, device=DEV)
    (base / "depths").mkdir()
    with torch.no_grad():
        for cam in ds.cameras:
            _image, extras = render(cam, None, model.active_sh_degree)
            depth = extras["depth"].detach().cpu().numpy().astype(np.float32)
            assert depth.shape == (cam.height, cam.width)
            if cam.name != MISSING:
                np.save(base / "depths" / (cam.name + ".npy"), A * depth + B)
    return base, ds


def _fresh(ds):
    return from_pcd(ds.pcd, sh_degree=1, device=DEV, generator=torch.Generator().manual_seed(0))


def _train(ds, steps=6, **kwargs):
    model, seen = _fresh(ds), []
    fit(model, ds.cameras, ds.targets, DEV, max_iter=steps, rng=np.random.default_rng(0),
        generator=torch.Generator().manual_seed(0), on_step=lambda s, o: seen.append(o), **kwargs)
    return model, seen


def test_priors_from_a_folder_train_a_model(folder, tmp_path):
    base, ds = folder
    with pytest.warns(UserWarning, match=f"camera {MISSING} trains without a depth term: no file"):
        priors = DepthPriors(ds, ds.pcd, base / "depths")
    assert len(priors.targets) == len(ds.cameras) == 6 and priors.fits.shape == (6, 6)
    missing = [c.name for c in ds.cameras].index(MISSING)
    print("fits:", priors.fits.tolist(), "reasons:", priors.reasons)
    assert priors.targets[missing] is None and np.isnan(priors.fits[missing]).all()
    used = [i for i, t in enumerate(priors.targets) if t is not None]
    assert used and all(priors.fits[i, 0] > 0 and priors.fits[i, 3] >= 2 for i in used)
    for i in used:
        c = ds.cameras[i]
        assert tuple(priors.targets[i].shape) == (c.height, c.width) and torch.isfinite(priors.targets[i]).all()
    priors.write_csv(tmp_path / "fits.csv")
    assert len((tmp_path / "fits.csv").read_text().splitlines()) == 7
    with warnings.catch_warnings(record=True) as caught:       # fewer survivors than min_points: no target, one line each
        warnings.simplefilter("always")
        few = DepthPriors(ds, ds.pcd, base / "depths", min_points=1000)
    assert few.targets == [None] * 6 and sum("fewer than 1000" in str(w.message) for w in caught) == 5 and len(caught) == 6

    model, seen = _train(ds, depth_targets=priors.targets)
    with_term = [float(o["depth_l1"]) for o in seen if "depth_l1" in o]
    print("depth l1 per step:", with_term, "of", len(seen), "steps")
    assert with_term and all(math.isfinite(v) and v != 0.0 for v in with_term)
    assert all(math.isfinite(float(o["loss"])) for o in seen)
    assert all(torch.isfinite(getattr(model, name)).all() for name in PARAM_ORDER)

    # a camera whose map is missing trains without the term
    lone = _fresh(ds)
    outs = []
    fit(lone, [ds.cameras[missing]], [ds.targets[missing]], DEV, max_iter=2, depth_targets=[priors.targets[missing]],
        rng=np.random.default_rng(0), generator=torch.Generator().manual_seed(0), on_step=lambda s, o: outs.append(o))
    assert len(outs) == 2 and all("depth_l1" not in o and math.isfinite(float(o["loss"])) for o in outs)

    # no targets at all is the unchanged code path, bit for bit; with targets the parameters differ
    plain, _ = _train(ds)
    nothing, _ = _train(ds, depth_targets=[None] * 6)
    for name in PARAM_ORDER:
        assert _bits(getattr(plain, name).detach()) == _bits(getattr(nothing, name).detach())
    assert any(_bits(getattr(plain, name).detach()) != _bits(getattr(model, name).detach()) for name in PARAM_ORDER)


def test_training_tool_with_and_without_the_depth_prior(folder, tmp_path):
    base, ds = folder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        used = sum(t is not None for t in DepthPriors(ds, ds.pcd, base / "depths").targets)     # the tool's own computation
    assert 1 <= used <= 5
    common = [sys.executable, str(ROOT / "tools" / "train.py"), "--dataset-dir", str(base), "--max-iter", "3", "--sh-degree", "1"]
    r = subprocess.run(common + ["--regularize-depth", "--depth-fits-csv", str(tmp_path / "fits.csv"), "--eval-holdout", "3",
                                 "--output", str(tmp_path / "with.ply")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "4 training cameras, 2 held out" in r.stdout        # the depth targets are split with the cameras
    assert f"depth priors for {used} of 6 cameras" in r.stdout and "wrote" in r.stdout and MISSING in r.stderr
    assert (tmp_path / "with.ply").exists() and len((tmp_path / "fits.csv").read_text().splitlines()) == 7
    r = subprocess.run(common + ["--output", str(tmp_path / "without.ply")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "depth priors" not in r.stdout and (tmp_path / "without.ply").exists()
