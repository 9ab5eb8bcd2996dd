"""Point-cloud initialisation on the GPU (tinysplat_amd.init): from_pcd against the reference's own from_pcd
(tests/golden/init_*.npz, tests/golden/make_init_fixtures.py), knn_points against the float64 brute-force
oracle on the clouds that stress a grid search, at 1 M points, run to run, and a training run started from it."""
import numpy as np
import pytest
import torch

from helpers import GOLD
from knn_oracle import knn_oracle
from tinysplat_amd import PointCloud, from_pcd, knn_points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 20_000


def ulps(a, b):
    """float32 distance in units in the last place (same-sign finite values)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _fixture_model(name):
    z = np.load(GOLD / f"init_{name}.npz")
    n = z["xyz"].shape[0]
    pcd = PointCloud(torch.arange(n), torch.from_numpy(z["xyz"]), torch.from_numpy(z["colors"]), torch.zeros(n))
    model = from_pcd(pcd, sh_degree=int(z["sh_degree"]), device=DEV,
                     generator=torch.Generator().manual_seed(int(z["seed"])))
    return z, model


@pytest.mark.parametrize("name", ["n600", "n4"])
def test_from_pcd_matches_the_reference(name):
    z, m = _fixture_model(name)
    got = {f: getattr(m, f).detach().cpu().numpy() for f in
           ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")}
    assert np.array_equal(got["means"], z["means"])
    assert np.array_equal(m.mean_dist.cpu().numpy(), z["mean_dist"])               # exp(scales) before the log
    inf = np.isinf(z["scales"])
    assert np.array_equal(np.isinf(got["scales"]), inf) and (got["scales"][inf] < 0).all()
    assert ulps(got["scales"][~inf], z["scales"][~inf]).max() <= 1
    assert (got["scales"] == got["scales"][:, :1]).all()
    assert ulps(got["colors_dc"], z["colors_dc"]).max() <= 1
    assert ulps(got["opacities"], z["opacities"]).max() <= 1
    assert np.abs(got["quats"] - z["quats"]).max() <= 3e-7
    assert got["colors_rest"].shape == z["colors_rest"].shape and not got["colors_rest"].any()
    assert m.active_sh_degree == 1 == int(z["active_sh_degree"]) and m.max_sh_degree == int(z["max_sh_degree"])
    if name == "n600":
        assert inf[:, 0].sum() == 11


def test_from_pcd_float64_points():
    z, m = _fixture_model("n300_f64")
    assert np.array_equal(m.means.cpu().numpy(), z["means"])
    rel = np.abs(np.exp(m.scales.cpu().double().numpy()) / np.exp(z["scales"].astype(np.float64)) - 1.0)
    assert rel.max() <= 1e-6, rel.max()


def cloud(kind, n=N, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)                                   # noqa: E731
    if kind == "uniform":
        return r(n, 3)
    if kind == "plane":
        p = r(n, 3)
        p[:, 2] = 0.5 + 1e-5 * r(n)
        return p
    if kind == "clusters":
        c = r(n // 100, 3)
        return c.repeat_interleave(100, 0)[:n] + 1e-3 * torch.randn(n, 3, generator=g)
    if kind == "duplicates":
        return r(n // 4, 3).repeat(4, 1)
    if kind == "collinear":
        return torch.tensor([0.3, -1.2, 2.0]) + r(n, 1) * torch.tensor([1.0, 2.0, -0.5])
    if kind == "outliers":
        p = r(n, 3)
        d = torch.randn(20, 3, generator=g)
        p[:20] = d / d.norm(dim=1, keepdim=True) * 1e4
        return p
    if kind == "identical":
        return torch.full((n, 3), 0.25)
    raise ValueError(kind)


def queries_for(pts, m=3000, seed=1):
    g = torch.Generator().manual_seed(seed)
    sel = torch.randint(0, pts.shape[0], (m,), generator=g)
    return pts[sel] + 0.01 * torch.randn(m, 3, generator=g) * (pts.std(dim=0) + 1e-3)


KINDS = ["uniform", "plane", "clusters", "duplicates", "collinear", "outliers", "identical"]
_runs = {}


def _run(kind, self_search, k):
    pts = cloud(kind)
    qs = pts if self_search else queries_for(pts)
    p = pts.to(DEV)
    q = p if self_search else qs.to(DEV)
    d, i, st = knn_points(q, p, k, return_stats=True)
    return pts, qs, d.cpu(), i.cpu(), st.cpu()


@pytest.mark.parametrize("self_search", [True, False], ids=["self", "queries"])
@pytest.mark.parametrize("kind", KINDS)
def test_knn_points_is_exact(kind, self_search):
    pts, qs, _, _, _ = _run(kind, self_search, 1)
    od, oi = knn_oracle(qs, pts, 16)
    for k in (1, 4, 16):
        _, _, d, i, st = _run(kind, self_search, k)
        assert d.dtype == torch.float32 and i.dtype == torch.int64 and d.shape == (qs.shape[0], k)
        assert torch.equal(i, oi[:, :k]), (kind, k, int((i != oi[:, :k]).any(dim=1).sum()))
        assert torch.equal(d, od[:, :k].float()), (kind, k)
        _, _, d2, i2, st2 = _run(kind, self_search, k)                            # run to run: bit-identical
        assert torch.equal(d, d2) and torch.equal(i, i2) and torch.equal(st, st2)
        _runs[(kind, self_search, k)] = st
    if self_search and kind == "uniform":
        assert all(int(_runs[(kind, True, k)][0]) == 0 for k in (1, 4, 16))       # no brute force on a uniform cloud
    if self_search and kind == "outliers":
        # the far points took the fallback (k = 1 is settled in the point's own cell: it is its own nearest point)
        assert all(int(_runs[(kind, True, k)][0]) >= 20 for k in (4, 16))


def test_knn_points_at_one_million_points():
    n = 1_000_000
    g = torch.Generator().manual_seed(3)
    uv = torch.rand(n, 2, generator=g) * 2 - 1
    z = 0.2 * torch.sin(3 * uv[:, :1]) * torch.cos(2 * uv[:, 1:])
    pts = torch.cat([uv, z], dim=1)
    d = torch.randn(100, 3, generator=g)
    pts[:100] = d / d.norm(dim=1, keepdim=True) * 500.0
    sel = torch.randperm(n, generator=g)[:2000]
    sel[:10] = torch.arange(10)                                                      # some of the outliers too
    p = pts.to(DEV)
    od, oi = knn_oracle(pts[sel], pts, 16)
    for k in (4, 16):
        dist, idx, st = knn_points(p, p, k, return_stats=True)
        dist2, idx2, st2 = knn_points(p, p, k, return_stats=True)
        assert torch.equal(dist, dist2) and torch.equal(idx, idx2) and torch.equal(st, st2)
        assert torch.equal(idx[sel.to(DEV)].cpu(), oi[:, :k])
        assert torch.equal(dist[sel.to(DEV)].cpu(), od[:, :k].float())
        assert int(st[0].item()) >= 100 and int(st[0].item()) < n // 100, st


def test_knn_points_rejects_bad_input():
    p = torch.rand(10, 3, device=DEV)
    with pytest.raises(ValueError):
        knn_points(p, p, 17)
    with pytest.raises(ValueError):
        knn_points(p, p, 11)
    with pytest.raises(ValueError):
        knn_points(p.double(), p.double(), 4)
    bad = p.clone()
    bad[3, 0] = float("inf")
    with pytest.raises(ValueError):
        knn_points(bad, p, 4)


def test_training_starts_from_a_point_cloud():
    from tinysplat_amd.densify import DensifyConfig, Densifier
    from tinysplat_amd.rasterizer import GaussianRasterizer
    from tinysplat_amd.synthetic import SH2RGB, PinholeCamera, make_scene
    from tinysplat_amd.training import fit
    w, h = 160, 120
    truth, cam0 = make_scene(4000, 1, w, h, seed=21, scale_mult=4.0)
    cams = [cam0, PinholeCamera.look_at_origin_plus_z(w, h, position=(0.3, 0.0, 0.0)),
            PinholeCamera.look_at_origin_plus_z(w, h, position=(-0.3, 0.1, 0.0))]
    tdev = truth.to(DEV)
    tdev.background = torch.zeros(3, device=DEV)
    with torch.no_grad():
        r = GaussianRasterizer(tdev, None, device=torch.device(DEV))
        targets = [r(c, None, 1)[0].clone() for c in cams]
    g = torch.Generator().manual_seed(4)
    sel = torch.randperm(4000, generator=g)[:2500]
    colors = (SH2RGB(truth.colors_dc[sel]).clamp(0, 1) * 255).round().to(torch.uint8)
    pcd = PointCloud(torch.arange(2500), truth.means[sel].double(), colors, torch.zeros(2500))
    model = from_pcd(pcd, sh_degree=1, device=DEV, generator=torch.Generator().manual_seed(5))
    assert torch.isfinite(model.scales).all()
    losses = []
    dens = Densifier(model, DensifyConfig(warmup_densify=50, warmup_grad=20, interval_densify=50, tau_means=1e-6))
    fit(model, cams, targets, DEV, 200, sh_increment_interval=100, max_sh_degree=model.max_sh_degree, densifier=dens,
        rng=np.random.default_rng(0), generator=torch.Generator().manual_seed(0),
        on_step=lambda s, o: losses.append(float(o["loss"])))
    assert len(losses) == 200 and all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), (losses[:10], losses[-10:])
