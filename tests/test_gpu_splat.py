""".splat export and import on the GPU (csrc/splatfile.hip) against the float64 oracle
(tests/splat_oracle.py) under the byte rule: a byte equals the oracle's, or differs by one where the oracle's value before
truncation lies within eps of an integer; the oracle alone decides which.  The launches do not cap their grid (one thread
per record, no stride loop), so the sizes below - partial waves, partial blocks, several blocks - are every path."""
import functools

import numpy as np
import pytest
import torch

import splat_cases as SC
import splat_oracle as SO
from tinysplat_amd import formats
from tinysplat_amd.synthetic import SplatModel, make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [0, 1, 63, 64, 65, 257, 2000]


@functools.lru_cache(maxsize=None)
def _scene(n):
    """n random Gaussians; at 2000 the edge rules' rows replace the first ones."""
    scene = SC.random_scene(n, seed=100 + n)
    if n >= 2000:
        edges, _ = SC.edge_scene()
        for k in scene:
            scene[k][:edges[k].shape[0]] = edges[k]
    return scene


def _model(scene, k_rest=0, seed=0):
    t = {k: torch.from_numpy(v).to(DEV) for k, v in scene.items()}
    n = scene["means"].shape[0]
    rest = 0.1 * torch.randn((n, k_rest, 3), generator=torch.Generator().manual_seed(seed)).to(DEV)
    return SplatModel(t["means"], t["colors_dc"], rest, t["scales"], t["quats"], t["opacities"],
                      active_sh_degree=formats.deg_from_sh(k_rest + 1))


def _arrays(model):
    return {k: getattr(model, k).detach().cpu().numpy() for k in ("means", "scales", "colors_dc", "opacities", "quats")}


# ------------------------------------------------------------------------------------------------ keys, order, records
@pytest.mark.parametrize("n", SIZES)
def test_keys_order_and_records(n):
    scene = _scene(n)
    model = _model(scene)
    keys, order = formats.splat_order(model)
    assert keys.shape == (n,) and keys.dtype == torch.float32 and order.shape == (n,) and order.dtype == torch.int64
    keys, order = keys.cpu().numpy(), order.cpu().numpy()
    print()
    SC.check_keys(keys, scene["scales"], scene["opacities"], f"n={n}")
    assert np.array_equal(order, SO.order(keys))                      # numpy's stable argsort of the returned keys
    plain = formats.splat_records(model, order=None)
    assert plain.shape == (n, 32) and plain.dtype == torch.uint8 and plain.is_cuda
    plain = plain.cpu().numpy()
    rec, pre = SO.encode(*SC.args(scene))
    assert np.array_equal(plain[:, :12], scene["means"].view(np.uint8).reshape(n, 12))     # positions: the bits
    SC.check_exp_scales(plain, scene["scales"], f"n={n}")
    if n >= 257:
        SO.compare_bytes(plain, rec, pre, f"n={n}")
    else:                                                               # too few bytes for a share: the flips are still ruled
        diff = plain[:, 24:].astype(np.int16) - rec[:, 24:].astype(np.int16)
        assert not ((diff != 0) & ~(SO.excused(pre[:, 24:]) & (np.abs(diff) == 1))).any()
    ranked = formats.splat_records(model).cpu().numpy()
    assert np.array_equal(ranked, plain[order])
    for limit in (0, 1, n // 2, n, n + 5):
        m = min(n, limit)
        assert np.array_equal(formats.splat_records(model, limit=limit).cpu().numpy(), ranked[:m])
        assert np.array_equal(formats.splat_records(model, order=None, limit=limit).cpu().numpy(), plain[:m])
    assert np.array_equal(formats.splat_records(model).cpu().numpy(), ranked)              # a second call: the same bytes


def test_edge_rules_on_the_device():
    edges, names = SC.edge_scene()
    got = formats.splat_records(_model(edges), order=None).cpu().numpy()
    e = {k: got[i, 24:].tolist() for k, i in names.items()}
    assert e["clip_below"][:4] == [0, 0, 0, 0] and e["clip_above"][:4] == [255, 255, 255, 255]
    assert e["inf_color"][:2] == [255, 0] and e["nan_color"][:3] == [0, 127, 0] and e["nan_opacity"][3] == 0
    for k in ("zero_quat", "nan_quat", "inf_quat", "identity"):
        assert e[k][4:] == [255, 128, 128, 128], k
    assert e["tiny_quat"][4:] == e["plain"][4:] == e["huge_quat"][4:] and e["plain"][4:] != [255, 128, 128, 128]
    assert e["negative_w"][4:] == [0, 128, 128, 128] and e["negative_w_mixed"][4] < 128
    rec, pre = SO.encode(*SC.args(edges))
    diff = got[:, 24:].astype(np.int16) - rec[:, 24:].astype(np.int16)
    assert not ((diff != 0) & ~(SO.excused(pre[:, 24:]) & (np.abs(diff) == 1))).any()


def test_duplicates_keep_index_order_and_nan_goes_last():
    scene = {k: v.copy() for k, v in SC.random_scene(300, seed=7).items()}
    twins = [250, 13, 77, 140, 3]
    for k in scene:
        scene[k][twins] = scene[k][twins[0]]                            # bit-identical Gaussians
    scene["opacities"][[40, 9]] = np.nan
    keys, order = formats.splat_order(_model(scene))
    keys, order = keys.cpu().numpy(), order.cpu().numpy()
    assert len(set(keys[twins].tolist())) == 1
    places = np.flatnonzero(np.isin(order, twins))
    assert order[places].tolist() == sorted(twins) and np.all(np.diff(places) == 1)
    assert order[-2:].tolist() == [9, 40] and np.isnan(keys[[9, 40]]).all() and not np.isnan(keys[order[:-2]]).any()
    assert np.array_equal(order, SO.order(keys)) and np.all(np.diff(keys[order[:-2]]) <= 0)


def test_colors_rest_does_not_reach_the_file():
    scene = _scene(2000)
    bare, full = _model(scene), _model(scene, k_rest=15, seed=3)
    assert full.active_sh_degree == 3 and full.colors_rest.abs().max() > 0
    assert torch.equal(formats.splat_records(full), formats.splat_records(bare))
    # tensors that are not contiguous go through a copy, as ply_records' do
    wide = torch.zeros((2000, 6), device=DEV)
    wide[:, ::2] = bare.means
    strided = SplatModel(wide[:, ::2], bare.colors_dc, bare.colors_rest, bare.scales, bare.quats, bare.opacities, 0)
    assert not strided.means.is_contiguous()
    assert torch.equal(formats.splat_records(strided), formats.splat_records(bare))


# ------------------------------------------------------------------------------------------------ file and load
@pytest.mark.parametrize("n,limit", [(0, None), (1, None), (65, None), (2000, None), (2000, 700)])
def test_file_and_load(n, limit, tmp_path):
    scene = _scene(n)
    model = _model(scene, k_rest=3 if n else 0)
    path = tmp_path / "scene.splat"
    formats.export_splat(model, path, limit=limit)
    m = n if limit is None else min(n, limit)
    blob = path.read_bytes()
    want = formats.splat_records(model, limit=limit).cpu().numpy()
    assert len(blob) == 32 * m and blob == want.tobytes()
    back = formats.load_splat(path, DEV)
    assert back.colors_rest.shape == (m, 0, 3) and back.active_sh_degree == 0 and back.num_points == m
    assert all(getattr(back, f).dtype == torch.float32 and getattr(back, f).is_cuda for f in formats.FIELDS)
    assert back.opacities.shape == (m, 1) and back.quats.shape == (m, 4) and back.scales.shape == (m, 3)
    print()
    SC.check_decoded(_arrays(back), want, f"n={n}")


def test_decode_edge_records_on_the_device(tmp_path):
    rec = SC.decode_edge_records()
    (tmp_path / "edges.splat").write_bytes(rec.tobytes())
    got = _arrays(formats.load_splat(tmp_path / "edges.splat", DEV))
    print()
    SC.check_decoded(got, rec, "edges")
    log_min = float(np.log(np.float32(SO.FLT_MIN)))
    assert np.abs(got["scales"][:2] - log_min).max() < 1e-4             # scale 0, negative, NaN, subnormal: log(FLT_MIN)
    assert got["opacities"][0, 0] == got["opacities"][2, 0] and got["opacities"][1, 0] == got["opacities"][3, 0]


def test_value_round_trip(tmp_path):
    """load_splat(export_splat(model)) against the model.  Truncation loses up to one unit of a byte; the float32
    evaluation may sit SO.EPS below the exact value (the byte rule's derivation), so the bars are (1 + EPS) / 255 and
    (1 + EPS) / 128.  The file holds clipped colours, so the model's colour is clipped to [0, 1] first; its quaternion is
    normalised (in float64) and compared with the file's, which load_splat does not renormalise."""
    model = make_scene(2000, 3, 64, 64, seed=9)[0].to(DEV)
    path = tmp_path / "scene.splat"
    formats.export_splat(model, path)
    order = formats.splat_order(model)[1].cpu().numpy()
    src = {k: v[order].astype(np.float64) for k, v in _arrays(model).items()}
    back = formats.load_splat(path, DEV)
    got = {k: v.astype(np.float64) for k, v in _arrays(back).items()}
    assert np.array_equal(got["means"], src["means"])
    unit = 1.0 + SO.EPS
    colour = lambda dc: np.clip(0.5 + SO.C0 * dc, 0.0, 1.0)
    d_col = np.abs(colour(src["colors_dc"]) - colour(got["colors_dc"])).max()
    sig = lambda o: 1.0 / (1.0 + np.exp(-o))
    alpha = np.frombuffer(path.read_bytes(), np.uint8).reshape(-1, 32)[:, 27]
    d_alpha = np.abs(sig(src["opacities"]) - sig(got["opacities"]))[:, 0]
    clamped = (alpha == 0) | (alpha == 255)
    qn = src["quats"] / np.linalg.norm(src["quats"], axis=1, keepdims=True)
    d_quat = np.abs(qn - got["quats"]).max()
    print(f"\nround trip: colour {d_col * 255:.4f} / 255, alpha {d_alpha[~clamped].max() * 255:.4f} / 255 "
          f"({int(clamped.sum())} clamped), quaternion {d_quat * 128:.4f} / 128")
    assert d_col <= unit / 255 and d_quat <= unit / 128
    assert (d_alpha[~clamped] <= unit / 255).all() and (d_alpha[clamped] <= 2 * unit / 255).all()
    assert np.isfinite(got["opacities"]).all() and np.isfinite(got["scales"]).all()


# ------------------------------------------------------------------------------------------------ render and refusals
def test_loaded_scene_renders(tmp_path):
    from tinysplat_amd import Scene
    model, cam = make_scene(2000, 3, 64, 64, seed=4, scale_mult=3.0)
    formats.export_splat(model.to(DEV), tmp_path / "scene.splat")
    loaded = formats.load_splat(tmp_path / "scene.splat", DEV)
    with torch.no_grad():
        rgb, _ = Scene([cam], loaded, device=DEV).render(cam)
    assert rgb.shape == (64, 64, 3) and torch.isfinite(rgb).all() and rgb.max() > 0


def test_cpu_tensors_are_refused():
    model = make_scene(10, 0, 64, 64)[0]
    with pytest.raises(RuntimeError):
        formats.splat_records(model)                                    # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        formats.splat_order(model)
    with pytest.raises(RuntimeError):
        formats.export_splat(model, "unused.splat")
