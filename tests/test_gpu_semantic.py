"""Label votes on the GPU against the exact reference: the per-pixel weights of the existing
forward launch, harvested with one-hot colours (semantic_cases.weight_table), quantised and summed on the host
(semantic_oracle).  The bar is equality."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import semantic_cases as SC  # noqa: E402
import semantic_oracle as SO  # noqa: E402
from tinysplat_amd import semantic as S  # noqa: E402
from tinysplat_amd.synthetic import PinholeCamera  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SCENES = {}


def scene(name):
    """(model on the GPU, camera, table float32 [N, H, W], radii, list length per tile, final_T): built and harvested
    once per session, never changed."""
    if name not in _SCENES:
        if name == "mixed":
            cam, model = SC.mixed_scene()
        elif name == "staging":
            cam, model, _ = SC.staging_scene()
        elif name == "opaque":
            cam, model = SC.opaque_stack()
        elif name == "clusters6":
            cam = SC.camera(96, 64)
            model, _ = SC.clusters_scene(cam, (3, 2), 25, 8)
        else:                                            # "random<seed>"
            seed = int(name[len("random"):])
            cam = SC.camera(40 + 3 * (seed % 5), 24 + 5 * (seed % 3))
            model = SC.random_scene(cam, 60, 100 + seed)
        model = model.to(DEV)
        table, radii = SC.weight_table(model, cam)
        lens, final_T = SC.lists_and_final_T(model, cam)
        for a in (table, radii, lens, final_T):
            a.setflags(write=False)
        _SCENES[name] = (model, cam, table, radii, lens, final_T)
    return _SCENES[name]


def lift(model, cams, maps, class_map, columns, votes=None):
    tensors = None if maps is None else [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in maps]
    cm = None if class_map is None else torch.from_numpy(class_map).to(DEV)
    return S.accumulate_votes(model, cams, tensors, cm, columns, votes)


def check_equal(name, label_map, class_map, columns):
    model, cam, table, *_ = scene(name)
    got = lift(model, [cam], None if label_map is None else [label_map], class_map, columns).cpu().numpy()
    want = SC.expected_votes(table, label_map, class_map, columns)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} entries differ"
    return got


# ------------------------------------------------------------------------------------------------ the vote kernel
def test_ragged_image_and_what_the_mixed_scene_provokes():
    model, cam, table, radii, lens, final_T = scene("mixed")
    h, w = cam.height, cam.width
    assert (w % 16, h % 16) == (2, 5) and table[:, :, 48:].sum() > 0 and table[:, 32:, :].sum() > 0      # ragged tiles vote
    label_map = SC.blocky_map(h, w, range(5), 5, 1, ignore_share=0.1)
    assert (label_map == 255).any()
    got = check_equal("mixed", label_map, SC.identity_map(5), 5)
    # one Gaussian on every tile's list with weight in every tile: twelve waves add to one row
    tiles = [(table[150, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] > 0).any() for ty in range(3) for tx in range(4)]
    assert all(tiles) and (lens >= 1).all() and got[150].sum() > 0
    # the GENERAL path: opacity above 0.99 - above 0.999 even, so that the clamp changes the weight at the centre pixel
    # (alpha there is the opacity: the weight is 0.999 T and the pixel goes on with 0.001 T)
    assert (torch.sigmoid(model.opacities[151:153]) > 0.9995).all()
    z = model.means[:, 2].cpu().numpy()
    for g, (x, y) in ((151, (12, 9)), (152, (40, 30))):
        w = float(table[g, y, x])
        rest = float(table[z > z[g], y, x].astype(np.float64).sum() + final_T[y, x])      # what g left of the pixel
        assert w > 0.5 and abs(rest / w - 0.001 / 0.999) < 1e-4                            # (0.00012 without the clamp)
    # behind the camera, or outside the image: radius 0, no list entry, an empty row
    assert (radii[153:156] == 0).all() and (radii[:153] > 0).sum() > 100
    assert not table[153:156].any() and not got[153:156].any()
    # pixels of the padded tile area beyond the image cannot vote: the votes are the image's weights, no more
    assert got.sum() == SO.quantise(table[:, label_map != 255]).sum()


def test_staging_boundaries():
    model, cam, table, radii, lens, final_T = scene("staging")
    assert lens.tolist() == SC.staging_scene()[2]                # an empty tile, lists of 1, 64, 65 and 130 entries
    assert (final_T > 1e-4).all()                                # nothing stops: the whole of every list is walked
    label_map = SC.blocky_map(cam.height, cam.width, range(3), 8, 2)
    got = check_equal("staging", label_map, SC.identity_map(3), 3)
    assert (got.sum(axis=1) > 0).all()                           # every one of the 195 is blended somewhere


def test_opaque_stack_stops_mid_list():
    model, cam, table, radii, lens, final_T = scene("opaque")
    assert (lens == 13).all() and (radii > 0).all()
    per_gaussian = table.reshape(13, -1).sum(axis=1)
    assert per_gaussian[0] > 0 and not per_gaussian[7:].any()    # listed, but every pixel has stopped before them
    assert table[1, 16, 16] > 0 and table[2, 16, 16] == 0        # the centre pixel stops AT the third: no weight for it
    assert (final_T > 0).all() and (final_T < 0.01).all()
    got = check_equal("opaque", SC.blocky_map(32, 32, range(4), 4, 3, ignore_share=0.2), SC.identity_map(4), 4)
    assert not got[7:].any()


def test_single_label_tiles_and_ignored_tiles():
    model, cam, table, *_ = scene("mixed")
    label_map = SC.blocky_map(cam.height, cam.width, range(5), 3, 4, ignore_share=0.1)
    label_map[:16, :16] = 3                                      # a tile of one label
    label_map[:16, 16:32] = 255                                  # a tile that is ignored altogether
    label_map[16:32, 16:32] = 1
    label_map[16:32, 16:24] = 255                                # one label and ignored pixels
    got = check_equal("mixed", label_map, SC.identity_map(5), 5)
    assert table[:, :16, 16:32].sum() > 0 and got.sum() == SO.quantise(table[:, label_map != 255]).sum()


def test_checker_of_seven_labels():
    model, cam, table, *_ = scene("mixed")
    ys, xs = np.mgrid[:cam.height, :cam.width]
    label_map = ((xs + 3 * ys) % 7).astype(np.uint8)
    assert all(len(np.unique(label_map[ty:ty + 16, tx:tx + 16])) == 7 for ty in (0, 16, 32) for tx in (0, 16, 32, 48))
    got = check_equal("mixed", label_map, SC.identity_map(7), 7)
    assert (got > 0).all(axis=1).sum() > 20                      # many Gaussians vote in all seven columns


def test_label_254_and_255_columns():
    label_map = SC.blocky_map(37, 50, [254, 0, 100], 6, 5, ignore_share=0.1)
    got = check_equal("mixed", label_map, SC.identity_map(255), 255)
    assert got[:, 254].sum() > 0 and got[:, 100].sum() > 0 and not got[:, 1:100].any()


def test_class_map_drops_and_reorders():
    label_map = SC.blocky_map(37, 50, range(3), 4, 6)
    class_map = np.full(256, 255, np.uint8)
    class_map[0], class_map[2] = 1, 0                            # label 1 is dropped, 0 and 2 swap
    got = check_equal("mixed", label_map, class_map, 2)
    full = SC.expected_votes(scene("mixed")[2], label_map, SC.identity_map(3), 3)
    assert np.array_equal(got[:, 0], full[:, 2]) and np.array_equal(got[:, 1], full[:, 0]) and full[:, 1].sum() > 0


def test_150_classes():
    label_map = SC.blocky_map(37, 50, range(150), 4, 7)
    assert len(np.unique(label_map)) > 60
    check_equal("mixed", label_map, SC.identity_map(150), 150)


def test_one_class_without_a_map_and_the_contributions():
    model, cam, table, *_ = scene("mixed")
    got = check_equal("mixed", None, None, 1)
    contributions = S.gaussian_contributions(model, [cam])
    assert contributions.dtype == torch.float64 and contributions.shape == (156,)
    assert np.array_equal(contributions.cpu().numpy(), got[:, 0].astype(np.float64) / 2.0 ** 24)
    exact = table.astype(np.float64).reshape(156, -1).sum(axis=1)
    nonzero = (table > 0).reshape(156, -1).sum(axis=1)
    assert (np.abs(contributions.cpu().numpy() - exact) <= nonzero * 2.0 ** -25).all()      # the quantisation, no more


def test_two_views_any_order_any_batching():
    model, cam_a, table_a, *_ = scene("mixed")
    cam_b = PinholeCamera.look_at_origin_plus_z(40, 48, position=(0.3, 0.1, -0.5))
    table_b, _ = SC.weight_table(model, cam_b)
    assert table_b.sum() > 10
    map_a, map_b = SC.blocky_map(37, 50, range(6), 5, 8, 0.1), SC.blocky_map(48, 40, range(6), 7, 9, 0.1)
    cm = SC.identity_map(6)
    a, b = lift(model, [cam_a], [map_a], cm, 6), lift(model, [cam_b], [map_b], cm, 6)
    ab, ba = lift(model, [cam_a, cam_b], [map_a, map_b], cm, 6), lift(model, [cam_b, cam_a], [map_b, map_a], cm, 6)
    assert torch.equal(ab, a + b) and torch.equal(ab, ba)
    assert torch.equal(ab, lift(model, [cam_a, cam_b], [map_a, map_b], cm, 6))                 # two runs
    assert np.array_equal(b.cpu().numpy(), SC.expected_votes(table_b, map_b, cm, 6))
    start = torch.arange(156 * 6, dtype=torch.int64, device=DEV).reshape(156, 6) * 1000003
    into = lift(model, [cam_b], [map_b], cm, 6, votes=start.clone())
    assert torch.equal(into, start + b)                                                        # accumulated, not overwritten


@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(seed):
    model, cam, table, *_ = scene(f"random{seed}")
    columns = (3, 5, 17)[seed % 3]
    label_map = SC.blocky_map(cam.height, cam.width, range(columns), 2 + seed, 50 + seed, ignore_share=0.05 * (seed % 4))
    got = check_equal(f"random{seed}", label_map, SC.identity_map(columns), columns)
    assert (got.sum(axis=1) > 0).sum() > 20


def test_telescoping():
    model, cam, table, _, _, final_T = scene("mixed")
    label_map = SC.blocky_map(37, 50, range(4), 5, 10)                       # no ignored pixel
    got = lift(model, [cam], [label_map], SC.identity_map(4), 4).cpu().numpy()
    lhs = float(got.sum()) / 2.0 ** 24                                         # (an integer below 2^53: exact)
    rhs = float((1.0 - final_T.astype(np.float64)).sum())
    nonzero = int((table > 0).sum())
    print(f"sum of votes / 2^24 = {lhs!r}, sum of 1 - final_T = {rhs!r}, difference {abs(lhs - rhs):.3e}, "
          f"bound {nonzero} * 2^-25 = {nonzero * 2.0 ** -25:.3e}")
    assert abs(lhs - rhs) <= nonzero * 2.0 ** -25


# -------------------------------------------------------------------------------------------------- labels from votes
@pytest.mark.parametrize("min_share", SC.MIN_SHARES)
def test_votes_labels_against_numpy(min_share):
    r = np.random.default_rng(12)
    big = r.integers(0, 1 << 40, size=(700, 150))
    big[r.random(700) < 0.1] = 0
    for rows in (SC.vote_rows(), big, big[:, :1].copy()):
        labels, conf = S.labels_from_votes(torch.from_numpy(rows).to(DEV), min_share)
        want = SO.labels_from_votes(rows, min_share)
        assert labels.dtype == torch.uint8 and conf.dtype == torch.float32
        assert np.array_equal(labels.cpu().numpy(), want[0]) and conf.cpu().numpy().tobytes() == want[1].tobytes()
    rows = SC.vote_rows()
    labels, conf = S.labels_from_votes(torch.from_numpy(rows).to(DEV), 0.25)
    labels, conf = labels.cpu().numpy(), conf.cpu().numpy()
    assert labels[1] == 1 and labels[2] == 0 and labels[4] == 255 and conf[4] == 0.0           # ties; an empty row
    assert labels[5] == 0 and conf[5] == np.float32(0.25)                                      # top == min_share * total


# ------------------------------------------------------------------------------------------------- rendering and IoU
def test_render_labels_against_the_table():
    model, cam, table, _, lens, _ = scene("clusters6")
    n = model.means.shape[0]
    labels = np.repeat(np.arange(6, dtype=np.uint8), 25)
    labels[::9] = 255                                            # some Gaussians carry no label
    got = S.render_labels(model, cam, torch.from_numpy(labels).to(DEV), 6).cpu().numpy()
    sums = SO.class_sums(table, labels, 6)
    want, margin = SO.rendered_labels(sums)
    per_pixel_len = np.kron(lens.reshape(4, 6), np.ones((16, 16), np.int64))[:cam.height, :cam.width]
    # a pixel where the two largest class sums are closer than the float32 sums' error bound decides nothing (a pixel
    # without any weight is 255 on both sides and stays in)
    excluded = (margin < per_pixel_len * 2.0 ** -24) & (sums.max(axis=0) > 0)
    print(f"{int(excluded.sum())} of {excluded.size} pixels excluded; {int((want != 255).sum())} labelled")
    assert n == 150 and excluded.mean() <= 0.02
    assert np.array_equal(got[~excluded], want[~excluded])
    assert len(np.unique(want[want != 255])) == 6 and (want == 255).any()


def test_label_iou_on_the_gpu():
    r = np.random.default_rng(13)
    pred = r.integers(0, 9, size=(64, 96)).astype(np.uint8)
    target = r.integers(0, 8, size=(64, 96)).astype(np.uint8)
    pred[r.random(pred.shape) < 0.1] = 255
    target[r.random(pred.shape) < 0.2] = 255
    iou, mean = S.label_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), 10)
    want, want_mean = SO.iou(pred, target, 10)
    assert np.array_equal(iou.cpu().numpy(), want, equal_nan=True) and abs(mean - want_mean) < 1e-12


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(f"tool_{name}", str(Path(__file__).resolve().parent.parent / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_export_and_eval_tools_on_a_synthetic_dataset(tmp_path, capsys):
    """tools/export.py --semantic-dir keeps exactly the Gaussians lift_labels assigns to the kept class, and tools/eval.py
    --semantic-dir prints an mIoU line (in-process: the tools' main(argv))."""
    import colmap_cases as CC
    from tinysplat_amd import Dataset, formats, from_pcd
    base = tmp_path / "scene"
    CC.write(base / "colmap" / "sparse" / "0")
    CC.write_images(base / "images")
    ds = Dataset(base / "colmap" / "sparse" / "0", base / "images", device=DEV)
    model = from_pcd(ds.pcd, sh_degree=1, device=DEV, generator=torch.Generator().manual_seed(0))
    formats.export_ply(model, tmp_path / "in.ply")
    (base / "semantic").mkdir()
    ys, xs = np.mgrid[:CC.H, :CC.W]
    for cam in ds.cameras:                                          # left half 1, right half 2, a band of ignored pixels
        m = np.where(xs < CC.W // 2, 1, 2).astype(np.int64)
        m[:4] = 255
        np.save(base / "semantic" / (cam.name + ".npy"), m)
    export, evaluate = _tool("export"), _tool("eval")
    export.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--filetype", "PLY", "--device", DEV, "--dataset-dir",
                 str(base), "--semantic-dir", str(base / "semantic"), "--semantic-classes", "3", "--keep-classes", "1"])
    loaded = formats.load_ply(tmp_path / "in.ply", DEV)
    cams = export.dataset_cameras(str(base), "colmap/sparse/0")
    lifted = S.lift_labels(loaded, None, S.SemanticMaps(cams, base / "semantic", num_classes=3, device=DEV))
    keep = lifted.labels == 1
    out = formats.load_ply(tmp_path / "out.ply", DEV)
    assert 0 < int(keep.sum()) < 60 and out.num_points == int(keep.sum()) and torch.equal(out.means, loaded.means[keep])
    export.main([str(tmp_path / "in.ply"), str(tmp_path / "rest.ply"), "--filetype", "PLY", "--device", DEV, "--dataset-dir",
                 str(base), "--semantic-dir", str(base / "semantic"), "--semantic-classes", "3", "--drop-classes", "1"])
    assert formats.load_ply(tmp_path / "rest.ply", DEV).num_points == 60 - int(keep.sum())
    capsys.readouterr()
    evaluate.main([str(tmp_path / "in.ply"), "--dataset-dir", str(base), "--device", DEV, "--holdout", "3",
                   "--semantic-dir", str(base / "semantic"), "--semantic-classes", "3"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("semantic: mIoU")]
    assert len(line) == 1 and "2 views" in line[0] and "4 training views" in line[0]
    assert 0.0 <= float(line[0].split()[2]) <= 1.0


def test_end_to_end_two_clusters():
    cam0 = SC.camera(64, 48)
    model, truth = SC.clusters_scene(cam0, (2, 1), 60, 3)
    model = model.to(DEV)
    truth_t = torch.from_numpy(truth).to(DEV)
    cams = [PinholeCamera.look_at_origin_plus_z(64, 48, position=p)
            for p in ((0.0, 0.0, 0.0), (0.15, 0.0, 0.0), (-0.15, 0.05, 0.0), (0.0, -0.1, -0.2))]
    maps = [S.render_labels(model, c, truth_t, 2) for c in cams]
    assert all((m == 0).any() and (m == 1).any() and (m == 255).any() for m in maps)
    lifted = S.lift_labels(model, cams, maps, class_map=torch.from_numpy(SC.identity_map(2)), num_classes=2)
    voted = lifted.votes.sum(dim=1) > 0
    assert int(voted.sum()) > 100 and torch.equal(lifted.labels[voted], truth_t[voted])
    assert (lifted.labels[~voted] == 255).all() and lifted.class_ids == [0, 1]
    only = S.select_gaussians(model, lifted.labels == 0)
    assert only.num_points == int((lifted.labels == 0).sum()) and torch.equal(only.means, model.means[lifted.labels == 0])
    for c, m in zip(cams, maps):
        drawn = S.render_labels(only, c, torch.zeros(only.num_points, dtype=torch.uint8, device=DEV), 1) != 255
        assert drawn.any() and (m[drawn] == 0).all()             # nothing outside the pixels of class 0
